"""The shapes by which the matmul tests reach every matmul kernel, and the route each turbo shape must be planned onto.

tests/test_gpu_matmul_edges.py multiplies these shapes on the GPU; tests/test_gemm_route_host.py asserts, on the CPU, that gemm_plan
(web-rwkv-gguf_amd/csrc/wrk_gemm_route.h) sends every turbo row to the kernel named here -- so a routing edit that moves a row onto another
kernel fails a test instead of silently thinning the GPU file's coverage.

path -> (kinds, [(k, m, T)], turbo, env, route).  route: None for the turbo-off paths (the matvec / dmv kernels: wrk_matvec.hip,
wrk_dmv.hip launch_dmv), else the kernel of the launch:
    "ksplit<NT,NW>"  gemm_kernel<NT, NW>            "pair"         gemm_pair_kernel<4>
    "tile1"          gemm_tile_kernel               "tile2"        gemm_tile2_kernel<4>
    "tile3"          xsum_kernel + gemm_tile3_kernel, K not split
    "tile3_split"    xsum_kernel + gemm_tile3_kernel (grid.z) + t3_reduce_kernel
"""
K4 = ("Q4_K", "Q5_K")
GG = ("Q4_K", "Q5_K", "Q6_K", "Q8_0", "F16")
PLANES = ("INT8", "NF4")

PATHS = {
    "vec1": (GG, [(512, 12, 1), (8192, 8, 1)], False, {}, None),
    "vecT": (GG, [(512, 20, 2), (512, 20, 3), (1024, 20, 4)], False, {}, None),
    "ks14": (GG, [(512, 64, 5)], True, {}, "ksplit<1,4>"),
    "ks18": (GG, [(4096, 64, 16)], True, {}, "ksplit<1,8>"),
    "ks24": (GG, [(512, 32, 17)], True, {}, "ksplit<2,4>"),
    "ks28": (GG, [(4096, 32, 40)], True, {}, "ksplit<2,8>"),
    "ks44": (GG, [(512, 32, 100)], True, {}, "ksplit<4,4>"),
    "pair": (("Q4_K", "Q5_K", "F16"), [(512, 6416, 5), (512, 6416, 16)], True, {"WRK_GEMM_PAIR": "1"}, "pair"),
    "tile1": (("Q4_K", "Q5_K", "Q6_K", "F16"), [(512, 2052, 100)], True, {}, "tile1"),
    "tile2": (("Q8_0", "F16"), [(512, 516, 520)], True, {}, "tile2"),
    "tile2_k4": (K4, [(512, 516, 520)], True, {"WRK_GEMM_TILE3": "0"}, "tile2"),
    "tile2_q8_48": (("Q8_0",), [(256, 4100, 48)], True, {}, "tile2"),
    "tile3": (K4, [(2048, 132, 515), (2560, 132, 515), (8192, 132, 515)], True, {}, "tile3"),
    "tile3_split": (K4, [(8192, 132, 140), (4096, 132, 128)], True, {}, "tile3_split"),
    "plane_vec": (PLANES, [(512, 12, 1), (2048, 8, 3)], False, {}, None),
    "plane_mfma": (PLANES, [(512, 32, 33)], True, {}, "ksplit<2,4>"),
}
