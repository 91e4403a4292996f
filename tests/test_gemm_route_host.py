"""The MFMA GEMM routing planner (web-rwkv-gguf_amd/csrc/wrk_gemm_route.h gemm_plan), on the CPU.

tests/host/gemm_route_main.cpp includes the two HIP-free headers alone (wrk_matjob.h, wrk_gemm_route.h), builds for every case below the
dense MatJobs that wrk_op_matmul or a runner builds, and prints the plan.  It is built with the host compiler under the address and
undefined-behaviour sanitizers, linked into the program: a stand-alone executable that runs the same whatever the environment preloads.

Every expectation here is worked by hand from the routing rules as DESIGN.md and the measurement comments document them -- never read off
the planner -- with the reason next to the row.  Row tiles: 16 rows (K-split kernel), 64 (K-sliced row groups, tile1, tile2), 128 (tile3);
a 256-block is 256 elements of K."""
import json
import os
import shutil
import subprocess

import pytest

from matmul_paths import PATHS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIG_KS = (1 << 24, 4096)            # a K-slice scratch no case outgrows (floats, counters)


@pytest.fixture(scope="module")
def planner(tmp_path_factory):
    cxx = shutil.which("g++")
    assert cxx, "the host compiler g++ is required"
    exe = str(tmp_path_factory.mktemp("gemm_route") / "gemm_route")
    cmd = [cxx, "-std=c++17", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "web-rwkv-gguf_amd", "csrc"),
           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan", "-Wall", "-Werror", "-g",
           os.path.join(ROOT, "tests", "host", "gemm_route_main.cpp"), "-o", exe]
    built = subprocess.run(cmd, capture_output=True, text=True)
    assert built.returncode == 0, built.stderr

    def plan(cases):
        """cases: [(tokens, (ks_part_cap, ks_cnt_cap) or None, xsum_cap, switches, jobs)] -> one plan per case"""
        lines = []
        for i, (n, ks, xsum, sw, jobs) in enumerate(cases):
            ks = ks or (0, 0)
            lines.append(f"c{i} {n} {ks[0]} {ks[1]} {xsum} {sw or '-'} {';'.join(jobs)}")
        ran = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True)
        assert ran.returncode == 0, ran.stdout + ran.stderr
        out = [json.loads(line) for line in ran.stdout.splitlines()]
        assert len(out) == len(cases), ran.stdout + ran.stderr
        return out
    return plan


def op_scratch(k, m, n):
    """what wrk_op_matmul reserves before a turbo launch of >= 128 tokens on a Q4_K / Q5_K matrix (wrk_api.hip)"""
    return n * (k // 32) * 4 + n * 4 + 1024 + (n * m * (k // 256) * 4 if n <= 256 else 0)


def name_of(p):
    """the route names of tests/matmul_paths.py, for a plan with ONE launch"""
    routes = set(p["route"])
    assert len(routes) == 1, p
    r = routes.pop()
    if r == "ksplit":
        return "pair" if p["split"]["pair"] else f"ksplit<{p['split']['nt']},{p['split']['nw']}>"
    if r == "tile3":
        return "tile3_split" if p["t3"]["kslices"] > 1 else "tile3"
    return r


SWITCH_OF = {"WRK_GEMM_PAIR": "pair", "WRK_GEMM_TILE3": "tile3", "WRK_GEMM_KS": "ks", "WRK_T3_SPLIT": "t3split"}


def test_every_turbo_path_of_the_matmul_tests(planner):
    """wrk_op_matmul's job: one matrix, dense [K, T, 1] input, no K-slice scratch, the context's tile3 scratch as the op reserved it."""
    cases, want = [], []
    for path, (kinds, shapes, turbo, env, route) in PATHS.items():
        if not turbo:
            assert route is None
            continue
        sw = ",".join(f"{SWITCH_OF[k]}={v}" for k, v in env.items())
        for kind in kinds:
            for k, m, T in shapes:
                scratch = op_scratch(k, m, T) if T >= 128 and kind in ("Q4_K", "Q5_K") else 0
                cases.append((T, None, scratch, sw, [f"{kind}:{k}:{m}"]))
                want.append((path, kind, k, m, T, route))
    for p, (path, kind, k, m, T, route) in zip(planner(cases), want):
        assert p["ok"] and p["n"] == T and p["wg_begin"] == [0], (path, kind, p)
        assert name_of(p) == route, (path, kind, k, m, T, p)


def test_workgroup_counts_of_the_matmul_tests(planner):
    """The grid x of one row per kernel: ceil(m / tile rows) -- 16 for the K-split kernel, 32 for the pair kernel, 64 for the tiles, 128
    for tile3 -- and tile3's token tiles and K slices."""
    cases = [(5, None, 0, "", ["Q4_K:512:64"]),                                       # 64 / 16
             (16, None, 0, "pair=1", ["Q5_K:512:6416"]),                              # 6416 / 32 = 200.5
             (100, None, 0, "", ["Q6_K:512:2052"]),                                   # 2052 / 64 = 32.06
             (48, None, 0, "", ["Q8_0:256:4100"]),                                    # 4100 / 64 = 64.06
             (515, None, op_scratch(2560, 132, 515), "", ["Q4_K:2560:132"]),          # 132 / 128 -> 2 row tiles, 515 / 128 -> 5 token tiles
             (140, None, op_scratch(8192, 132, 140), "", ["Q4_K:8192:132"]),          # 2 x 2 tiles x 32 blocks = 128 < 160 even at one block per slice
             (128, None, op_scratch(4096, 132, 128), "", ["Q5_K:4096:132"])]          # 2 x 1 tiles x 16 blocks
    p = planner(cases)
    assert [q["wgs"]["ksplit"] for q in p[:2]] == [4, 201]
    assert p[2]["wgs"]["tile1"] == 33 and p[3]["wgs"]["tile2"] == 65
    assert (p[4]["wgs"]["tile3"], p[4]["t3"]["ttiles"], p[4]["t3"]["kslices"]) == (2, 5, 1)
    assert (p[5]["wgs"]["tile3"], p[5]["t3"]["ttiles"], p[5]["t3"]["bps"], p[5]["t3"]["kslices"]) == (2, 2, 1, 32)
    assert (p[6]["wgs"]["tile3"], p[6]["t3"]["ttiles"], p[6]["t3"]["bps"], p[6]["t3"]["kslices"]) == (2, 1, 1, 16)


def test_k_sliced_rules(planner):
    """A runner's launch: the K-slice scratch rides on job 0.  LDS = 16 nt tokens x (bps x 256 + 8) f16."""
    ffn_value, wide, q8 = ["Q4_K:8192:2048"], ["Q4_K:2048:8192"], ["Q8_0:2048:2048"]
    cases = [
        # up to 16 tokens only few row tiles x long rows: 128 tiles of 16 < 256, K >= 4096.  4 blocks per slice: 32 row groups x 8 slices = 256 workgroups
        (16, BIG_KS, 0, "", ffn_value),
        # 17 .. 32 tokens: every eligible launch, two token tiles; nt x bps <= 4 -> 2 blocks: 32 x 16 = 512 workgroups
        (24, BIG_KS, 0, "", ffn_value),
        # beyond 32 tokens none; 32 tiles of 64 x 64 < 96 at K > 2560: no tile kernel; 128 row tiles < 256 and K >= 4096: deep
        (48, BIG_KS, 0, "", ffn_value),
        # 512 row tiles of 16 >= 256: not for the K-sliced kernel at <= 16 tokens; not deep
        (16, BIG_KS, 0, "", wide),
        # 24 tokens: every eligible launch; 2 blocks per slice: 128 row groups x 4 slices
        (24, BIG_KS, 0, "", wide),
        # Q8_0 launches always; candidates from 2 blocks: 32 x 4 = 128 < 256 workgroups -> 1 block: 32 x 8
        (8, BIG_KS, 0, "", q8),
        # WRK_GEMM_KS=0: none -> the K-split kernel, deep
        (16, BIG_KS, 0, "ks=0", ffn_value),
        # WRK_GEMM_KS=2: every eligible launch, also the one of 512 row tiles; 4 blocks: 128 row groups x 2 slices = 256
        (16, BIG_KS, 0, "ks=2", wide),
        # no scratch: never
        (16, None, 0, "", ffn_value),
        # scratch one float short of 32 row groups x 8 slices x 64 rows x 16 tokens: not taken
        (16, (32 * 8 * 64 * 16 - 1, 4096), 0, "", ffn_value),
        (16, (32 * 8 * 64 * 16, 32), 0, "", ffn_value),
        (16, (32 * 8 * 64 * 16, 31), 0, "", ffn_value),     # one counter short of 32 row groups
        # WRK_KS_BPS=2 forces two blocks per slice: 32 row groups x 16 slices
        (16, BIG_KS, 0, "bps=2", ffn_value),
        # a group: r, k, v of a D = 2048 layer at 24 tokens: 2 blocks per slice (3 x 32 x 4 = 384 workgroups), row groups side by side
        (24, BIG_KS, 0, "", ["Q4_K:2048:2048", "Q4_K:2048:2048", "Q6_K:2048:2048"]),
        # the edges of "few row tiles x long rows" at 16 tokens: 256 tiles of 16 are not few (and 256 workgroups not deep) ...
        (16, BIG_KS, 0, "", ["Q4_K:4096:4096"]),
        # ... K = 4096 is long: 16 blocks, 4 per slice give 32 x 4 = 128 < 256 workgroups, 2 per slice 32 x 8 = 256
        (16, BIG_KS, 0, "", ["Q4_K:4096:2048"]),
    ]
    p = planner(cases)

    def ks(q):
        return name_of(q), q["ks"]["nt"], q["ks"]["bps"], q["wgs"]["ksliced"], q["ks"]["lds"]
    assert ks(p[0]) == ("ksliced", 1, 4, 256, 16 * 1032 * 2) and p[0]["ks"]["nslices"] == [8]
    assert ks(p[1]) == ("ksliced", 2, 2, 512, 32 * 520 * 2) and p[1]["ks"]["nslices"] == [16]
    assert name_of(p[2]) == "ksplit<2,8>"
    assert name_of(p[3]) == "ksplit<1,4>" and p[3]["wgs"]["ksplit"] == 512
    assert ks(p[4]) == ("ksliced", 2, 2, 512, 32 * 520 * 2) and p[4]["ks"]["nslices"] == [4]
    assert ks(p[5]) == ("ksliced", 1, 1, 256, 16 * 264 * 2) and p[5]["ks"]["nslices"] == [8]
    assert name_of(p[6]) == "ksplit<1,8>"
    assert ks(p[7]) == ("ksliced", 1, 4, 256, 16 * 1032 * 2) and p[7]["ks"]["nslices"] == [2]
    assert name_of(p[8]) == "ksplit<1,8>"
    assert name_of(p[9]) == "ksplit<1,8>"
    assert name_of(p[10]) == "ksliced"
    assert name_of(p[11]) == "ksplit<1,8>"
    assert ks(p[12]) == ("ksliced", 1, 2, 512, 16 * 520 * 2) and p[12]["ks"]["nslices"] == [16]
    assert ks(p[13]) == ("ksliced", 2, 2, 384, 32 * 520 * 2)
    assert name_of(p[14]) == "ksplit<1,4>"
    assert ks(p[15]) == ("ksliced", 1, 2, 256, 16 * 520 * 2) and p[15]["ks"]["nslices"] == [8]
    assert p[13]["wg_begin"] == [0, 128, 256] and p[13]["ks"]["rg_begin"] == [0, 32, 64] and p[13]["ks"]["nslices"] == [4, 4, 4]


def sums_bytes(n, k):
    """tile3's input sums of one input: hi and lo f16 [n][K / 32], f32 factors [n], each rounded up to 256 bytes"""
    def up(b):
        return (b + 255) // 256 * 256
    return 2 * up(n * (k // 32) * 2) + up(n * 4)


def test_tile3_token_windows(planner):
    """Taken for n >= 512, for 128 < n <= 256 and for n = 128 with K >= 4096; Q4_K / Q5_K with m >= 128 only; needs its scratch."""
    big = 1 << 30
    cases = [
        (512, None, big, "", ["Q4_K:2048:2048"]),       # >= 512: taken, four token tiles: no K split
        (200, None, big, "", ["Q4_K:2048:2048"]),       # 128 < n <= 256: taken; 16 x 2 tiles x 8 blocks = 256 >= 160 only at one block per slice
        (256, None, big, "", ["Q5_K:2048:2048"]),
        (128, None, big, "", ["Q4_K:2048:2048"]),       # n = 128 and K < 4096: not taken; 32 x 2 = 64 tiles at K <= 2560: tile1 (tile2 from 512 tokens)
        (128, None, big, "", ["Q4_K:4096:2048"]),       # n = 128 and K >= 4096: taken; 16 tiles x 16 blocks = 256
        (384, None, big, "", ["Q4_K:2048:2048"]),       # three token tiles: not taken; 32 x 6 tiles >= 96: tile1
        (127, None, big, "", ["Q4_K:2048:2048"]),       # below 128: not taken
        (512, None, big, "", ["Q6_K:2048:2048"]),       # Q4_K / Q5_K only; Q6_K has no tile2 body: tile1
        (512, None, big, "", ["Q4_K:2048:124"]),        # m < 128: not taken; 2 x 8 tiles < 64: no tile kernel at all
        (512, None, 0, "", ["Q4_K:2048:2048"]),         # no scratch: the second-generation tile
        (512, None, big, "tile3=0", ["Q4_K:2048:2048"]),
        (128, None, big, "", ["Q4_K:4096:8192"]),       # 64 x 1 tiles: four blocks per slice fill the chip (64 x 4 = 256 >= 160)
        (200, None, big, "t3split=0", ["Q4_K:2048:2048"]),
    ]
    p = planner(cases)
    assert [name_of(q) for q in p] == ["tile3", "tile3_split", "tile3_split", "tile1", "tile3_split", "tile1", "tile1", "tile1", "ksplit<4,4>",
                                       "tile2", "tile2", "tile3_split", "tile3"]
    assert (p[0]["wgs"]["tile3"], p[0]["t3"]["ttiles"]) == (16, 4)
    assert (p[1]["t3"]["bps"], p[1]["t3"]["kslices"]) == (1, 8) and (p[4]["t3"]["bps"], p[4]["t3"]["kslices"]) == (1, 16)
    assert (p[11]["t3"]["bps"], p[11]["t3"]["kslices"]) == (4, 4)


def test_tile3_scratch_layout_and_fit(planner):
    """The sum arrays of an input, then (K split) the f32 partial tiles [slice][token][row] of every job from the next 256-byte boundary.
    Sums one byte short: the launch is planned as tile2 from the start.  Partials one byte short: tile3 without the split."""
    s512 = sums_bytes(512, 2048)
    assert s512 == 2 * 65536 + 2048
    s200 = sums_bytes(200, 2048)
    part200 = 8 * 200 * 2048 * 4                    # 8 slices of one block
    one = ["Q4_K:2048:2048"]
    # r, k read one shifted input each (here: k and v share input 7), all K = 2048
    three = ["Q4_K:2048:2048:in5", "Q4_K:2048:2048:in7", "Q5_K:2048:2048:in7"]
    cases = [(512, None, s512, "", one), (512, None, s512 - 1, "", one),
             (200, None, s200 + part200, "", one), (200, None, s200 + part200 - 1, "", one),
             (512, None, 2 * s512, "", three), (512, None, 2 * s512 - 1, "", three)]
    p = planner(cases)
    assert name_of(p[0]) == "tile3" and (p[0]["t3"]["sh"], p[0]["t3"]["sl"], p[0]["t3"]["ts"]) == ([0], [65536], [131072])
    assert name_of(p[1]) == "tile2" and p[1]["wgs"]["tile2"] == 32 and p[1]["wgs"]["tile3"] == 0
    assert name_of(p[2]) == "tile3_split" and p[2]["t3"]["part"] == [s200]
    assert name_of(p[3]) == "tile3" and p[3]["t3"]["kslices"] == 1
    assert name_of(p[4]) == "tile3" and p[4]["wg_begin"] == [0, 16, 32] and p[4]["wgs"]["tile3"] == 48
    assert p[4]["t3"]["sums_of"] == [0, 1, 1] and p[4]["t3"]["sh"] == [0, s512, s512] and p[4]["t3"]["ts"] == [131072, s512 + 131072, s512 + 131072]
    assert name_of(p[5]) == "tile2" and p[5]["wg_begin"] == [0, 32, 64]


def test_gemm_ok_rejections(planner):
    """Any job that is not for the MFMA path sends the whole group back to the caller (its -2)."""
    good = "Q4_K:512:64"
    cases = [(16, None, 0, "", [good]),
             (16, None, 0, "", ["Q4_K:512:64:xpad"]),       # input rows K + 4 elements apart: not 16-byte aligned
             (16, None, 0, "", ["F16:48:64"]),              # K % 32
             (16, None, 0, "", ["Q4_K:512:64:round"]),      # MATRIX_ROUND_F16 lives in the matvec kernels
             (16, None, 0, "", ["INT8:192:64"]),            # INT8 rows not aligned to the 128-element blocks (K % 32 == 0)
             (16, None, 0, "", ["NF4:512:64:nolevels"]),
             (16, None, 0, "", ["NF4:512:64"]),
             (16, None, 0, "", ["INT8:256:64"]),
             (16, None, 0, "", [good, "Q4_K:512:64:round"]),    # one bad job rejects the group
             (16, None, 0, "", ["Q4_K:512:62"]),            # rows in fours
             (3, None, 0, "min=4", [good]),                 # below WRK_GEMM_MIN
             (4, None, 0, "min=4", [good]),
             (16, None, 0, "", [good] * 9)]                 # more jobs than a launch holds
    p = planner(cases)
    assert [q["ok"] for q in p] == [True, False, False, False, False, False, True, True, False, False, False, True, False]
    for q in p:
        if not q["ok"]:
            assert set(q["route"]) <= {"none"} and not any(q["wgs"].values()), q


def test_group_of_a_k_split_job_and_tile_jobs(planner):
    """100 tokens: 2052 rows of K = 512 are 33 x 2 = 66 tiles >= 64 (tile1), 32 rows are below the tile's 64 (K-split): two launches, each
    numbering its workgroups from 0; a second tile job follows the first one's 33 row tiles."""
    p = planner([(100, None, 0, "", ["Q4_K:512:2052", "Q4_K:512:32", "Q5_K:512:2052", "F16:512:48"])])[0]
    assert p["route"] == ["tile1", "ksplit", "tile1", "ksplit"]
    assert p["wg_begin"] == [0, 0, 33, 2]
    assert p["wgs"] == {"ksliced": 0, "tile3": 0, "tile2": 0, "tile1": 66, "ksplit": 5}
    assert (p["split"]["nt"], p["split"]["nw"], p["split"]["pair"]) == (4, 4, False)
