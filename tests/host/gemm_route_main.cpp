// Host driver of the MFMA GEMM routing planner (web-rwkv-gguf_amd/csrc/wrk_gemm_route.h): reads launch groups from stdin, builds the dense
// MatJobs that wrk_op_matmul or a runner builds for them, and prints each plan as one JSON line.  Built and run by
// tests/test_gemm_route_host.py, which holds the expectations.
//
// One case per line, blank-separated:
//   name tokens ks_part_cap ks_cnt_cap xsum_cap switches jobs
// ks_part_cap (floats) / ks_cnt_cap / xsum_cap (bytes): 0 = that scratch is absent.  switches: `-` or a comma list of
// min= ks= bps= tile= tile2= tile2f16= tile3= t3split= pair= (the values the environment variables would set).  jobs: `;`-separated
// kind:k:m[:option...] with options round (MATRIX_ROUND_F16), xpad (input rows 4 elements wider than K: not 16-byte aligned), nolevels
// (NF4 without its level table), in<N> (the job reads input buffer N; default: a buffer of its own).
#include "wrk_matjob.h"
#include "wrk_gemm_route.h"

#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

using namespace wrk;

static std::vector<std::string> split(const std::string& s, char c) {
    std::vector<std::string> out;
    std::stringstream ss(s);
    for (std::string t; std::getline(ss, t, c);) out.push_back(t);
    return out;
}

static uint32_t kind_of(const std::string& s) {
    const char* names[] = {"F16", "Q8_0", "Q4_K", "Q5_K", "Q6_K", "INT8", "NF4"};
    const uint32_t kinds[] = {WRK_MAT_F16, WRK_MAT_Q8_0, WRK_MAT_Q4_K, WRK_MAT_Q5_K, WRK_MAT_Q6_K, WRK_MAT_INT8, WRK_MAT_NF4};
    for (int i = 0; i < 7; ++i)
        if (s == names[i]) return kinds[i];
    std::fprintf(stderr, "unknown kind %s\n", s.c_str());
    std::exit(2);
}

// device bytes per row (the layouts of wrk_matvec.hip repack_row_bytes), 16-byte aligned
static uint32_t row_bytes_of(uint32_t kind, uint32_t k) {
    const size_t nb = k / 256;
    size_t b = 0;
    switch (kind) {
        case WRK_MAT_F16: b = (size_t)k * 2; break;
        case WRK_MAT_Q8_0: b = (size_t)k + k / 32 * 2; break;
        case WRK_MAT_Q4_K: b = nb * 148; break;
        case WRK_MAT_Q5_K: b = nb * 180; break;
        case WRK_MAT_Q6_K: b = nb * 210; break;
        case WRK_MAT_INT8: b = (size_t)k + (k / 128 + 2) * 4; break;
        default: b = (size_t)k / 2 + k / 64 * 2; break;
    }
    return (uint32_t)((b + 15) & ~(size_t)15);
}

static DTensor dense(uintptr_t p, uint32_t dtype, uint32_t c, uint32_t t) {
    DTensor d;
    d.p = (void*)p;
    d.dtype = dtype;
    d.shape[0] = d.stride[0] = c; d.shape[1] = d.stride[1] = t; d.shape[2] = d.stride[2] = 1; d.shape[3] = d.stride[3] = 1;
    d.offset[0] = d.offset[1] = d.offset[2] = d.offset[3] = 0;
    return d;
}

template <class T> static void list(const char* key, const T* v, int n, bool comma = true) {
    std::printf("\"%s\":[", key);
    for (int i = 0; i < n; ++i) std::printf("%s%llu", i ? "," : "", (unsigned long long)v[i]);
    std::printf("]%s", comma ? "," : "");
}

int main() {
    static const char* route_names[GEMM_ROUTES] = {"none", "ksliced", "tile3", "tile2", "tile1", "ksplit"};
    int cases = 0;
    for (std::string line; std::getline(std::cin, line);) {
        if (line.empty() || line[0] == '#') continue;
        std::stringstream ls(line);
        std::string name, switches, jobspec;
        unsigned long long tokens, ks_part_cap, ks_cnt_cap, xsum_cap;
        if (!(ls >> name >> tokens >> ks_part_cap >> ks_cnt_cap >> xsum_cap >> switches >> jobspec)) { std::fprintf(stderr, "bad case: %s\n", line.c_str()); return 2; }
        GemmSwitches sw;
        if (switches != "-")
            for (const std::string& kv : split(switches, ',')) {
                const size_t eq = kv.find('=');
                const std::string key = kv.substr(0, eq);
                const int v = std::atoi(kv.substr(eq + 1).c_str());
                if (key == "min") sw.min_tokens = (uint32_t)v;
                else if (key == "ks") sw.ks_mode = v;
                else if (key == "bps") sw.ks_bps = v;
                else if (key == "tile") sw.tile = v != 0;
                else if (key == "tile2") sw.tile2 = v != 0;
                else if (key == "tile2f16") sw.tile2_f16 = v != 0;
                else if (key == "tile3") sw.tile3 = v != 0;
                else if (key == "t3split") sw.t3_split = v != 0;
                else if (key == "pair") sw.pair = v != 0;
                else { std::fprintf(stderr, "unknown switch %s\n", key.c_str()); return 2; }
            }
        std::vector<MatJob> jobs;
        for (const std::string& js : split(jobspec, ';')) {
            const std::vector<std::string> f = split(js, ':');
            if (f.size() < 3) { std::fprintf(stderr, "bad job: %s\n", js.c_str()); return 2; }
            const uint32_t kind = kind_of(f[0]), k = (uint32_t)std::atoi(f[1].c_str()), m = (uint32_t)std::atoi(f[2].c_str());
            const uintptr_t id = jobs.size() + 1;
            MatJob j{(const uint8_t*)(id << 32), kind == WRK_MAT_NF4 ? (const uint8_t*)((id << 32) + 0x100) : nullptr, kind, WRK_MATRIX_EXACT, k, m, row_bytes_of(kind, k),
                     dense((id << 32) + 0x10000000u, WRK_F16, k, (uint32_t)tokens), dense((id << 32) + 0x20000000u, WRK_F32, m, (uint32_t)tokens), WRK_ACT_NONE, 0};
            for (size_t o = 3; o < f.size(); ++o) {
                if (f[o] == "round") j.flags = WRK_MATRIX_ROUND_F16;
                else if (f[o] == "xpad") j.in.stride[0] = k + 4;
                else if (f[o] == "nolevels") j.aux = nullptr;
                else if (f[o].rfind("in", 0) == 0) j.in.p = (void*)((((uintptr_t)std::atoi(f[o].c_str() + 2) + 100) << 32) + 0x10000000u);
                else { std::fprintf(stderr, "unknown option %s\n", f[o].c_str()); return 2; }
            }
            jobs.push_back(j);
        }
        if (jobs.empty()) { std::fprintf(stderr, "no jobs: %s\n", line.c_str()); return 2; }
        // the scratch rides on the first job of a group
        if (ks_part_cap) { jobs[0].ks_part = (float*)0x7000000000ull; jobs[0].ks_cnt = (uint32_t*)0x7100000000ull; jobs[0].ks_part_cap = ks_part_cap; jobs[0].ks_cnt_cap = (uint32_t)ks_cnt_cap; }
        if (xsum_cap) { jobs[0].xsum = (void*)0x7200000000ull; jobs[0].xsum_cap = xsum_cap; }

        GemmPlan P;
        const bool ok = gemm_plan(jobs.data(), (int)jobs.size(), sw, P);
        const int nj = (int)jobs.size() <= GEMM_MAX_JOBS ? (int)jobs.size() : 0;
        int count[GEMM_ROUTES] = {};
        for (int q = 0; q < nj; ++q) ++count[P.route[q]];
        std::printf("{\"name\":\"%s\",\"ok\":%s,\"n\":%u,\"route\":[", name.c_str(), ok ? "true" : "false", P.n);
        for (int q = 0; q < nj; ++q) std::printf("%s\"%s\"", q ? "," : "", route_names[P.route[q]]);
        std::printf("],");
        list("wg_begin", P.wg_begin, nj);
        std::printf("\"wgs\":{");
        for (int r = 1; r < GEMM_ROUTES; ++r) std::printf("%s\"%s\":%u", r > 1 ? "," : "", route_names[r], P.wgs[r]);
        std::printf("},\"ks\":{\"nt\":%d,\"bps\":%d,\"lds\":%zu,", P.ks.nt, P.ks.bps, P.ks.lds_bytes);
        list("nslices", P.ks.nslices, count[GEMM_KSLICED]);
        list("rg_begin", P.ks.rg_begin, count[GEMM_KSLICED], false);
        std::printf("},\"t3\":{\"ttiles\":%u,\"bps\":%u,\"kslices\":%u,", P.t3.ttiles, P.t3.bps, P.t3.kslices);
        list("sums_of", P.t3.sums_of, count[GEMM_TILE3]);
        list("sh", P.t3.sh_off, count[GEMM_TILE3]);
        list("sl", P.t3.sl_off, count[GEMM_TILE3]);
        list("ts", P.t3.ts_off, count[GEMM_TILE3]);
        list("part", P.t3.part_off, P.t3.kslices > 1 ? count[GEMM_TILE3] : 0, false);
        std::printf("},\"split\":{\"nt\":%d,\"nw\":%d,\"pair\":%s}}\n", P.split.nt, P.split.nw, P.split.pair ? "true" : "false");
        ++cases;
    }
    std::fprintf(stderr, "gemm_route: %d cases\n", cases);
    return 0;
}
