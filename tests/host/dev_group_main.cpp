// Host test of wrk_dev_group (web-rwkv-gguf_amd/csrc/wrk_dev_group.h): the policy by which a frame's buffer groups are reallocated,
// against malloc / free stand-ins for the three HIP calls the header makes.  Built and run by tests/test_dev_group_host.py.
#include "wrk_dev_group.h"

#include <cstdint>
#include <cstdio>
#include <cstdlib>

static int live = 0, mallocs = 0, frees = 0, syncs = 0, fail_next = 0;
static size_t last_bytes = 0;

extern "C" hipError_t hipMalloc(void** p, size_t bytes) {
    last_bytes = bytes;
    if (fail_next) { --fail_next; *p = (void*)(uintptr_t)0xdead00;  return hipErrorOutOfMemory; }      // a failed call may leave junk behind
    if (posix_memalign(p, 256, bytes) != 0) return hipErrorOutOfMemory;
    ++live; ++mallocs;
    return hipSuccess;
}
extern "C" hipError_t hipFree(void* p) { free(p); --live; ++frees; return hipSuccess; }
extern "C" hipError_t hipStreamSynchronize(hipStream_t) { ++syncs; return hipSuccess; }

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); ++failures; } } while (0)

// three pieces over (rows: grows, width: exact): a [rows] u32, b [rows][width] f32, c one 40-byte block
struct Pieces {
    static constexpr int DIMS = 2;
    static constexpr unsigned EXACT = 2;
    uint32_t* a = nullptr;
    float* b = nullptr;
    char* c = nullptr;
    void layout(wrk_dev_cut& cut, const size_t* d) { cut.take(a, d[0] * 4); cut.take(b, d[0] * d[1] * 4); cut.take(c, 40); }
};
// two dimensions that both only grow
struct Grow2 {
    static constexpr int DIMS = 2;
    static constexpr unsigned EXACT = 0;
    char *x = nullptr, *y = nullptr;
    void layout(wrk_dev_cut& cut, const size_t* d) { cut.take(x, d[0] * 3); cut.take(y, d[1] * 5 + 1); }
};
// one piece of d[0] bytes
struct Bytes {
    static constexpr int DIMS = 1;
    static constexpr unsigned EXACT = 0;
    char* p = nullptr;
    void layout(wrk_dev_cut& cut, const size_t* d) { cut.take(p, d[0]); }
};

static int drops = 0;
static void drop() { ++drops; }

// the pieces lie inside [mem, mem + total), 256-aligned, in order, each with room for its size rounded up to 256
static void check_layout(const wrk_dev_group<Pieces>& g, size_t rows, size_t width) {
    const char *m = (const char*)g.mem, *a = (const char*)g.a, *b = (const char*)g.b, *c = g.c;
    const size_t sa = wrk_up256(rows * 4), sb = wrk_up256(rows * width * 4), sc = wrk_up256(40);
    CHECK(g.dim[0] == rows && g.dim[1] == width);
    CHECK(a == m && b == a + sa && c == b + sb);
    CHECK(((uintptr_t)a | (uintptr_t)b | (uintptr_t)c) % 256 == 0);
    CHECK(g.asked == sa + sb + sc && last_bytes == g.asked);
    for (size_t i = 0; i < rows; ++i) g.a[i] = 1u;                 // the sanitizers check that every piece is really there
    for (size_t i = 0; i < rows * width; ++i) g.b[i] = 2.0f;
    for (size_t i = 0; i < 40; ++i) g.c[i] = 3;
}

static void not_held(const wrk_dev_group<Pieces>& g) {
    CHECK(!g.held() && g.mem == nullptr && g.a == nullptr && g.b == nullptr && g.c == nullptr && g.dim[0] == 0 && g.dim[1] == 0);
    CHECK(!g.holds({}) && !g.holds({0}) && !g.holds({0, 0}) && !g.holds({1, 7}));
}

int main() {
    hipStream_t s = nullptr;
    {
        wrk_dev_group<Pieces> g;
        not_held(g);
        // the first ensure allocates and does not call drop
        CHECK(g.ensure(s, {10, 7}, drop) == hipSuccess);
        CHECK(drops == 0 && mallocs == 1 && frees == 0 && syncs == 1 && live == 1 && g.held());
        check_layout(g, 10, 7);
        CHECK(g.holds({}) && g.holds({10}) && g.holds({3, 7}) && !g.holds({11}) && !g.holds({3, 8}) && !g.holds({3, 6}) && !g.holds({1, 7, 1}));
        // an equal or smaller request changes no pointer and calls nothing
        const void *m = g.mem, *a = g.a, *b = g.b, *c = g.c;
        CHECK(g.ensure(s, {10, 7}, drop) == hipSuccess && g.ensure(s, {4, 7}, drop) == hipSuccess && g.ensure(s, {0, 7}, drop) == hipSuccess);
        CHECK(g.mem == m && g.a == a && g.b == b && g.c == c && drops == 0 && mallocs == 1 && frees == 0 && syncs == 1);
        CHECK(g.dim[0] == 10 && g.dim[1] == 7);
        // a request with the wrong number of dimensions is refused and changes nothing
        CHECK(g.ensure(s, {10}, drop) == hipErrorInvalidValue && g.mem == m && syncs == 1);
        // larger in the growing dimension: one sync, one drop, one free, one allocation
        CHECK(g.ensure(s, {33, 7}, drop) == hipSuccess);
        CHECK(drops == 1 && mallocs == 2 && frees == 1 && syncs == 2 && live == 1);
        check_layout(g, 33, 7);
        // a changed exact dimension reallocates, smaller or larger; the growing dimension keeps its maximum
        CHECK(g.ensure(s, {2, 5}, drop) == hipSuccess);
        CHECK(drops == 2 && mallocs == 3 && frees == 2 && live == 1);
        check_layout(g, 33, 5);
        CHECK(g.ensure(s, {2, 9}, drop) == hipSuccess);
        CHECK(drops == 3 && live == 1);
        check_layout(g, 33, 9);
        // an allocation that fails while the group is held: drop was called, the group is empty, the next ensure succeeds
        fail_next = 1;
        CHECK(g.ensure(s, {40, 9}, drop) == hipErrorOutOfMemory);
        CHECK(drops == 4 && live == 0 && g.asked == wrk_up256(40 * 4) + wrk_up256(40 * 9 * 4) + 256);
        not_held(g);
        // ... and while it is not held: no drop
        fail_next = 1;
        CHECK(g.ensure(s, {3, 9}, drop) == hipErrorOutOfMemory);
        CHECK(drops == 4 && live == 0);
        not_held(g);
        CHECK(g.ensure(s, {3, 9}, drop) == hipSuccess);
        CHECK(drops == 4 && live == 1);
        check_layout(g, 3, 9);          // the dimensions of before the failure are forgotten
        g.release();
        CHECK(live == 0);
        not_held(g);
        g.release();                    // releasing twice frees once
        CHECK(live == 0 && mallocs == frees);
    }
    {
        // every growing dimension takes the maximum of the request and what is held
        wrk_dev_group<Grow2> g;
        drops = 0;
        CHECK(g.ensure(s, {8, 2}, drop) == hipSuccess && g.dim[0] == 8 && g.dim[1] == 2);
        CHECK(g.ensure(s, {3, 6}, drop) == hipSuccess && g.dim[0] == 8 && g.dim[1] == 6 && drops == 1);
        CHECK(g.ensure(s, {9, 1}, drop) == hipSuccess && g.dim[0] == 9 && g.dim[1] == 6 && drops == 2);
        CHECK(g.y == g.x + wrk_up256(9 * 3) && g.asked == wrk_up256(9 * 3) + wrk_up256(6 * 5 + 1));
        CHECK(g.holds({9, 6}) && g.holds({0, 6}) && !g.holds({0, 7}));
        g.x[9 * 3 - 1] = 1; g.y[6 * 5] = 1;
        // a group of all-zero dimensions still owns an allocation
        wrk_dev_group<Bytes> e;
        CHECK(e.ensure(s, {0}, drop) == hipSuccess && e.held() && e.asked == 256 && e.holds({0}) && !e.holds({1}));
        e.release();
        g.release();
        CHECK(live == 0);
    }
    if (failures) { std::printf("%d checks failed\n", failures); return 1; }
    std::printf("dev_group: ok (%d allocations, %d frees)\n", mallocs, frees);
    return 0;
}
