// Device memory owned in groups: one allocation cut into pieces at 256-byte offsets, and the one policy by which a group of a frame's
// side buffers is reallocated.  Needs the HIP runtime API and nothing of the project.
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstddef>
#include <initializer_list>

inline size_t wrk_up256(size_t x) { return (x + 255) & ~(size_t)255; }

// Pieces of one device allocation at 256-byte offsets: add() every piece first, then allocate `total` once.  The offsets alone, for an
// owner that keeps the memory itself (wrk_dev_arena, wrk_dev_group, wrk_occurrence, wrk_grammar)
struct wrk_dev_layout {
    size_t total = 0;
    size_t add(size_t bytes) { const size_t o = total; total += wrk_up256(bytes); return o; }
};

// One pass of a group's layout function over its allocation: take() every piece in order.  Without a base the pass only sizes the
// allocation and leaves every pointer null
struct wrk_dev_cut {
    char* base = nullptr;
    wrk_dev_layout lay;
    template <class T> void take(T*& p, size_t bytes) {
        const size_t o = lay.add(bytes);
        p = base ? (T*)(base + o) : nullptr;
    }
};

// A group: the device pointers of `Pieces`, all inside one allocation, and the dimensions it was sized for.  Pieces declares
//   static constexpr int DIMS;          how many dimensions size it
//   static constexpr unsigned EXACT;    bit i set: dimension i must match exactly; clear: the group only grows along it
//   void layout(wrk_dev_cut& c, const size_t* d);     takes every piece, sized by d[0 .. DIMS): the only place the sizes are written
// Held or not, the pointers and dim[] always agree: a group that is not held has null pointers and zero dimensions.
template <class Pieces> struct wrk_dev_group : Pieces {
    static constexpr int DIMS = Pieces::DIMS;
    void* mem = nullptr;
    size_t dim[DIMS] = {};
    size_t asked = 0;       // bytes of the last allocation ensure() tried (0: it did not get that far)

    wrk_dev_group() = default;
    wrk_dev_group(const wrk_dev_group&) = delete;
    wrk_dev_group& operator=(const wrk_dev_group&) = delete;

    bool held() const { return mem != nullptr; }
    // the group is held and serves n[i] along dimension i, for the leading dimensions given: what an enqueue asks before it hands the
    // pointers to a kernel
    bool holds(std::initializer_list<size_t> n) const {
        if (!mem || n.size() > (size_t)DIMS) return false;
        int i = 0;
        for (size_t v : n) {
            if ((Pieces::EXACT >> i & 1u) ? v != dim[i] : v > dim[i]) return false;
            ++i;
        }
        return true;
    }
    // Nothing when holds(want) (all DIMS of them).  Else: synchronise `stream`, drop() if and only if the group was held (whatever holds
    // its addresses must go before the memory does), free, take max(want, dim) along every growing dimension, allocate once.  After a
    // failed allocation the group is not held (null pointers, zero dimensions) and the next ensure allocates again; a failed
    // synchronise leaves it as it was
    template <class Drop> hipError_t ensure(hipStream_t stream, std::initializer_list<size_t> want, Drop&& drop) {
        if (want.size() != (size_t)DIMS) return hipErrorInvalidValue;
        if (holds(want)) return hipSuccess;
        asked = 0;
        hipError_t e = hipStreamSynchronize(stream);
        if (e != hipSuccess) return e;
        if (mem) drop();
        size_t next[DIMS];
        int i = 0;
        for (size_t v : want) {
            next[i] = (Pieces::EXACT >> i & 1u) || v > dim[i] ? v : dim[i];
            ++i;
        }
        release();
        wrk_dev_cut size;
        Pieces::layout(size, next);
        asked = size.lay.total ? size.lay.total : 256;
        e = hipMalloc(&mem, asked);
        if (e != hipSuccess) { mem = nullptr; return e; }
        for (i = 0; i < DIMS; ++i) dim[i] = next[i];
        wrk_dev_cut cut{(char*)mem, {}};
        Pieces::layout(cut, dim);
        return hipSuccess;
    }
    void release() {
        if (mem) (void)hipFree(mem);
        mem = nullptr;
        for (int i = 0; i < DIMS; ++i) dim[i] = 0;
        wrk_dev_cut none;
        Pieces::layout(none, dim);
    }
};
