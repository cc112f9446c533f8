// twins_host.cpp — TEST-ONLY host build of consensus-rs_amd/csrc/bft_twins.h (the mark and merge steps the twin
// kernels run, SPEC.md §11f), checked against tests/twins_ref.py on the CPU. As a shared library (tests/twins_lib.py)
// it indexes one launch's log; with -DTWINS_HOST_MAIN it is a stand-alone program for the sanitizers: it reads a log
// and the expected index from stdin, runs the steps into heap buffers of exactly the counted sizes and compares.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../consensus-rs_amd/csrc/bft_twins.h"

using namespace bft;
using namespace bft::twins;

namespace {
// the passes of kern_twins.hip, one loop per kernel; the twin arrays are allocated after the scan, as there
struct Index {
    uint64_t M = 0, T = 0, counts[2] = {0, 0};
    uint64_t *moff = nullptr, *mref = nullptr, *byz = nullptr, *fmap = nullptr, *tmsg = nullptr, *if0 = nullptr;
    uint32_t *mark = nullptr, *kind = nullptr, *tslot = nullptr;
    ~Index() { free(moff); free(mref); free(byz); free(fmap); free(tmsg); free(if0); free(mark); free(kind); free(tslot); }
};
template <class T> T* heap(uint64_t n) { return (T*)malloc(n ? n * sizeof(T) : 1); }

void build(Index& x, const uint32_t* mlog, const uint32_t* mlog_n, uint32_t n_inst, uint32_t cap, uint64_t seed,
           uint32_t first_instance, uint32_t n_val, uint32_t byz_count) {
    x.moff = heap<uint64_t>(n_inst + 1);
    for (uint32_t i = 0; i < n_inst; ++i) { x.moff[i] = x.M; x.M += mlog_n[i] < cap ? mlog_n[i] : cap; }
    x.moff[n_inst] = x.M;
    x.mref = heap<uint64_t>(x.M);
    for (uint32_t i = 0; i < n_inst; ++i)
        for (uint64_t j = 0; x.moff[i] + j < x.moff[i + 1]; ++j) x.mref[x.moff[i] + j] = (uint64_t)i * cap + j;
    x.byz = heap<uint64_t>(4ull * n_inst);
    uint8_t* perm = heap<uint8_t>(n_val);                       // exactly n bytes: the draw stays inside them
    for (uint32_t i = 0; i < n_inst; ++i) byz_mask(seed, first_instance + i, n_val, byz_count, perm, 1, x.byz + 4ull * i);
    free(perm);
    x.mark = heap<uint32_t>(x.M + 1);
    x.kind = heap<uint32_t>(x.M + 1);
    x.tslot = heap<uint32_t>(x.M + 1);
    for (uint64_t m = 0; m <= x.M; ++m) {                       // bft_twin_mark_kernel
        uint32_t k = MARK_NONE;
        if (m < x.M) k = needs_twin(mlog + x.mref[m] * MLOG_WORDS, x.byz + 4u * (x.mref[m] / cap));
        x.kind[m] = k;
        x.mark[m] = k != MARK_NONE ? 1u : 0u;
        if (k == MARK_PP) ++x.counts[0];
        if (k == MARK_VOTE) ++x.counts[1];
    }
    uint32_t run = 0;
    for (uint64_t m = 0; m <= x.M; ++m) { x.tslot[m] = run; run += x.mark[m]; }   // the exclusive scan
    x.T = x.tslot[x.M];
    x.fmap = heap<uint64_t>(x.M + x.T);
    x.tmsg = heap<uint64_t>(x.T);
    x.if0 = heap<uint64_t>(n_inst + 1);
    for (uint64_t m = 0; m < x.M; ++m) {                        // bft_twin_merge_kernel
        const uint32_t before = x.tslot[m];
        merge_put(m, before < x.T ? before : (uint32_t)x.T, x.mark[m] != 0 && before < x.T, x.fmap, x.tmsg);
    }
    for (uint32_t i = 0; i <= n_inst; ++i) x.if0[i] = frame0(x.moff[i], x.tslot);
}
}  // namespace

extern "C" {
// the index of a launch's log [n_inst][cap][8]: fmap [frame_cap] (message | 1 << 63 for a twin), if0 [n_inst + 1],
// kind [messages] (0 none, 1 PrePrepare twin, 2 vote twin), byz [n_inst][4], counts [2]. Returns the frame count;
// writes nothing but counts when frame_cap is below it.
uint64_t twins_host_index(const uint32_t* mlog, const uint32_t* mlog_n, uint32_t n_inst, uint32_t cap, uint64_t seed,
                          uint32_t first_instance, uint32_t n_val, uint32_t byz_count, uint64_t frame_cap, uint64_t* fmap,
                          uint64_t* if0, uint32_t* kind, uint64_t* byz, uint64_t* counts) {
    Index x;
    build(x, mlog, mlog_n, n_inst, cap, seed, first_instance, n_val, byz_count);
    counts[0] = x.counts[0];
    counts[1] = x.counts[1];
    if (frame_cap < x.M + x.T) return x.M + x.T;
    memcpy(fmap, x.fmap, (x.M + x.T) * 8);
    memcpy(if0, x.if0, (n_inst + 1ull) * 8);
    memcpy(kind, x.kind, x.M * 4);
    memcpy(byz, x.byz, 4ull * n_inst * 8);
    return x.M + x.T;
}
}

#ifdef TWINS_HOST_MAIN
// stdin (little-endian): u32 n_inst, cap, first_instance, n_val, byz_count; u64 seed; u32 mlog_n[n_inst];
// u32 mlog[n_inst][cap][8]; u64 frames; u64 fmap[frames]; u64 if0[n_inst + 1]
static bool rd(void* p, size_t n) { return n == 0 || fread(p, 1, n, stdin) == n; }
int main() {
    uint32_t hd[5];
    uint64_t seed = 0, frames = 0;
    if (!rd(hd, 20) || !rd(&seed, 8)) return 2;
    const uint32_t n_inst = hd[0], cap = hd[1];
    uint32_t* cnt = heap<uint32_t>(n_inst);
    uint32_t* mlog = heap<uint32_t>((uint64_t)n_inst * cap * MLOG_WORDS);
    if (!rd(cnt, 4ull * n_inst) || !rd(mlog, 4ull * n_inst * cap * MLOG_WORDS) || !rd(&frames, 8)) return 2;
    uint64_t* want = heap<uint64_t>(frames);
    uint64_t* want0 = heap<uint64_t>(n_inst + 1ull);
    if (!rd(want, frames * 8) || !rd(want0, (n_inst + 1ull) * 8)) return 2;
    int rc = 0;
    {
        Index x;
        build(x, mlog, cnt, n_inst, cap, seed, hd[2], hd[3], hd[4]);
        if (x.M + x.T != frames || memcmp(x.fmap, want, frames * 8) != 0 || memcmp(x.if0, want0, (n_inst + 1ull) * 8) != 0) {
            printf("index differs: %llu messages %llu twins, expected %llu frames\n", (unsigned long long)x.M,
                   (unsigned long long)x.T, (unsigned long long)frames);
            rc = 1;
        }
        for (uint64_t t = 0; t < x.T && !rc; ++t)
            if (x.fmap[x.tmsg[t] + t + 1] != (x.tmsg[t] | F_TWIN)) { printf("twin slot %llu\n", (unsigned long long)t); rc = 1; }
        if (!rc)
            printf("ok %llu messages %llu pp twins %llu vote twins\n", (unsigned long long)x.M, (unsigned long long)x.counts[0],
                   (unsigned long long)x.counts[1]);
    }
    free(want0); free(want); free(mlog); free(cnt);
    return rc;
}
#endif
