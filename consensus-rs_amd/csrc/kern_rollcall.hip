// kern_rollcall.hip — the GPU passes of the roll call (bftsim_rollcall_trace, SPEC.md §11i), run behind
// the observer's passes and the chronicler's walk over their records, certificate rows and key tables, which they only
// read. One wavefront per instance in every pass:
//   views   lanes over the candidates (the heights, then the chronicler's slots); a due candidate counts the smaller due
//           ones, which is its place in the sorted table, and writes its view there with its proposer
//   walk    64 frames at a time: every lane adds its frame to its signer's counters, which live in LDS ([word][validator],
//           LDS atomics); the PrePrepares of the 64 go through LDS and are matched in frame order by the lanes that own
//           the view slots (slot s: lane s % 64, the first 64 slots in registers). Then the fold: the outcomes, the
//           proposers' due / proposed / missed / won into the same LDS rows, one flush of the rows with vector stores, the
//           silent bitmap by ballot, the report's counters with one atomic per wave and counter
//   gather  the instance's views to their place in the record list, from the exclusive scan of the instances' counts
#include <hip/hip_runtime.h>

#include "bft_rollcall.h"

namespace bft {
namespace rollcall {

__device__ inline void wave_sync() {
    __builtin_amdgcn_wave_barrier();
    asm volatile("" ::: "memory");
}

__global__ __launch_bounds__(64) void bft_rollcall_views_kernel(Args a) {
    const uint32_t lane = threadIdx.x;
    const uint64_t inst = blockIdx.x;
    const uint32_t H = a.max_heights, cands = H + a.inst_nkeys[inst];        // nkeys <= tl_cap: never past the table
    const timeline::Key* keys = a.keys + inst * a.tl_cap;
    const uint64_t row0 = inst * H;
    View* views = a.views + inst * view_cap(H, a.tl_cap);
    uint32_t total = 0;
    for (uint32_t t = 0; t < cands; t += 64u) {
        const uint32_t j = t + lane;
        Cand c;
        c.due = false;
        if (j < cands) c = cand_of(a.certs, row0, H, keys, j);
        total += (uint32_t)__popcll(__ballot(c.due));
        if (c.due) {
            uint32_t rank = 0;                                      // keys are unique: the smaller due ones are its place
            for (uint32_t q = 0; q < cands; ++q) {
                const Cand o = cand_of(a.certs, row0, H, keys, q);
                rank += o.due && view_less(o.height, o.round, c.height, c.round) ? 1u : 0u;
            }
            view_put(views[rank], c, a.certs, row0, a.genesis, a.n, a.seed_le != 0);
        }
    }
    if (lane == 0) a.inst_views[inst] = total;
}

struct Staged {                     // a counting PrePrepare, its height in range
    uint64_t round;
    uint32_t hx, signer;
};

__global__ __launch_bounds__(64) void bft_rollcall_walk_kernel(Args a) {
    __shared__ uint32_t row[ROW_WORDS][256];                        // a wave's 64 validators: 64 banks
    __shared__ Staged tf[64];
    const uint32_t lane = threadIdx.x;
    const uint64_t inst = blockIdx.x;
    const uint64_t f0 = a.inst_frame0[inst], f1 = a.inst_frame0[inst + 1];
    const uint32_t H = a.max_heights, nviews = a.inst_views[inst];
    const uint64_t row0 = inst * H;
    View* views = a.views + inst * view_cap(H, a.tl_cap);
    for (uint32_t w = 0; w < ROW_WORDS; ++w)
        for (uint32_t v = lane; v < 256u; v += 64u) row[w][v] = 0;
    View mine{};                                                    // slot `lane`
    const bool have = lane < nviews;
    if (have) mine = views[lane];
    wave_sync();
    uint32_t n_frames = 0, n_oor = 0;
    for (uint64_t fb = f0; fb < f1; fb += 64u) {
        const uint64_t k = fb + lane;
        bool go = false, oor = false, pp = false;
        if (k < f1) {
            const uint32_t code = a.r.code[k], hx = a.r.hx[k], sg = (uint32_t)a.signer[k];
            const bool c = counts(a.status[k], code) && sg < a.n && sg < 256u;     // an accepted frame's signer is below n
            go = c && hx != 0;
            oor = c && hx == 0;
            if (go) {
                atomicAdd(&row[ROW_FRAMES + code - 1u][sg], 1u);
                atomicMax(&row[ROW_LAST_HEIGHT][sg], hx);
                atomicMax(&row[ROW_LAST_FRAME][sg], (uint32_t)(k - f0) + 1u);
                pp = code == (uint32_t)MT_PREPREPARE;
                if (pp) { Staged& v = tf[lane]; v.round = a.r.round[k]; v.hx = hx; v.signer = sg; }
            }
        }
        n_frames += (uint32_t)__popcll(__ballot(go));
        n_oor += (uint32_t)__popcll(__ballot(oor));
        uint64_t todo = __ballot(pp);
        wave_sync();
        while (todo) {                                              // wave-uniform, in frame order
            const uint32_t f = (uint32_t)__builtin_ctzll(todo);
            todo &= todo - 1ull;
            const Staged v = tf[f];
            const uint64_t kk = fb + f, crow = row0 + (v.hx - 1u);
            bool wins = false;                                      // the digests compared in place
            if (a.certs.round[crow] != ROUND_NONE)
                wins = a.r.round[f0 + a.certs.frame[crow]] == v.round &&
                       audit::same_digest((const uint64_t*)(a.r.digest + 32 * kk), (const uint64_t*)(a.certs.digest + 32 * crow));
            const uint32_t rel = (uint32_t)(kk - f0);
            if (have) view_pp(mine, v.hx, v.round, v.signer, rel, wins);
            for (uint32_t s = 64u + lane; s < nviews; s += 64u) view_pp(views[s], v.hx, v.round, v.signer, rel, wins);
        }
        wave_sync();
    }
    // the fold: outcomes, and the proposers' counters
    if (have) views[lane] = mine;
    uint32_t n_proposed = 0, n_missed = 0, n_unattr = 0, n_won = 0;
    for (uint32_t t = 0; t < nviews; t += 64u) {
        const uint32_t s = t + lane;
        uint32_t oc = 0;
        if (s < nviews) {
            View v = views[s];
            oc = outcome_of(v);
            v.outcome = oc;
            views[s] = v;
            if (v.proposer < a.n && v.proposer < 256u) {
                atomicAdd(&row[ROW_DUE][v.proposer], 1u);
                atomicAdd(&row[row_of_outcome(oc)][v.proposer], 1u);
                if (oc & OUT_WON) atomicAdd(&row[ROW_WON][v.proposer], 1u);
            }
        }
        n_proposed += (uint32_t)__popcll(__ballot((oc & 0xffu) == (uint32_t)OUT_PROPOSED));
        n_missed += (uint32_t)__popcll(__ballot((oc & 0xffu) == (uint32_t)OUT_MISSED));
        n_unattr += (uint32_t)__popcll(__ballot((oc & 0xffu) == (uint32_t)OUT_UNATTRIBUTED));
        n_won += (uint32_t)__popcll(__ballot((oc & OUT_WON) != 0));
    }
    wave_sync();
    uint32_t n_silent = 0;
    for (uint32_t base = 0; base < a.n && base < 256u; base += 64u) {
        const uint32_t v = base + lane;
        const bool in = v < a.n;
        uint32_t signed_frames = 0;
        if (in) {
            const uint64_t idx = inst * a.n + v;
            for (uint32_t c = 0; c < 4; ++c) {
                const uint32_t x = row[ROW_FRAMES + c][v];
                a.rows.frames[4 * idx + c] = x;
                signed_frames += x;
            }
            a.rows.last_height[idx] = row[ROW_LAST_HEIGHT][v];
            a.rows.last_frame[idx] = row_last_frame(row[ROW_LAST_FRAME][v]);
            a.rows.due[idx] = row[ROW_DUE][v];
            a.rows.proposed[idx] = row[ROW_PROPOSED][v];
            a.rows.missed[idx] = row[ROW_MISSED][v];
            a.rows.won[idx] = row[ROW_WON][v];
        }
        const uint64_t m = __ballot(in && signed_frames == 0);
        if (lane == 0) a.inst_silent[4 * inst + base / 64u] = m;
        n_silent += (uint32_t)__popcll(m);
    }
    if (lane == 0) {
        const bool partial = (a.tl_flags[inst] & timeline::FLAG_KEY_OVERFLOW) != 0;
        a.inst_flags[inst] = partial ? (uint32_t)FLAG_PARTIAL : 0u;
        if (n_frames) atomicAdd(a.counts + CNT_FRAMES, (unsigned long long)n_frames);
        if (n_oor) atomicAdd(a.counts + CNT_OUT_OF_RANGE, (unsigned long long)n_oor);
        if (nviews) atomicAdd(a.counts + CNT_VIEWS, (unsigned long long)nviews);
        if (n_proposed) atomicAdd(a.counts + CNT_OUTCOME + 0, (unsigned long long)n_proposed);
        if (n_missed) atomicAdd(a.counts + CNT_OUTCOME + 1, (unsigned long long)n_missed);
        if (n_unattr) atomicAdd(a.counts + CNT_OUTCOME + 2, (unsigned long long)n_unattr);
        if (n_won) atomicAdd(a.counts + CNT_WON, (unsigned long long)n_won);
        if (n_silent) { atomicAdd(a.counts + CNT_SILENT, (unsigned long long)n_silent); atomicAdd(a.counts + CNT_SILENT_INST, 1ull); }
        if (partial) atomicAdd(a.counts + CNT_PARTIAL_INST, 1ull);
    }
}

__global__ __launch_bounds__(64) void bft_rollcall_gather_kernel(Args a) {
    const uint64_t inst = blockIdx.x;
    const uint32_t nviews = a.inst_views[inst];
    const uint64_t at = a.pos[inst];
    const View* views = a.views + inst * view_cap(a.max_heights, a.tl_cap);
    for (uint32_t s = threadIdx.x; s < nviews && at + s < a.rec_cap; s += 64u) a.recs[at + s] = record_of(views[s], (uint32_t)inst);
}

hipError_t launch_views(const Args& a, hipStream_t s) {
    if (a.inst == 0) return hipSuccess;
    hipLaunchKernelGGL(bft_rollcall_views_kernel, dim3((uint32_t)a.inst), dim3(64), 0, s, a);
    return hipGetLastError();
}
hipError_t launch_walk(const Args& a, hipStream_t s) {
    if (a.inst == 0) return hipSuccess;
    hipLaunchKernelGGL(bft_rollcall_walk_kernel, dim3((uint32_t)a.inst), dim3(64), 0, s, a);
    return hipGetLastError();
}
hipError_t launch_gather(const Args& a, hipStream_t s) {
    if (a.inst == 0 || a.rec_cap == 0) return hipSuccess;
    hipLaunchKernelGGL(bft_rollcall_gather_kernel, dim3((uint32_t)a.inst), dim3(64), 0, s, a);
    return hipGetLastError();
}

}  // namespace rollcall
}  // namespace bft
