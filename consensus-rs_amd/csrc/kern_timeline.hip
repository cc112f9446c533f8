// kern_timeline.hip — the GPU passes of the trace chronicler (bftsim_timeline_trace, SPEC.md §11h), run
// behind the observer's classify and tally passes over their records and certificate rows, which they only read:
//   walk   one wavefront per instance, the tally kernel's shape: 64 frames at a time into LDS (code, height, round,
//          signer; the digest stays in the records), then walked in order by a wave-uniform loop; the lanes own the key
//          slots (slot s: lane s % 64) and match a frame's key all at once, a Prepare's digest against the frame's row
//          of the records. The slot's owner alone reads and writes its key. The rows of the instance have one writer,
//          lane 0: a key's quorum reaches it through the wave's registers, so no table or row access crosses lanes
//   rows   one lane per (instance, height): the three flags, the instance's open height, the report's row counters
#include <hip/hip_runtime.h>

#include "bft_timeline.h"

namespace bft {
namespace timeline {

__device__ inline void wave_sync() {
    __builtin_amdgcn_wave_barrier();
    asm volatile("" ::: "memory");
}
// one atomic per wave and counter: the lanes for which `c` holds
__device__ inline void count_wave(unsigned long long* counts, uint32_t word, bool c) {
    const uint64_t m = __ballot(c);
    if (m && (threadIdx.x & 63u) == 0) atomicAdd(counts + word, (unsigned long long)__popcll(m));
}

struct Staged {                     // a frame that counts, its height in range
    uint64_t round;
    uint32_t hx, code, signer, pad;
};

__global__ __launch_bounds__(64) void bft_timeline_walk_kernel(Args a) {
    __shared__ Staged tf[64];
    const uint32_t lane = threadIdx.x;
    const uint64_t inst = blockIdx.x;
    const uint64_t f0 = a.inst_frame0[inst], f1 = a.inst_frame0[inst + 1];
    Key* keys = a.keys + inst * a.tl_cap;
    const uint64_t row0 = inst * a.max_heights;
    uint32_t nkeys = 0, flags = 0, n_prep = 0, n_rc = 0, n_oor = 0, n_rcq = 0;
    for (uint64_t fb = f0; fb < f1; fb += 64u) {
        const uint64_t k = fb + lane;
        bool go = false, oor = false;
        uint32_t code = 0;
        if (k < f1) {
            code = a.r.code[k];
            const uint32_t hx = a.r.hx[k];
            const bool c = counts(a.status[k], code);
            go = c && hx != 0;
            oor = c && hx == 0;
            if (go) {
                Staged& v = tf[lane];
                v.round = a.r.round[k]; v.hx = hx; v.code = code; v.signer = (uint32_t)a.signer[k]; v.pad = 0;
            }
        }
        uint64_t todo = __ballot(go);
        n_prep += (uint32_t)__popcll(__ballot(go && code == (uint32_t)MT_PREPARE));
        n_rc += (uint32_t)__popcll(__ballot(go && code == (uint32_t)MT_ROUND_CHANGE));
        n_oor += (uint32_t)__popcll(__ballot(oor));
        wave_sync();
        while (todo) {                                             // wave-uniform, in frame order
            const uint32_t f = (uint32_t)__builtin_ctzll(todo);
            todo &= todo - 1ull;
            const Staged& v = tf[f];
            if (v.signer >= a.n || v.signer > 255u) continue;      // never for an accepted frame: no bit outside the bitmap
            const uint64_t kk = fb + f;
            const uint64_t* dig = (const uint64_t*)(a.r.digest + 32 * kk);
            uint32_t slot = NONE;
            for (uint32_t t = 0; t < nkeys; t += 64u) {            // every lane looks at its own slots
                const uint32_t s = t + lane;
                const uint64_t m = __ballot(s < nkeys && key_is(keys[s], v.code, v.hx, v.round, dig));
                if (m) slot = t + (uint32_t)__builtin_ctzll(m);
            }
            const bool fresh = slot == NONE;
            if (fresh) {
                if (nkeys == a.tl_cap) { flags |= FLAG_KEY_OVERFLOW; continue; }
                slot = nkeys++;
            }
            const uint32_t owner = slot & 63u, rel = (uint32_t)(kk - f0);
            const bool prep = v.code == (uint32_t)MT_PREPARE;
            uint32_t crossed = 0;
            uint64_t w0 = 0, w1 = 0, w2 = 0, w3 = 0;
            if (lane == owner) {
                Key& key = keys[slot];
                if (fresh) key_put(key, v.code, v.hx, v.round, dig);
                crossed = key_vote(key, v.signer, a.quorum, rel) ? 1u : 0u;
                if (crossed && prep) { w0 = key.voters[0]; w1 = key.voters[1]; w2 = key.voters[2]; w3 = key.voters[3]; }
            }
            crossed = (uint32_t)__shfl((int)crossed, (int)owner, 64);
            const uint64_t row = row0 + (v.hx - 1u);
            if (crossed && prep) {                                 // the quorum to the rows' writer
                w0 = __shfl((unsigned long long)w0, (int)owner, 64); w1 = __shfl((unsigned long long)w1, (int)owner, 64);
                w2 = __shfl((unsigned long long)w2, (int)owner, 64); w3 = __shfl((unsigned long long)w3, (int)owner, 64);
                if (lane == 0) row_prepare(a.rows, row, v.round, dig, w0, w1, w2, w3, rel);
            }
            if (!prep) {
                n_rcq += crossed;
                if (lane == 0) {
                    if (crossed) row_rc_quorum(a.rows, row, v.round, rel, a.r.round + f0);
                    row_rc_frame(a.rows, row, v.round);
                }
            }
        }
        wave_sync();
    }
    if (lane == 0) {
        a.inst_nkeys[inst] = nkeys;
        a.inst_flags[inst] = flags;
        a.open_height[inst] = a.max_heights + 1u;                  // the rows pass lowers it
        if (n_prep) atomicAdd(a.counts + CNT_PREPARE_FRAMES, (unsigned long long)n_prep);
        if (n_rc) atomicAdd(a.counts + CNT_RC_FRAMES, (unsigned long long)n_rc);
        if (n_oor) atomicAdd(a.counts + CNT_OUT_OF_RANGE, (unsigned long long)n_oor);
        if (n_rcq) atomicAdd(a.counts + CNT_RC_QUORUMS, (unsigned long long)n_rcq);
        if (flags & FLAG_KEY_OVERFLOW) atomicAdd(a.counts + CNT_KEY_OVERFLOWS, 1ull);
    }
}

__global__ __launch_bounds__(256) void bft_timeline_rows_kernel(Args a) {
    const uint64_t row = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    uint32_t fl = 0;
    bool prepared = false, rc = false;
    if (row < a.inst * a.max_heights) {
        const uint64_t inst = row / a.max_heights;
        const uint32_t x = (uint32_t)(row % a.max_heights) + 1u;
        const bool has_cert = a.certs.round[row] != ROUND_NONE;
        const uint32_t cf = a.certs.frame[row];
        prepared = a.rows.prep_quorums[row] != 0;
        rc = a.rows.rc_quorums[row] != 0;
        fl = row_flags(a.keys + inst * a.tl_cap, a.inst_nkeys[inst], x, prepared, has_cert,
                       (const uint64_t*)(a.certs.digest + 32 * row), has_cert ? a.r.round[a.inst_frame0[inst] + cf] : 0ull, cf);
        a.rows.flags[row] = (uint8_t)fl;
        if (!has_cert) atomicMin(a.open_height + inst, x);
    }
    count_wave(a.counts, CNT_PREPARED, prepared);
    count_wave(a.counts, CNT_RC_HEIGHTS, rc);
    count_wave(a.counts, CNT_PREPARED_FIRST, (fl & ROW_PREPARED_FIRST) != 0);
    count_wave(a.counts, CNT_CERT_UNPREPARED, (fl & ROW_CERT_UNPREPARED) != 0);
    count_wave(a.counts, CNT_LOCKED_OPEN, (fl & ROW_LOCKED_OPEN) != 0);
}

hipError_t launch_walk(const Args& a, hipStream_t s) {
    if (a.inst == 0) return hipSuccess;
    hipLaunchKernelGGL(bft_timeline_walk_kernel, dim3((uint32_t)a.inst), dim3(64), 0, s, a);
    return hipGetLastError();
}
hipError_t launch_rows(const Args& a, hipStream_t s) {
    const uint64_t rows = a.inst * a.max_heights;
    if (rows == 0) return hipSuccess;
    hipLaunchKernelGGL(bft_timeline_rows_kernel, dim3((uint32_t)((rows + 255) / 256)), dim3(256), 0, s, a);
    return hipGetLastError();
}

}  // namespace timeline
}  // namespace bft
