// kern_archive.hip — the GPU passes of the trace archiver (bftsim_archive_trace, SPEC.md §11e), run
// after the observer's tally while its records are still on the device:
//   pick     lane per frame: its instance by binary search in inst_frame0, then an atomicMin of its index within the
//            instance into the table word it competes for (bft_archive.h pick_word). The smallest index wins whatever
//            the scheduling
//   emit     one wavefront per row. Lane 0 decodes the picked PrePrepare frame into the block's one
//            bftwire_preprepare in LDS and re-encodes the header's 12 leading fields into the slot; then the votes a
//            lane each, 64 a round: every lane counts its vote's encoded length, a wave prefix sum places it, and the
//            lane writes it straight to the slot from the dense seal list. Every store is bounded by the slot
//   heights  lane per instance: archived_height, and the report's counters with one atomic per wave and counter
#include <hip/hip_runtime.h>

#include "bft_archive.h"

namespace bft {
namespace archive {

__global__ __launch_bounds__(256) void bft_archive_pick_kernel(Args a) {
    const uint64_t k = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (k >= a.frames) return;
    // the last instance whose first frame is at or below k (an empty instance shares its first frame with the next)
    uint64_t lo = 0, hi = a.inst;
    while (hi - lo > 1) {
        const uint64_t mid = (lo + hi) >> 1;
        if (a.inst_frame0[mid] <= k) lo = mid; else hi = mid;
    }
    const uint64_t f0 = a.inst_frame0[lo];
    const uint64_t w = pick_word(a.r, a.status, a.signer, k, f0, lo * a.max_heights, a.c, a.quorum);
    if (w != ~0ull) atomicMin(a.pick + w, (uint32_t)(k - f0));
}

__global__ __launch_bounds__(64) void bft_archive_emit_kernel(Args a) {
    __shared__ bftwire_preprepare pp;
    __shared__ uint8_t seal_buf[72];
    __shared__ uint32_t front;
    const uint32_t lane = threadIdx.x;
    const uint64_t row = blockIdx.x;
    const uint64_t f0 = a.inst_frame0[row / a.max_heights];
    const uint32_t st = row_status(a.c, row, a.pick, a.quorum);            // wave-uniform
    const uint64_t w0 = row * pick_words(a.quorum);
    const uint32_t pf = a.pick[w0];
    uint8_t* slot = a.hdr + row * a.slot_bytes;
    const uint32_t cap = (uint32_t)a.slot_bytes;
    uint32_t total = 0, nv = 0, nf = 0;
    bool bad = false;
    if (st == AR_OK) {
        if (lane == 0) {
            const uint64_t k = f0 + pf;
            const uint64_t o0 = a.foff[k] - a.base, o1 = a.foff[k + 1] - a.base;
            front = emit_front(a.stream + o0, o1 - o0, pp, seal_buf, slot, cap);
        }
        __syncthreads();
        const uint32_t fl = front;
        const uint64_t* vw = a.c.voters + 4 * row;
        nv = voter_count(vw);
        bad = fl == NONE || nv != a.quorum + 1u;
        if (!bad) {
            if (lane == 0) {
                uint32_t n = fl;
                votes_head(wire::BufE{slot, &n, cap}, nv);
            }
            total = fl + votes_head_len(nv);
            for (uint32_t r0 = 0; r0 < nv; r0 += 64u) {                    // wave-uniform
                const uint32_t r = r0 + lane;
                const uint8_t* seal = nullptr;
                uint32_t len = 0;
                bool foreign = false, missing = false;
                if (r < nv) {
                    const uint32_t pk = a.pick[w0 + 1u + r];
                    missing = pk == NONE;
                    if (!missing) {
                        const uint64_t k = f0 + pk;
                        seal = a.r.seal + 65ull * a.r.seal_k[k];
                        len = vote_len(seal);
                        foreign = a.status[k] == audit::ST_SEAL_FOREIGN;
                    }
                }
                uint32_t incl = len;                                       // inclusive prefix sum over the wave
                for (uint32_t o = 1; o < 64u; o <<= 1) {
                    const uint32_t t = (uint32_t)__shfl_up((int)incl, o, 64);
                    if (lane >= o) incl += t;
                }
                const uint32_t at = total + incl - len;
                bool over = false;
                if (seal) over = write_vote(slot, at, cap, seal) != len || at + len > cap;
                bad = bad || __ballot(missing || over) != 0;
                nf += (uint32_t)__popcll(__ballot(foreign));
                total += (uint32_t)__shfl((int)incl, 63, 64);
            }
        }
        bad = bad || total > cap;
    }
    if (lane == 0) {
        const bool ok = st == AR_OK && !bad;
        a.hdr_len[row] = ok ? total : 0u;
        a.out_status[row] = (uint8_t)st;
        a.pp_frame[row] = pf;
        a.n_votes[row] = (uint16_t)(ok ? nv : 0u);
        a.n_foreign[row] = (uint16_t)(ok ? nf : 0u);
        if (bad) atomicAdd(a.counts + CNT_ERR, 1ull);
    }
}

__device__ inline void sum_wave(unsigned long long* counts, uint32_t word, uint32_t v) {
    for (int o = 32; o > 0; o >>= 1) v += (uint32_t)__shfl_xor((int)v, o, 64);
    if (v && (threadIdx.x & 63u) == 0) atomicAdd(counts + word, (unsigned long long)v);
}

__global__ __launch_bounds__(256) void bft_archive_heights_kernel(Args a) {
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    uint32_t by[3] = {0, 0, 0}, votes = 0, foreign = 0, whole_n = 0;
    if (i < a.inst) {
        const uint64_t row0 = i * a.max_heights;
        bool whole = false;
        a.height[i] = archived_height(a.out_status + row0, a.max_heights, &whole);
        whole_n = whole ? 1u : 0u;
        for (uint32_t x = 0; x < a.max_heights; ++x) {
            const uint32_t st = a.out_status[row0 + x];
            for (uint32_t s = 0; s < 3; ++s) by[s] += st == s ? 1u : 0u;
            votes += a.n_votes[row0 + x];
            foreign += a.n_foreign[row0 + x];
        }
    }
    for (uint32_t s = 0; s < 3; ++s) sum_wave(a.counts, CNT_STATUS + s, by[s]);
    sum_wave(a.counts, CNT_VOTES, votes);
    sum_wave(a.counts, CNT_FOREIGN, foreign);
    sum_wave(a.counts, CNT_ARCHIVED, whole_n);
}

hipError_t launch_pick(const Args& a, hipStream_t s) {
    if (a.frames == 0 || a.inst == 0) return hipSuccess;
    hipLaunchKernelGGL(bft_archive_pick_kernel, dim3((uint32_t)((a.frames + 255) / 256)), dim3(256), 0, s, a);
    return hipGetLastError();
}
hipError_t launch_emit(const Args& a, hipStream_t s) {
    const uint64_t rows = a.inst * a.max_heights;
    if (rows == 0) return hipSuccess;
    hipLaunchKernelGGL(bft_archive_emit_kernel, dim3((uint32_t)rows), dim3(64), 0, s, a);
    return hipGetLastError();
}
hipError_t launch_heights(const Args& a, hipStream_t s) {
    if (a.inst == 0) return hipSuccess;
    hipLaunchKernelGGL(bft_archive_heights_kernel, dim3((uint32_t)((a.inst + 255) / 256)), dim3(256), 0, s, a);
    return hipGetLastError();
}

}  // namespace archive
}  // namespace bft
