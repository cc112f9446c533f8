// kern_accuse.hip — the GPU passes of the trace accuser (bftsim_accuse_trace, SPEC.md §11g), run
// behind the observer's classify and tally passes over their records, which they only read:
//   walk     one wavefront per instance, the tally kernel's shape: 64 frames at a time into LDS, then walked in order
//            by a wave-uniform loop; the lanes own the view slots (slot s: lane s % 64) and match a frame's view all at
//            once. The slot's owner alone reads and writes the slot's view and its first[3][N], so every table access
//            is one thread's in program order. The two digests of a comparison are read from the records in place
//   mark     lane per frame: has it a pair
//   (scan)   hipCUB over the marks, by the caller (bftsim.hip)
//   gather   lane per marked frame: its 32-byte record at its scanned position
#include <hip/hip_runtime.h>

#include "bft_accuse.h"

namespace bft {
namespace accuse {

__device__ inline void wave_sync() {
    __builtin_amdgcn_wave_barrier();
    asm volatile("" ::: "memory");
}

struct Staged {                     // a frame that counts
    uint64_t round;
    uint32_t hx, code, signer, pad;
};

__global__ __launch_bounds__(64) void bft_accuse_walk_kernel(Args a) {
    __shared__ Staged tf[64];
    const uint32_t lane = threadIdx.x;
    const uint64_t inst = blockIdx.x;
    const uint64_t f0 = a.inst_frame0[inst], f1 = a.inst_frame0[inst + 1];
    View* views = a.views + inst * a.view_cap;
    uint32_t* first = a.first + inst * a.view_cap * 3ull * a.n;
    uint32_t nviews = 0, flags = 0, by_code[3] = {0, 0, 0};
    uint64_t acc[4] = {0, 0, 0, 0};
    for (uint64_t fb = f0; fb < f1; fb += 64u) {
        const uint64_t k = fb + lane;
        bool go = false;
        if (k < f1) {
            const uint32_t code = a.r.code[k], hx = a.r.hx[k];
            go = counts(a.status[k], code, hx);
            if (go) {
                Staged& v = tf[lane];
                v.round = a.r.round[k]; v.hx = hx; v.code = code; v.signer = (uint32_t)a.signer[k]; v.pad = 0;
            }
        }
        uint64_t todo = __ballot(go);
        wave_sync();
        while (todo) {                                             // wave-uniform, in frame order
            const uint32_t f = (uint32_t)__builtin_ctzll(todo);
            todo &= todo - 1ull;
            const Staged& v = tf[f];
            if (v.signer >= a.n) continue;                         // never for an accepted frame: no cell outside the table
            uint32_t slot = NONE;
            for (uint32_t t = 0; t < nviews; t += 64u) {           // every lane looks at its own slots
                const uint32_t s = t + lane;
                const uint64_t m = __ballot(s < nviews && view_is(views[s], v.hx, v.round));
                if (m) slot = t + (uint32_t)__builtin_ctzll(m);
            }
            const bool fresh = slot == NONE;
            if (fresh) {
                if (nviews == a.view_cap) { flags |= FLAG_VIEW_OVERFLOW; continue; }
                slot = nviews++;
            }
            const uint32_t owner = slot & 63u;
            uint32_t pair = NONE;
            if (lane == owner) {
                if (fresh) view_put(views[slot], v.hx, v.round);
                const uint64_t kk = fb + f;
                pair = group_step(first + cell(slot, v.code, v.signer, a.n), (uint32_t)(kk - f0), kk, a.r.digest);
                if (pair != NONE) a.frame_pair[kk] = (uint32_t)(f0 + pair);
            }
            pair = (uint32_t)__shfl((int)pair, (int)owner, 64);
            if (pair != NONE) {
                for (uint32_t c = 0; c < 3; ++c) by_code[c] += v.code == c + 1u ? 1u : 0u;      // no indexed registers
                for (uint32_t q = 0; q < 4; ++q) acc[q] |= (v.signer >> 6) == q ? 1ull << (v.signer & 63u) : 0ull;
            }
        }
        wave_sync();
    }
    if (lane == 0) {
        uint32_t pc = 0;
        for (int q = 0; q < 4; ++q) {
            a.inst_accused[4 * inst + q] = acc[q];
            pc += (uint32_t)__popcll(acc[q]);
        }
        a.inst_flags[inst] = flags;
        const uint32_t recs = by_code[0] + by_code[1] + by_code[2];
        if (recs) atomicAdd(a.counts + CNT_RECORDS, (unsigned long long)recs);
        for (int c = 0; c < 3; ++c)
            if (by_code[c]) atomicAdd(a.counts + CNT_CODE + c, (unsigned long long)by_code[c]);
        if (pc) {
            atomicAdd(a.counts + CNT_ACCUSED, (unsigned long long)pc);
            atomicAdd(a.counts + CNT_INSTANCES, 1ull);
        }
        if (flags & FLAG_VIEW_OVERFLOW) atomicAdd(a.counts + CNT_VIEW_OVERFLOWS, 1ull);
    }
}

__global__ __launch_bounds__(256) void bft_accuse_mark_kernel(Args a) {
    const uint64_t k = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (k <= a.frames) a.mark[k] = k < a.frames && a.frame_pair[k] != NONE ? 1u : 0u;
}

__global__ __launch_bounds__(256) void bft_accuse_gather_kernel(Args a) {
    const uint64_t k = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (k >= a.frames || a.mark[k] == 0) return;
    const uint64_t at = a.pos[k];
    if (at >= a.rec_cap) return;
    record_put(a.records[at], a.r, a.signer, inst_of(a.inst_frame0, a.inst, k), a.frame_pair[k], k);
}

hipError_t launch_walk(const Args& a, hipStream_t s) {
    if (a.inst == 0) return hipSuccess;
    hipLaunchKernelGGL(bft_accuse_walk_kernel, dim3((uint32_t)a.inst), dim3(64), 0, s, a);
    return hipGetLastError();
}
hipError_t launch_mark(const Args& a, hipStream_t s) {
    hipLaunchKernelGGL(bft_accuse_mark_kernel, dim3((uint32_t)((a.frames + 1 + 255) / 256)), dim3(256), 0, s, a);
    return hipGetLastError();
}
hipError_t launch_gather(const Args& a, hipStream_t s) {
    if (a.frames == 0) return hipSuccess;
    hipLaunchKernelGGL(bft_accuse_gather_kernel, dim3((uint32_t)((a.frames + 255) / 256)), dim3(256), 0, s, a);
    return hipGetLastError();
}

}  // namespace accuse
}  // namespace bft
