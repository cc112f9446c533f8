// kern_ledger.hip — the GPU passes of the ledger importer (bftsim_verify_ledger, SPEC.md §11d):
//   decode    lane per header slot, read in place with byte loads bounded by min(hdr_len, slot_bytes): the record, the
//             block hash, the seal digest and the header's vote count (bft_ledger.h). The cursor is a value and every
//             field lands in the record in memory, so a lane has no byte array of its own
//   scatter   lane per header, after the scan of the counts: each vote's 65 bytes, its header index and its header's
//             seal digest into the dense vote list the recoveries run over
//   tally     the recovered address of every vote among the validators (table in LDS, binary search), into its header's
//             voter bitmap, duplicate count and bad-vote flag. Two mappings, chosen by the host from the votes per
//             header: a lane per header walking its votes, or a wave per header, 64 votes a round, the bitmap in LDS
//             (the old word of the LDS atomic says whether the voter was there). No global atomic per vote
//   link      lane per header: height, parent, prev_hash, time, votes, proposer -> the status; then lane per instance:
//             verified_height. The report's counters take one atomic per wave and counter
// The recoveries between scatter and tally are libbftsig's (bftsim.hip).
#include <hip/hip_runtime.h>

#include "bft_ledger.h"

namespace bft {
namespace ledger {

__global__ __launch_bounds__(64) void bft_ledger_decode_kernel(Args a) {
    __shared__ __attribute__((aligned(8))) uint8_t kb[64 * 136];
    const uint64_t i = (uint64_t)blockIdx.x * 64u + threadIdx.x;
    if (i >= a.slots) return;
    const uint32_t len = a.hdr_len[i];
    a.vbase[i] = decode_header(a.hdr + i * a.slot_bytes, len, a.slot_bytes, kb + threadIdx.x * 136u, a.recs[i]);
}

__global__ __launch_bounds__(256) void bft_ledger_scatter_kernel(Args a) {
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= a.slots) return;
    const Rec& r = a.recs[i];
    if (r.st != ST_OK || r.n_votes == NONE) return;
    const uint64_t base = a.vbase[i];
    if (base + r.n_votes > a.votes) return;                        // the scan and the records agree; never past the list
    scatter_votes(a.hdr + i * a.slot_bytes, a.hdr_len[i], r, (uint32_t)i, base, a.vsig, a.vhdr, a.vdig);
}

// one atomic per wave and counter: the lanes for which `c` holds
__device__ inline void count_wave(unsigned long long* counts, uint32_t word, bool c) {
    const uint64_t m = __ballot(c);
    if (m && (threadIdx.x & 63u) == 0) atomicAdd(counts + word, (unsigned long long)__popcll(m));
}
__device__ inline void load_addresses(uint8_t* addr, const Args& a) {
    for (uint32_t j = threadIdx.x; j < a.n * 20u; j += 256u) addr[j] = a.addresses[j];
    __syncthreads();
}

// lane per header: its votes one after the other (a header of 3 votes costs a lane, not a wave)
__global__ __launch_bounds__(256) void bft_ledger_tally_lane_kernel(Args a) {
    __shared__ uint8_t addr[256 * 20];
    load_addresses(addr, a);
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    uint32_t dup = 0;
    if (i < a.slots) {
        Tally t{{0, 0, 0, 0}, 0, 0};
        const Rec& r = a.recs[i];
        if (r.st == ST_OK && r.n_votes != NONE) {
            const uint64_t base = a.vbase[i];
            const uint32_t nv = base + r.n_votes <= a.votes ? r.n_votes : 0u;      // never past the dense list
            for (uint32_t v = 0; v < nv; ++v) tally_vote(t, vote_validator(addr, a.n, a.vaddr, a.vok, base + v));
        }
        for (int q = 0; q < 4; ++q) a.voters[4 * i + q] = t.voters[q];
        a.dup[i] = dup = t.dup;
        a.bad[i] = (uint8_t)t.bad;
    }
    for (int o = 32; o > 0; o >>= 1) dup += (uint32_t)__shfl_xor((int)dup, o, 64);
    if ((threadIdx.x & 63u) == 0 && dup) atomicAdd(a.counts + CNT_DUP, (unsigned long long)dup);
}

// wave per header (four headers a block): 64 votes a round
__global__ __launch_bounds__(256) void bft_ledger_tally_wave_kernel(Args a) {
    __shared__ uint8_t addr[256 * 20];
    __shared__ uint32_t bm[4][8];
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    if (lane < 8) bm[w][lane] = 0;
    load_addresses(addr, a);                                       // a block barrier: the bitmaps are zero behind it
    const uint64_t i = (uint64_t)blockIdx.x * 4u + w;
    uint32_t nv = 0, dup = 0;
    uint64_t base = 0;
    bool bad = false;
    if (i < a.slots) {
        const Rec& r = a.recs[i];
        if (r.st == ST_OK && r.n_votes != NONE) { nv = r.n_votes; base = a.vbase[i]; }
        if (base + nv > a.votes) nv = 0;                            // never past the dense list
    }
    for (uint32_t v0 = 0; v0 < nv; v0 += 64u) {                    // wave-uniform: nv is the wave's header's
        const uint32_t v = v0 + lane;
        bool is_dup = false, is_bad = false;
        if (v < nv) {
            const int32_t idx = vote_validator(addr, a.n, a.vaddr, a.vok, base + v);
            if (idx < 0) {
                is_bad = true;
            } else {
                const uint32_t bit = 1u << ((uint32_t)idx & 31u);
                is_dup = (atomicOr(&bm[w][((uint32_t)idx >> 5) & 7u], bit) & bit) != 0;
            }
        }
        dup += (uint32_t)__popcll(__ballot(is_dup));
        bad = bad || __ballot(is_bad) != 0;
    }
    __syncthreads();                                               // every lane's LDS atomic is behind this
    if (i < a.slots) {
        if (lane < 4) a.voters[4 * i + lane] = (uint64_t)bm[w][2 * lane] | ((uint64_t)bm[w][2 * lane + 1] << 32);
        if (lane == 0) {
            a.dup[i] = dup;
            a.bad[i] = bad ? 1 : 0;
            if (dup) atomicAdd(a.counts + CNT_DUP, (unsigned long long)dup);
        }
    }
}

__global__ __launch_bounds__(256) void bft_ledger_link_kernel(Args a) {
    __shared__ uint8_t addr[256 * 20];
    load_addresses(addr, a);
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    uint32_t st = 0xffu;
    if (i < a.slots) {
        const uint64_t in = i / a.H;
        const uint32_t x = (uint32_t)(i % a.H) + 1u;
        st = link_status(a.recs + in * a.H, x, a.genesis_hash, a.genesis_time, a.block_period, a.voters + 4 * i, a.bad[i],
                         a.quorum, addr, a.n);
        const Rec& r = a.recs[i];
        a.status[i] = (uint8_t)st;
        a.n_votes[i] = (uint16_t)(r.st == ST_OK && r.n_votes != NONE ? r.n_votes : 0u);
        for (int k = 0; k < 32; ++k) a.bhash[32 * i + k] = r.bhash[k];
    }
    for (uint32_t s = 0; s < ST_COUNT; ++s) count_wave(a.counts, CNT_STATUS + s, st == s);
    count_wave(a.counts, CNT_HEADERS, st != 0xffu && st != ST_ABSENT);
}

__global__ __launch_bounds__(256) void bft_ledger_heights_kernel(Args a) {
    const uint64_t in = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    bool whole = false;
    if (in < a.inst) a.vheight[in] = verified_height(a.status + in * a.H, a.H, &whole);
    count_wave(a.counts, CNT_WHOLE, whole);
}

hipError_t launch_decode(const Args& a, hipStream_t s) {
    if (a.slots == 0) return hipSuccess;
    hipLaunchKernelGGL(bft_ledger_decode_kernel, dim3((uint32_t)((a.slots + 63) / 64)), dim3(64), 0, s, a);
    return hipGetLastError();
}
hipError_t launch_scatter(const Args& a, hipStream_t s) {
    if (a.slots == 0 || a.votes == 0) return hipSuccess;
    hipLaunchKernelGGL(bft_ledger_scatter_kernel, dim3((uint32_t)((a.slots + 255) / 256)), dim3(256), 0, s, a);
    return hipGetLastError();
}
hipError_t launch_tally(const Args& a, uint32_t mapping, hipStream_t s) {
    if (a.slots == 0) return hipSuccess;
    if (mapping == TALLY_WAVE)
        hipLaunchKernelGGL(bft_ledger_tally_wave_kernel, dim3((uint32_t)((a.slots + 3) / 4)), dim3(256), 0, s, a);
    else
        hipLaunchKernelGGL(bft_ledger_tally_lane_kernel, dim3((uint32_t)((a.slots + 255) / 256)), dim3(256), 0, s, a);
    return hipGetLastError();
}
hipError_t launch_link(const Args& a, hipStream_t s) {
    if (a.slots == 0) return hipSuccess;
    hipLaunchKernelGGL(bft_ledger_link_kernel, dim3((uint32_t)((a.slots + 255) / 256)), dim3(256), 0, s, a);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    hipLaunchKernelGGL(bft_ledger_heights_kernel, dim3((a.inst + 255) / 256), dim3(256), 0, s, a);
    return hipGetLastError();
}

}  // namespace ledger
}  // namespace bft
