// kern_audit.hip — the GPU passes of the trace observer (bftsim_audit_trace, SPEC.md §11c):
//   decode    lane per frame through the decoders and emitters the tree already has (bft_audit.h), every frame
//             read in place with byte loads bounded by its span. Staging a wave's 64 frames in LDS with 16-byte
//             coalesced loads, the export's shape, measured 1.70x slower here (30.1 against 17.7 ms on 1.32 M
//             frames): the parser, not the loads, bounds a lane, and the 32 KiB stage halved the
//             resident blocks
//   classify  lane per frame: the recovered address among the validators (table in LDS), the seal against the signer
//   tally     one wavefront per instance: 64 frames at a time into LDS, then walked in order by a wave-uniform
//             loop; the lanes own the key slots (slot s: lane s % 64) and match a frame's key all at once
// The recoveries between decode and classify are libbftsig's (bftsim.hip).
#include <hip/hip_runtime.h>

#include "bft_audit.h"

namespace bft {
namespace audit {

__device__ inline void wave_sync() {
    __builtin_amdgcn_wave_barrier();
    asm volatile("" ::: "memory");
}

// the record of every active lane's frame `p[0, span)` (frame index fb + lane). Wave-uniform call.
__device__ inline void decode_wave(const DecodeArgs& a, uint64_t fb, bool act, const uint8_t* p, uint64_t span,
                                   wire::Decoded* dec, bftwire_preprepare* pp, uint8_t* kb, uint8_t* mbuf) {
    const uint32_t lane = threadIdx.x;
    const uint64_t i = fb + lane;
    uint8_t* kbuf = kb + lane * 136u;
    bool done = !act, commit = false;
    if (act && span > MAX_SPAN) {
        rec_undecodable(a.r, i);
        done = true;
    }
    if (!done && wire::decode_frame(p, (uint32_t)span, dec[lane])) {
        if (subject_record(dec[lane], a.max_heights, kbuf, a.r, i)) commit = dec[lane].code == (uint32_t)MT_COMMIT;
        else rec_undecodable(a.r, i);
        done = true;
    }
    // the decodable Commits of the wave take consecutive slots of the dense seal list: one atomic per wave
    const uint64_t cm = __ballot(commit);
    if (cm) {
        const uint32_t lead = (uint32_t)__builtin_ctzll(cm);
        uint32_t base = 0;
        if (lane == lead) base = atomicAdd(a.n_seals, (uint32_t)__popcll(cm));
        base = (uint32_t)__shfl((int)base, (int)lead, 64);
        if (commit) seal_record(dec[lane], kbuf, a.r, i, base + (uint32_t)__popcll(cm & ((1ull << lane) - 1ull)));
    }
    // what is no Subject frame: a Preprepare (one per view against the votes' N^2) or undecodable. One lane at a
    // time through the wave's one bftwire_preprepare and payload buffer in LDS
    uint64_t rest = __ballot(!done);
    while (rest) {
        const uint32_t l = (uint32_t)__builtin_ctzll(rest);
        rest &= rest - 1ull;
        if (lane == l) {
            uint32_t has_seal = 0;
            if (!(wire::decode_pp_frame(p, (uint32_t)span, *pp, &has_seal, mbuf) &&
                  pp_record(*pp, has_seal, a.addresses, a.n, a.seed_le != 0, a.max_heights, kbuf, mbuf, a.r, i)))
                rec_undecodable(a.r, i);
        }
        wave_sync();
    }
}

__global__ __launch_bounds__(64) void bft_audit_decode_kernel(DecodeArgs a) {
    __shared__ __attribute__((aligned(8))) uint8_t kb[64 * 136];
    __shared__ wire::Decoded dec[64];
    __shared__ bftwire_preprepare pp;
    __shared__ uint8_t mbuf[PP_BUF];
    const uint32_t lane = threadIdx.x;
    const uint64_t fb = (uint64_t)blockIdx.x * 64u;
    const uint32_t live = (uint32_t)(a.frames - fb < 64u ? a.frames - fb : 64u);
    const uint64_t k = fb + (lane < live ? lane : live);          // idle lanes: the empty frame at the block's end
    const uint64_t o0 = a.foff[k] - a.base, o1 = a.foff[lane < live ? k + 1 : k] - a.base;
    decode_wave(a, fb, lane < live, a.stream + o0, o1 - o0, dec, &pp, kb, mbuf);
}

// one atomic per wave and counter: the lanes for which `c` holds
__device__ inline void count_wave(unsigned long long* counts, uint32_t word, bool c) {
    const uint64_t m = __ballot(c);
    if (m && (threadIdx.x & 63u) == 0) atomicAdd(counts + word, (unsigned long long)__popcll(m));
}

__global__ __launch_bounds__(256) void bft_audit_classify_kernel(ClassifyArgs a) {
    __shared__ uint8_t addr[256 * 20];
    for (uint32_t j = threadIdx.x; j < a.n * 20u; j += 256u) addr[j] = a.addresses[j];
    __syncthreads();
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    const bool live = i < a.frames;
    uint32_t st = 0xffu, code = 0;
    if (live) {
        int32_t signer;
        st = classify(a.r, i, addr, a.n, a.rec_addr, a.rec_ok, a.seal_addr, a.seal_ok, &signer);
        a.status[i] = (uint8_t)st;
        a.signer[i] = signer;
        code = a.r.code[i];
    }
    for (uint32_t s = 0; s < 6; ++s) count_wave(a.counts, CNT_STATUS + s, st == s);
    const bool acc = st == ST_OK || st == ST_SEAL_FOREIGN;
    for (uint32_t c = 1; c <= 4; ++c) count_wave(a.counts, CNT_CODE + c - 1u, acc && code == c);
}

__global__ __launch_bounds__(64) void bft_audit_tally_kernel(TallyArgs a) {
    __shared__ Vote tv[64];
    const uint32_t lane = threadIdx.x;
    const uint64_t inst = blockIdx.x;
    const uint64_t f0 = a.inst_frame0[inst], f1 = a.inst_frame0[inst + 1];
    Key* keys = a.keys + inst * a.key_cap;
    uint32_t nkeys = 0, flags = 0, n_cert = 0, n_conf = 0, n_oor = 0;
    for (uint64_t fb = f0; fb < f1; fb += 64u) {
        const uint64_t k = fb + lane;
        bool go = false;
        if (k < f1) {
            const uint32_t st = a.status[k], code = a.r.code[k], hx = a.r.hx[k];
            const bool tallied = (st == ST_OK || st == ST_SEAL_FOREIGN) && (code == (uint32_t)MT_PREPREPARE || code == (uint32_t)MT_COMMIT);
            go = tallied && hx != 0;
            if (tallied && hx == 0) ++n_oor;
            if (go) {
                Vote& v = tv[lane];
                const uint64_t* d = (const uint64_t*)(a.r.digest + 32 * k);
                for (int q = 0; q < 4; ++q) v.digest[q] = d[q];
                v.round = a.r.round[k]; v.hx = hx; v.code = code; v.signer = (uint32_t)a.signer[k]; v.want = a.r.pp_want[k];
            }
        }
        uint64_t todo = __ballot(go);
        wave_sync();
        while (todo) {                                             // wave-uniform, in frame order
            const uint32_t f = (uint32_t)__builtin_ctzll(todo);
            todo &= todo - 1ull;
            const Vote& v = tv[f];
            // every lane looks at its own slots: the vote's key, and the height's certificate
            uint32_t slot = NONE;
            bool has_cert = false, same_cert = false;
            for (uint32_t t = 0; t < nkeys; t += 64u) {
                const uint32_t s = t + lane;
                const uint32_t rel = s < nkeys ? key_relation(keys[s], v) : 0u;
                const uint64_t m = __ballot((rel & 1u) != 0);
                if (m) slot = t + (uint32_t)__builtin_ctzll(m);
                has_cert = has_cert || __ballot((rel & 2u) != 0) != 0;
                same_cert = same_cert || __ballot((rel & 4u) != 0) != 0;
            }
            if (v.code == (uint32_t)MT_COMMIT && same_cert) continue;      // the certified digest again
            const bool fresh = slot == NONE;
            if (fresh) {
                if (nkeys == a.key_cap) { flags |= 1u; continue; }         // BFTSIM_AUDIT_KEY_OVERFLOW
                slot = nkeys++;
            }
            const uint32_t owner = slot & 63u;
            uint32_t res = 0;
            if (lane == owner) {
                Key& key = keys[slot];
                res = tally_apply(key, fresh, v, a.quorum, has_cert);
                if (res & TALLY_CERTIFY) {                                 // the row is written once, here
                    const uint64_t row = inst * a.max_heights + (v.hx - 1u);
                    a.cert_round[row] = cert_round(key);
                    for (int q = 0; q < 4; ++q) {
                        ((uint64_t*)(a.cert_digest + 32 * row))[q] = key.digest[q];
                        a.cert_voters[4 * row + q] = key.voters[q];
                    }
                    a.cert_frame[row] = (uint32_t)(fb + f - f0);
                    a.cert_flags[row] = (uint8_t)cert_flags(key);
                }
            }
            res = (uint32_t)__shfl((int)res, (int)owner, 64);
            if (res & TALLY_CERTIFY) ++n_cert;
            if (res & TALLY_CONFLICT) { ++n_conf; flags |= 2u; }           // BFTSIM_AUDIT_CONFLICT
        }
        wave_sync();
    }
    for (int o = 32; o > 0; o >>= 1) n_oor += (uint32_t)__shfl_xor((int)n_oor, o, 64);
    if (lane == 0) {
        a.inst_flags[inst] = flags;
        if (n_oor) atomicAdd(a.counts + CNT_OUT_OF_RANGE, (unsigned long long)n_oor);
        if (n_cert) atomicAdd(a.counts + CNT_CERTIFIED, (unsigned long long)n_cert);
        if (n_conf) atomicAdd(a.counts + CNT_CONFLICTS, (unsigned long long)n_conf);
        if (flags & 1u) atomicAdd(a.counts + CNT_KEY_OVERFLOWS, 1ull);
    }
}

hipError_t launch_decode(const DecodeArgs& a, hipStream_t s) {
    if (a.frames == 0) return hipSuccess;
    hipLaunchKernelGGL(bft_audit_decode_kernel, dim3((uint32_t)((a.frames + 63) / 64)), dim3(64), 0, s, a);
    return hipGetLastError();
}
hipError_t launch_classify(const ClassifyArgs& a, hipStream_t s) {
    if (a.frames == 0) return hipSuccess;
    hipLaunchKernelGGL(bft_audit_classify_kernel, dim3((uint32_t)((a.frames + 255) / 256)), dim3(256), 0, s, a);
    return hipGetLastError();
}
hipError_t launch_tally(const TallyArgs& a, hipStream_t s) {
    if (a.inst == 0) return hipSuccess;
    hipLaunchKernelGGL(bft_audit_tally_kernel, dim3((uint32_t)a.inst), dim3(64), 0, s, a);
    return hipGetLastError();
}

}  // namespace audit
}  // namespace bft
