// kern_twins.hip — the GPU passes of trace twins (bftsim_set_trace_twins, SPEC.md §11f), all of them
// cold code on the verify pass's stream:
//   byz      lane per instance: its Byzantine set, drawn as the consensus kernels draw it (the permutation in LDS, a
//            lane's bytes a dword apart so that 64 lanes hit 64 banks)
//   mark     lane per dense message: needs_twin of its log entry; the two counts by a ballot and one atomic per wave
//   (scan)   hipCUB over the marks, by the caller (bftsim.hip), as the trace's size pass scans its lengths
//   merge    lane per dense message: the merged frame index and each twin slot's message; then lane per instance: its
//            first frame
//   prep     lane per twin: the digest of the flipped block id, the original's signing key, a Commit's seal digest
//   digest   lane per twin, after the seals are signed: the sign digest of the twin's GossipMessage
// The signatures between and after the last two are libbftsig's (bftsim.hip).
#include <hip/hip_runtime.h>

#include "bft_crypto.h"
#include "bft_twins.h"

namespace bft {
namespace twins {

__global__ __launch_bounds__(64) void bft_twin_byz_kernel(Args a) {
    __shared__ uint8_t perm[256 * 64 * 4];                       // byte i of lane l at (i * 64 + l) * 4
    const uint64_t i = (uint64_t)blockIdx.x * 64u + threadIdx.x;
    if (i >= a.n_inst) return;
    uint64_t m[4];
    byz_mask(a.seed, a.first_instance + (uint32_t)i, a.n_val, a.byz_count, perm + 4u * threadIdx.x, 256u, m);
    for (int k = 0; k < 4; ++k) a.byz[4 * i + k] = m[k];
}

__global__ __launch_bounds__(256) void bft_twin_mark_kernel(Args a) {
    const uint64_t m = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    uint32_t kind = MARK_NONE;
    if (m < a.M) {
        const uint64_t ref = a.mref[m];
        kind = needs_twin(a.mlog + ref * MLOG_WORDS, a.byz + 4u * (ref / a.cap));
    }
    if (m <= a.M) a.mark[m] = kind != MARK_NONE ? 1u : 0u;
    const uint64_t pp = __ballot(kind == MARK_PP), vo = __ballot(kind == MARK_VOTE);
    if ((pp | vo) && (threadIdx.x & 63u) == 0)
        atomicAdd(a.counts, (unsigned long long)__popcll(pp) | ((unsigned long long)__popcll(vo) << 32));
}

__global__ __launch_bounds__(256) void bft_twin_merge_kernel(Args a) {
    const uint64_t m = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (m < a.M) {
        const uint32_t before = a.tslot[m];
        const bool marked = a.mark[m] != 0 && before < a.T;       // never past the twin arrays
        merge_put(m, before < a.T ? before : (uint32_t)a.T, marked, a.fmap, a.tmsg);
    }
    if (m <= a.n_inst) a.if0[m] = frame0(a.moff[m], a.tslot);
}

__global__ __launch_bounds__(64) void bft_twin_prep_kernel(Params p, Args a) {
    __shared__ __attribute__((aligned(16))) uint8_t hb[64 * LANE_HASH_BUF];
    __shared__ uint8_t kb[64 * 136];
    const uint64_t t = (uint64_t)blockIdx.x * 64u + threadIdx.x;
    if (t >= a.T) return;
    const uint64_t m = a.tmsg[t], ref = a.mref[m];
    const uint32_t* e = a.mlog + ref * MLOG_WORDS;
    const uint32_t code = (e[1] >> 8) & 0xffu;
    const uint64_t b = ((uint64_t)e[4] | ((uint64_t)e[5] << 32)) ^ BLK_FLIP;
    uint8_t d[32];
    crypto_block_digest(p, (uint32_t)(ref / a.cap), b, hb + threadIdx.x * LANE_HASH_BUF, d);
    for (int i = 0; i < 32; ++i) a.raw[t * 32 + i] = d[i];
    const uint32_t key = a.key[m];
    a.tkey[t] = key;
    if (code == (uint32_t)MT_COMMIT) {
        const uint32_t k = atomicAdd(a.ncm, 1u);
        a.msg_k[t] = k;
        a.seal_key[k] = key;
        uint8_t sd[32];
        crypto::seal_digest(kb + threadIdx.x * 136, d, sd);
        for (int i = 0; i < 32; ++i) a.seal_dig[(uint64_t)k * 32 + i] = sd[i];
    }
}

__global__ __launch_bounds__(64) void bft_twin_digest_kernel(Params p, Args a) {
    __shared__ __attribute__((aligned(16))) uint8_t hb[64 * LANE_HASH_BUF];
    __shared__ uint8_t kb[64 * 136];
    const uint64_t t = (uint64_t)blockIdx.x * 64u + threadIdx.x;
    if (t >= a.T) return;
    uint8_t* hbuf = hb + threadIdx.x * LANE_HASH_BUF;
    uint8_t* kbuf = kb + threadIdx.x * 136;
    const uint64_t m = a.tmsg[t], ref = a.mref[m];
    const uint32_t il = (uint32_t)(ref / a.cap);
    const uint32_t* e = a.mlog + ref * MLOG_WORDS;
    const uint32_t code = (e[1] >> 8) & 0xffu;
    uint8_t out[32];
    if (code == (uint32_t)MT_PREPREPARE) {                        // create_time 0: a twin is never a RoundChange
        const uint64_t b = ((uint64_t)e[4] | ((uint64_t)e[5] << 32)) ^ BLK_FLIP;
        const uint32_t x = blk_h(b), prop = blk_prop(b);
        uint32_t prev[8];
        crypto_parent(p, il, x, prev);
        const uint64_t time = p.genesis_time + (uint64_t)p.block_period * ((uint64_t)blk_T(b) + 1ull);
        const uint32_t hlen = header_raw((uint64_t*)hbuf, prev, p.addresses + 20u * prop, p.seed, p.first_instance + il, x,
                                         prop, blk_var(b), time);
        crypto::sign_digest(kbuf, code, 0ull, e[3], e[2], nullptr, hbuf, hlen, nullptr, out);
    } else {
        const uint8_t* seal = code == (uint32_t)MT_COMMIT ? a.seals + (uint64_t)a.msg_k[t] * 65 : nullptr;
        crypto::sign_digest(kbuf, code, 0ull, e[3], e[2], a.raw + t * 32, nullptr, 0, seal, out);
    }
    for (int i = 0; i < 32; ++i) a.sign_dig[t * 32 + i] = out[i];
}

hipError_t launch_mark(const Args& a, hipStream_t s) {
    hipLaunchKernelGGL(bft_twin_byz_kernel, dim3((uint32_t)((a.n_inst + 63) / 64)), dim3(64), 0, s, a);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    hipLaunchKernelGGL(bft_twin_mark_kernel, dim3((uint32_t)((a.M + 1 + 255) / 256)), dim3(256), 0, s, a);
    return hipGetLastError();
}
hipError_t launch_merge(const Args& a, hipStream_t s) {
    const uint64_t k = (a.M > a.n_inst + 1 ? a.M : a.n_inst + 1);
    hipLaunchKernelGGL(bft_twin_merge_kernel, dim3((uint32_t)((k + 255) / 256)), dim3(256), 0, s, a);
    return hipGetLastError();
}
hipError_t launch_prep(const Params& p, const Args& a, hipStream_t s) {
    if (a.T == 0) return hipSuccess;
    hipLaunchKernelGGL(bft_twin_prep_kernel, dim3((uint32_t)((a.T + 63) / 64)), dim3(64), 0, s, p, a);
    return hipGetLastError();
}
hipError_t launch_digest(const Params& p, const Args& a, hipStream_t s) {
    if (a.T == 0) return hipSuccess;
    hipLaunchKernelGGL(bft_twin_digest_kernel, dim3((uint32_t)((a.T + 63) / 64)), dim3(64), 0, s, p, a);
    return hipGetLastError();
}

}  // namespace twins
}  // namespace bft
