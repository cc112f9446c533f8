// bftsim.hip — gfx950 kernels and the C ABI of libbftsim (include/bftsim.h), but for the trace analysers and the
// ledger importer, whose host code is bftsim_observe.hip; what the two files share is bftsim_impl.h.
//
// Kernels:
//   bft_consensus_kernel  one 64-lane wave per 64/S instances (N <= 64), or one workgroup of
//                         S = 128 / 256 lanes per instance (N <= 256); lane = validator (bft_wave.h);
//   bft_consensus_fast_kernel  N = 64 with big-endian seeds: the closed-form phases (bft_fast64.h),
//                         handing instances that need the general path to bft_consensus_resume_kernel;
//   bft_hash_pair_kernel  one lane pair per instance: Keccak-256 of every committed header, chained
//                         through prev_hash (big-endian seeds and power-of-two N, where proposer
//                         seeds are always 0 and the consensus kernel does not need hashes);
//   bft_stats_kernel      per-launch totals for the RCCL all-reduce of the benchmark.
#include <hip/hip_runtime.h>

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <dlfcn.h>
#include <unistd.h>
#include <hipcub/hipcub.hpp>

#include <mutex>
#include <string>
#include <utility>
#include <vector>

#include "bftsim_impl.h"
#include "bft_fast64.h"
#include "bft_crypto.h"
#include "bft_twins.h"

namespace bft {


// ledger export (core/ledger.rs:193-245): the Header bytes of every committed height, thread per
// (instance, height), parent hash from the hash table; into 8-aligned BFTSIM_HEADER_SLOT-byte slots
__global__ __launch_bounds__(256) void bft_export_kernel(Params p, uint8_t* out, uint32_t* lens) {
    const uint64_t t = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    const uint64_t H = p.heights;
    if (t >= (uint64_t)p.n_instances * H) return;
    const uint32_t il = (uint32_t)(t / H), x = (uint32_t)(t % H) + 1u;
    if (x > p.committed_height[il]) { lens[t] = 0; return; }
    uint32_t prev[8];
    if (x == 1) {
        for (int i = 0; i < 8; ++i)
            prev[i] = (uint32_t)p.genesis_hash[4 * i] | ((uint32_t)p.genesis_hash[4 * i + 1] << 8) |
                      ((uint32_t)p.genesis_hash[4 * i + 2] << 16) | ((uint32_t)p.genesis_hash[4 * i + 3] << 24);
    } else {
        const uint32_t* ph = (const uint32_t*)(p.hash + ((uint64_t)il * p.rows + (x - 1)) * 32);
        for (int i = 0; i < 8; ++i) prev[i] = ph[i];
    }
    const uint32_t* row = p.rec + ((uint64_t)il * p.rows + x) * 4;
    const uint32_t prop = row[1] & 0xffffu, var = (row[1] >> 16) & 1u;
    const uint64_t time = p.genesis_time + (uint64_t)p.block_period * ((uint64_t)row[2] + 1ull);
    lens[t] = header_raw((uint64_t*)(out + t * BFTSIM_HEADER_SLOT), prev, p.addresses + 20u * prop, p.seed,
                         p.first_instance + il, x, prop, var, time);
}

// totals: [0] instances [1] committed [2] views [3] ticks [4..10] flag counts (the histograms are
// accumulated by the consensus kernel); block-level reduction in LDS, then one global atomic per
// counter per block
constexpr int STAT_WORDS = 11;
__global__ __launch_bounds__(256) void bft_stats_kernel(Params p, unsigned long long* st) {
    __shared__ unsigned long long acc[STAT_WORDS];
    for (uint32_t k = threadIdx.x; k < STAT_WORDS; k += 256) acc[k] = 0;
    __syncthreads();
    uint32_t il = blockIdx.x * 256u + threadIdx.x;
    if (il < p.n_instances) {
        atomicAdd(&acc[0], 1ull);
        atomicAdd(&acc[1], (unsigned long long)p.committed_height[il]);
        atomicAdd(&acc[2], (unsigned long long)p.views[il]);
        atomicAdd(&acc[3], (unsigned long long)p.ticks[il]);
        uint32_t f = p.flags[il];
        for (int b = 0; b < 7; ++b)
            if (f & (1u << b)) atomicAdd(&acc[4 + b], 1ull);
    }
    __syncthreads();
    for (uint32_t k = threadIdx.x; k < STAT_WORDS; k += 256)
        if (acc[k]) atomicAdd(&st[k], acc[k]);
}

// hash of each instance's block at its committed height (the genesis hash at height 0): it
// commits to the whole chain, so it stands in for the per-height rows in windowed runs
__global__ __launch_bounds__(256) void bft_tip_kernel(Params p, uint8_t* tips) {
    uint32_t il = blockIdx.x * 256u + threadIdx.x;
    if (il >= p.n_instances) return;
    uint32_t ch = p.committed_height[il];
    const uint8_t* src = ch == 0 ? p.genesis_hash
                                 : p.hash + ((uint64_t)il * p.rows + (p.window_mask ? (ch & p.window_mask) : ch)) * 32;
    for (int i = 0; i < 32; ++i) tips[(uint64_t)il * 32 + i] = src[i];
}


// ------------------------------------------------------------------------------ real-crypto mode
// The batched sign / recover pass over a launch's broadcast log (SPEC.md §11; bftsim_crypto_verify).
struct CryptoArgs {
    const uint32_t* mlog;
    const uint32_t* mlog_n;
    uint32_t cap;
    uint32_t n_val;
    const uint64_t* moff;             // [n_inst] first dense message index of each instance
    uint64_t forged[4];
    // dense, per message
    uint64_t* mref;                   // instance * cap + slot
    uint8_t* raw;                     // Subject digest (block hash, zeros for RoundChange)
    uint32_t* key;                    // signing key: sender, or n_val + sender (forged key)
    uint32_t* msg_k;                  // commit seal index
    uint8_t* sign_dig;
    uint8_t* sigs;
    uint8_t* rec_addr;
    uint8_t* rec_ok;
    // dense, per commit
    uint32_t* ncm;
    uint8_t* seal_dig;
    uint8_t* seal_raw;
    uint32_t* seal_key;
    uint8_t* seals;
    uint8_t* seal_ok;
    // results
    uint32_t* inst_ck;                // [n_inst][8] XOR of keccak(signature || seal)
    unsigned long long* counts;       // [8] messages, commits, forged, recovered-as-sender, mismatches, seal errors
};

// crypto_parent / crypto_block_digest (the digest of a logged block id as the run left it): bft_twins.h

// pass 1 (workgroup per instance): digests, signing keys, the commits' seal digests
__global__ __launch_bounds__(64) void bft_crypto_prep_kernel(Params p, CryptoArgs a) {
    __shared__ __attribute__((aligned(16))) uint8_t hb[64 * LANE_HASH_BUF];
    __shared__ uint8_t kb[64 * 136];
    uint8_t* hbuf = hb + threadIdx.x * LANE_HASH_BUF;
    uint8_t* kbuf = kb + threadIdx.x * 136;
    const uint32_t il = blockIdx.x;
    const uint32_t cnt = a.mlog_n[il] < a.cap ? a.mlog_n[il] : a.cap;
    for (uint32_t j = threadIdx.x; j < cnt; j += 64u) {
        const uint32_t* e = a.mlog + ((uint64_t)il * a.cap + j) * MLOG_WORDS;
        const uint64_t m = a.moff[il] + j;
        const uint32_t code = (e[1] >> 8) & 0xffu, sender = e[1] >> 16;
        const bool forged = (e[6] & MLOG_FORGED) != 0;
        uint8_t d[32];
        if (code == MT_ROUND_CHANGE) { for (int i = 0; i < 32; ++i) d[i] = 0; }     // EMPTY_HASH (round_change.rs:55-58)
        else crypto_block_digest(p, il, (uint64_t)e[4] | ((uint64_t)e[5] << 32), hbuf, d);
        for (int i = 0; i < 32; ++i) a.raw[m * 32 + i] = d[i];
        const uint32_t key = sender + (forged ? a.n_val : 0u);
        a.key[m] = key;
        a.mref[m] = (uint64_t)il * a.cap + j;
        if (code == MT_COMMIT) {
            const uint32_t k = atomicAdd(a.ncm, 1u);
            a.msg_k[m] = k;
            a.seal_key[k] = key;
            uint8_t sd[32];
            crypto::seal_digest(kbuf, d, sd);
            for (int i = 0; i < 32; ++i) { a.seal_dig[(uint64_t)k * 32 + i] = sd[i]; a.seal_raw[(uint64_t)k * 32 + i] = d[i]; }
        }
    }
}

// pass 2 (lane per message): the sign digest of the GossipMessage (signature None, the seal of a Commit)
__global__ __launch_bounds__(64) void bft_crypto_digest_kernel(Params p, CryptoArgs a, uint64_t M) {
    __shared__ __attribute__((aligned(16))) uint8_t hb[64 * LANE_HASH_BUF];
    __shared__ uint8_t kb[64 * 136];
    const uint64_t m = (uint64_t)blockIdx.x * 64u + threadIdx.x;
    if (m >= M) return;
    uint8_t* hbuf = hb + threadIdx.x * LANE_HASH_BUF;
    uint8_t* kbuf = kb + threadIdx.x * 136;
    const uint64_t ref = a.mref[m];
    const uint32_t il = (uint32_t)(ref / a.cap);
    const uint32_t* e = a.mlog + ref * MLOG_WORDS;
    const uint32_t code = (e[1] >> 8) & 0xffu, tick = e[0];
    const uint32_t h_ = e[2], r_ = e[3];
    // create_time: RoundChange carries the wall clock in ms (round_change.rs:61), the others 0
    const uint64_t ctime = code == MT_ROUND_CHANGE
                               ? 1000ull * (p.genesis_time + (uint64_t)p.block_period * (uint64_t)tick) : 0ull;
    const uint8_t* seal = code == MT_COMMIT ? a.seals + (uint64_t)a.msg_k[m] * 65 : nullptr;
    uint8_t out[32];
    if (code == MT_PREPREPARE) {
        const uint64_t b = (uint64_t)e[4] | ((uint64_t)e[5] << 32);
        const uint32_t x = blk_h(b), prop = blk_prop(b), var = blk_var(b);
        uint32_t prev[8];
        crypto_parent(p, il, x, prev);
        const uint64_t time = p.genesis_time + (uint64_t)p.block_period * ((uint64_t)blk_T(b) + 1ull);
        const uint32_t hlen = header_raw((uint64_t*)hbuf, prev, p.addresses + 20u * prop, p.seed, p.first_instance + il,
                                         x, prop, var, time);
        crypto::sign_digest(kbuf, code, ctime, r_, h_, nullptr, hbuf, hlen, nullptr, out);
    } else {
        crypto::sign_digest(kbuf, code, ctime, r_, h_, a.raw + m * 32, nullptr, 0, seal, out);
    }
    for (int i = 0; i < 32; ++i) a.sign_dig[m * 32 + i] = out[i];
}

// pass 3 (lane per message): the receivers' checks (handle_message, core.rs:314-322: the recovered
// address must be a validator; verify_commit, commit.rs:94-100: the seal must recover) against what the
// simulation assumed (forged senders dropped, everyone else accepted), and the per-instance checksum
__global__ __launch_bounds__(64) void bft_crypto_check_kernel(Params p, CryptoArgs a, uint64_t M) {
    __shared__ uint8_t kb[64 * 136];
    const uint64_t m = (uint64_t)blockIdx.x * 64u + threadIdx.x;
    if (m >= M) return;
    uint8_t* kbuf = kb + threadIdx.x * 136;
    const uint64_t ref = a.mref[m];
    const uint32_t il = (uint32_t)(ref / a.cap);
    const uint32_t* e = a.mlog + ref * MLOG_WORDS;
    const uint32_t code = (e[1] >> 8) & 0xffu, sender = e[1] >> 16;
    const bool forged = (e[6] & MLOG_FORGED) != 0;
    const uint8_t* ra = a.rec_addr + m * 20;
    bool member = false, as_sender = false;
    if (a.rec_ok[m]) {
        for (uint32_t v = 0; v < a.n_val; ++v) {
            bool eq = true;
            for (int i = 0; i < 20 && eq; ++i) eq = ra[i] == p.addresses[20u * v + i];
            if (eq) { member = true; as_sender = as_sender || v == sender; }
        }
    }
    bool seal_err = false;
    const uint8_t* seal = nullptr;
    if (code == MT_COMMIT) {
        const uint32_t k = a.msg_k[m];
        seal = a.seals + (uint64_t)k * 65;
        seal_err = !a.seal_ok[k];
    }
    const bool mismatch = forged ? member : !as_sender;
    uint8_t t[32];
    crypto::sig_term(kbuf, a.sigs + m * 65, seal, t);
    for (int w = 0; w < 8; ++w) {
        const uint32_t v = (uint32_t)t[4 * w] | ((uint32_t)t[4 * w + 1] << 8) | ((uint32_t)t[4 * w + 2] << 16) |
                           ((uint32_t)t[4 * w + 3] << 24);
        atomicXor(a.inst_ck + (uint64_t)il * 8 + w, v);
    }
    atomicAdd(a.counts + 0, 1ull);
    if (code == MT_COMMIT) atomicAdd(a.counts + 1, 1ull);
    if (forged) atomicAdd(a.counts + 2, 1ull);
    if (as_sender) atomicAdd(a.counts + 3, 1ull);
    if (mismatch) atomicAdd(a.counts + 4, 1ull);
    if (seal_err) atomicAdd(a.counts + 5, 1ull);
}


// pass 4 (lane per message): the signatures of the canonical committer's commit set (the block's votes,
// core.rs:402-413 → backend.rs:163-174): each Commit of height x, the committed round, the committed
// block (or a wildcard), from a sender in that set. seals (bftsim_set_ledger_votes, SPEC.md §11d): the Commit's seal
// a.seals[msg_k[m]] instead, which depends on the block alone and is what verify_seal recovers (backend.rs:343-367)
__global__ __launch_bounds__(64) void bft_crypto_votes_kernel(Params p, CryptoArgs a, uint64_t M, uint8_t* vsig,
                                                              uint8_t* vhas, uint32_t seals) {
    const uint64_t m = (uint64_t)blockIdx.x * 64u + threadIdx.x;
    if (m >= M) return;
    const uint64_t ref = a.mref[m];
    const uint32_t il = (uint32_t)(ref / a.cap);
    const uint32_t* e = a.mlog + ref * MLOG_WORDS;
    const uint32_t code = (e[1] >> 8) & 0xffu, sender = e[1] >> 16, x = e[2], r = e[3];
    if (code != MT_COMMIT || (e[6] & MLOG_OLD) || x == 0 || x > p.committed_height[il]) return;
    const uint32_t* row = p.rec + ((uint64_t)il * p.rows + x) * 4;
    const uint64_t b = (uint64_t)e[4] | ((uint64_t)e[5] << 32);
    if (row[0] != r) return;
    if (!(e[6] & MLOG_WILD) && ((row[1] & 0xffffu) != blk_prop(b) || ((row[1] >> 16) & 1u) != blk_var(b))) return;
    const uint32_t* vo = p.votes + ((uint64_t)il * p.rows + x) * 8;
    if (!((vo[sender >> 5] >> (sender & 31u)) & 1u)) return;
    const uint64_t slot = ((uint64_t)il * p.heights + (x - 1)) * p.n + sender;
    const uint8_t* src = seals ? a.seals + (uint64_t)a.msg_k[m] * 65 : a.sigs + m * 65;
    for (int i = 0; i < 65; ++i) vsig[slot * 65 + i] = src[i];
    vhas[slot] = 1;
}

// the ledger's Header of every committed height with its votes (SPEC.md §11): the header bytes of
// bft_export_kernel with `votes: Some(Votes([signature...]))` in ascending validator order (the
// reference's order is a HashMap's, protocol/mod.rs:183); thread per (instance, height)
__global__ __launch_bounds__(64) void bft_export_votes_kernel(Params p, const uint8_t* vsig, const uint8_t* vhas,
                                                             uint8_t* out, uint64_t slot, uint32_t* lens) {
    __shared__ __attribute__((aligned(16))) uint64_t wbs[64 * HDR_WORDS];
    const uint64_t t = (uint64_t)blockIdx.x * 64u + threadIdx.x;
    const uint64_t H = p.heights;
    if (t >= (uint64_t)p.n_instances * H) return;
    const uint32_t il = (uint32_t)(t / H), x = (uint32_t)(t % H) + 1u;
    if (x > p.committed_height[il]) { lens[t] = 0; return; }
    uint32_t prev[8];
    if (x == 1) {
        for (int i = 0; i < 8; ++i)
            prev[i] = (uint32_t)p.genesis_hash[4 * i] | ((uint32_t)p.genesis_hash[4 * i + 1] << 8) |
                      ((uint32_t)p.genesis_hash[4 * i + 2] << 16) | ((uint32_t)p.genesis_hash[4 * i + 3] << 24);
    } else {
        const uint32_t* ph = (const uint32_t*)(p.hash + ((uint64_t)il * p.rows + (x - 1)) * 32);
        for (int i = 0; i < 8; ++i) prev[i] = ph[i];
    }
    const uint32_t* row = p.rec + ((uint64_t)il * p.rows + x) * 4;
    const uint32_t prop = row[1] & 0xffffu, var = (row[1] >> 16) & 1u;
    const uint64_t time = p.genesis_time + (uint64_t)p.block_period * ((uint64_t)row[2] + 1ull);
    uint64_t* wb = wbs + threadIdx.x * HDR_WORDS;
    const uint32_t hl = header_raw(wb, prev, p.addresses + 20u * prop, p.seed, p.first_instance + il, x, prop, var, time);
    uint8_t* o = out + t * slot;
    const uint8_t* hb = (const uint8_t*)wb;
    uint64_t k = 0;
    for (uint32_t i = 0; i + 1 < hl; ++i) o[k++] = hb[i];        // all but the trailing `votes: None`
    const uint8_t* has = vhas + ((uint64_t)il * H + (x - 1)) * p.n;
    uint32_t nv = 0;
    for (uint32_t v = 0; v < p.n; ++v) nv += has[v];
    if (nv < 16u) o[k++] = (uint8_t)(0x90u | nv);
    else { o[k++] = 0xdc; o[k++] = (uint8_t)(nv >> 8); o[k++] = (uint8_t)nv; }
    for (uint32_t v = 0; v < p.n; ++v) {
        if (!has[v]) continue;
        const uint8_t* sg = vsig + (((uint64_t)il * H + (x - 1)) * p.n + v) * 65;
        o[k++] = 0xdc; o[k++] = 0x00; o[k++] = 65;
        for (int i = 0; i < 65; ++i) {
            if (sg[i] >= 128u) o[k++] = 0xcc;
            o[k++] = sg[i];
        }
    }
    lens[t] = (uint32_t)k;
}

// ------------------------------------------------------------------------------ the trace (SPEC.md §11b)
// The signed wire frame of every logged broadcast (bftsim_export_trace), from what bftsim_crypto_verify kept:
// a size pass (lane per message, the frame emitter of bft_trace.h with a counting functor), a scan, an emit pass.
// the last argument of a trace kernel: nothing for a trace without twins, whose kernels so keep their arguments
template <bool TW> struct TwinOpt {};
template <> struct TwinOpt<true> { TwinArgs a; };
template <bool TW>
__device__ inline const TwinArgs* twin_args(const TwinOpt<TW>& t) {
    if constexpr (TW) return &t.a; else return nullptr;
}
// frame f of the trace -> its dense message; TW (twins on): through the merged index, tw = the frame is the twin
template <bool TW>
__device__ inline uint64_t trace_frame_msg(const TwinArgs* t, uint64_t f, bool& tw) {
    if constexpr (TW) {
        const uint64_t v = t->fmap[f];
        tw = (v & twins::F_TWIN) != 0;
        return v & ~twins::F_TWIN;
    } else {
        tw = false;
        return f;
    }
}
// the frame inputs of dense message m, or of its twin (tw): the same message for the other variant of its block, from
// the twin slot's arrays; hbuf: this lane's LANE_HASH_BUF bytes (a Preprepare's header)
template <bool TW>
__device__ inline trace::Msg trace_msg(const Params& p, const TraceArgs& a, const TwinArgs* ta, uint64_t m, bool tw,
                                       uint8_t* hbuf) {
    const uint64_t ref = a.mref[m];
    const uint32_t il = (uint32_t)(ref / a.cap);
    const uint32_t* e = a.mlog + ref * MLOG_WORDS;
    trace::Msg g;
    g.code = (e[1] >> 8) & 0xffu;
    g.ctime = trace::create_time(g.code, p.genesis_time, p.block_period, e[0]);
    g.height = e[2];
    g.round = e[3];
    g.digest = a.raw + m * 32;
    g.header = nullptr;
    g.hlen = 0;
    g.sig = a.sigs + m * 65;
    g.seal = g.code == MT_COMMIT ? a.seals + (uint64_t)a.msg_k[m] * 65 : nullptr;
    if constexpr (TW) {
        if (tw) {
            const uint64_t t = ta->tslot[m];
            g.digest = ta->traw + t * 32;
            g.sig = ta->tsigs + t * 65;
            g.seal = g.code == MT_COMMIT ? ta->tseals + (uint64_t)ta->tmsg_k[t] * 65 : nullptr;
        }
    }
    if (g.code == MT_PREPREPARE) {
        const uint64_t b = ((uint64_t)e[4] | ((uint64_t)e[5] << 32)) ^ (TW && tw ? twins::BLK_FLIP : 0ull);
        const uint32_t x = blk_h(b), prop = blk_prop(b), var = blk_var(b);
        uint32_t prev[8];
        crypto_parent(p, il, x, prev);
        const uint64_t time = p.genesis_time + (uint64_t)p.block_period * ((uint64_t)blk_T(b) + 1ull);
        g.hlen = header_raw((uint64_t*)hbuf, prev, p.addresses + 20u * prop, p.seed, p.first_instance + il, x, prop, var,
                            time);
        g.header = hbuf;
    }
    return g;
}
// size pass: lens[f] = the frame's length, lens[F] = 0 (the scan's last entry is the total)
template <bool TW>
__global__ __launch_bounds__(64) void bft_trace_size_kernel(Params p, TraceArgs a, uint64_t F, uint64_t* lens, TwinOpt<TW> to) {
    const TwinArgs* t = twin_args(to);
    __shared__ __attribute__((aligned(16))) uint8_t hb[64 * LANE_HASH_BUF];
    const uint64_t f = (uint64_t)blockIdx.x * 64u + threadIdx.x;
    if (f >= F) { if (f == F) lens[F] = 0; return; }
    bool tw;
    const uint64_t m = trace_frame_msg<TW>(t, f, tw);
    lens[f] = trace::frame_len(trace_msg<TW>(p, a, t, m, tw, hb + threadIdx.x * LANE_HASH_BUF));
}

// first byte of each instance: ioff[i] = foff[if0[i]], i <= n_inst (if0: the instances' first frames)
__global__ __launch_bounds__(256) void bft_trace_inst_kernel(const uint64_t* if0, const uint64_t* foff, uint64_t n1,
                                                             uint64_t* ioff) {
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i < n1) ioff[i] = foff[if0[i]];
}
// {tick, phase | code << 8 | sender << 16, flags, instance - inst_begin} of frames [f0, f1); a twin's flags carry
// twins::META_TWIN
template <bool TW>
__global__ __launch_bounds__(256) void bft_trace_meta_kernel(TraceArgs a, uint64_t f0, uint64_t f1, uint32_t inst_begin,
                                                             uint32_t* meta, TwinOpt<TW> to) {
    const TwinArgs* t = twin_args(to);
    const uint64_t f = f0 + (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (f >= f1) return;
    bool tw;
    const uint64_t ref = a.mref[trace_frame_msg<TW>(t, f, tw)];
    const uint32_t* e = a.mlog + ref * MLOG_WORDS;
    ((uint4*)meta)[f - f0] = make_uint4(e[0], e[1], e[6] | (tw ? twins::META_TWIN : 0u), (uint32_t)(ref / a.cap) - inst_begin);
}

// emit pass (`out` holds the frames of [f0, f1)): a wave per 64 consecutive frames, which are one contiguous piece
// of the stream. Each lane expands
// its frame into an LDS stage laid out like that piece (as many whole frames per round as the stage holds), then
// the wave copies the stage out with coalesced 16-byte stores (byte stores for the unaligned head and tail).
// Every lane's writes are bounded by its frame's counted length and the copy by the counted lengths of the
// round's frames, so a disagreement of the two passes only counts in *err. Only a Preprepare needs a header
// buffer: a round takes at most TRACE_PP of them, which keeps the block at 4 per CU.
constexpr uint32_t TRACE_STAGE = 32 * 1024, TRACE_PP = 16;
template <bool TW>
__global__ __launch_bounds__(64) void bft_trace_emit_kernel(Params p, TraceArgs a, uint64_t f0, uint64_t f1,
                                                            const uint64_t* foff, uint8_t* out, uint32_t* err, TwinOpt<TW> to) {
    const TwinArgs* t = twin_args(to);
    __shared__ __attribute__((aligned(16))) uint8_t hb[TRACE_PP * LANE_HASH_BUF];
    __shared__ __attribute__((aligned(16))) uint8_t stage[TRACE_STAGE];
    const uint32_t lane = threadIdx.x;
    const uint64_t fb = f0 + (uint64_t)blockIdx.x * 64u;
    const uint32_t live = (uint32_t)(f1 - fb < 64u ? f1 - fb : 64u);
    const uint64_t f = fb + (lane < live ? lane : live);        // idle lanes: the empty frame at the block's end
    const uint64_t base = foff[f0];
    const uint64_t o0 = foff[f] - base, o1 = foff[lane < live ? f + 1 : f] - base;
    bool tw = false;
    const uint64_t m = TW ? (lane < live ? trace_frame_msg<TW>(t, f, tw) : 0) : f;
    const bool pp = lane < live && ((a.mlog[a.mref[m] * MLOG_WORDS + 1] >> 8) & 0xffu) == (uint32_t)MT_PREPREPARE;
    const uint64_t ppmask = __ballot(pp);
    uint32_t first = 0;
    while (first < live) {                                      // wave-uniform
        const uint64_t r0 = __shfl(o0, (int)first);
        const uint32_t shift = (uint32_t)(r0 & 15u);            // stage byte k = stream byte r0 - shift + k
        // Preprepares among lanes [first, lane): this lane's header slot; both conditions ascend with the lane
        const uint32_t slot = (uint32_t)__popcll((ppmask >> first) & ((1ull << (lane >= first ? lane - first : 0u)) - 1ull));
        const bool fits = lane >= first && o1 - r0 + shift <= TRACE_STAGE && slot + (pp ? 1u : 0u) <= TRACE_PP;
        const uint32_t cnt = (uint32_t)__popcll(__ballot(fits));    // a run of lanes from `first`
        if (cnt == 0) {                                         // one frame above the stage: not produced by any log
            if (lane == first) atomicAdd(err, 1u);
            first += 1;
            continue;
        }
        if (fits && lane < live) {
            const uint32_t len = (uint32_t)(o1 - o0);
            if (trace::write_frame(stage + shift + (uint32_t)(o0 - r0), len,
                                   trace_msg<TW>(p, a, t, m, tw, hb + (pp ? slot : 0u) * LANE_HASH_BUF)) != len)
                atomicAdd(err, 1u);
        }
        __syncthreads();
        const uint32_t end = shift + (uint32_t)(__shfl(o1, (int)(first + cnt - 1u)) - r0);
        uint8_t* dst = out + (r0 - shift);                      // 16-byte aligned
        const uint32_t hi = (shift + 15u) & ~15u;
        const uint32_t b0 = hi < end ? hi : end, b1 = (end & ~15u) > b0 ? (end & ~15u) : b0;
        if (shift + lane < b0) dst[shift + lane] = stage[shift + lane];
        for (uint32_t k = b0 + 16u * lane; k < b1; k += 1024u) *(uint4*)(dst + k) = *(const uint4*)(stage + k);
        if (b1 + lane < end) dst[b1 + lane] = stage[b1 + lane];
        __syncthreads();
        first += cnt;
    }
}

}  // namespace bft

#include "bft_host.h"
using bft::host_keccak;
using bft::host_genesis_hash;

// Attribution pass of scripts/gpu_profile.sh only (BFTSIM_TESTING=1 + BFTSIM_PMC_EVICT=1, never the product path):
// rocprofv3 charges a kernel's dirty L2 lines to whichever later dispatch evicts them, so back-to-back kernels
// borrow each other's write-backs (a resume kernel with no hand-overs charged 30.8 MB). After
// every kernel of a launch this kernel reads 64 MiB (twice the eight XCDs' L2), evicting what the kernel left
// dirty; scripts/pmc_summary.py adds its WRITE_SIZE to the kernel before it.
// a launch's zeroed state in one dispatch (instead of one memset each): the record rows (16 B each), the
// histogram, the FAST kernel's hand-over flags and queue head (null when not a FAST launch)
__global__ __launch_bounds__(256) void bft_clear_kernel(uint4* rec, uint64_t n_rec, uint64_t* hist, uint32_t* resume,
                                                        uint32_t n_resume, uint32_t* resume_q) {
    const uint64_t t = (uint64_t)blockIdx.x * 256u + threadIdx.x, stride = (uint64_t)gridDim.x * 256u;
    for (uint64_t i = t; i < n_rec; i += stride) rec[i] = make_uint4(0u, 0u, 0u, 0u);
    if (resume)
        for (uint64_t i = t; i < n_resume; i += stride) resume[i] = 0u;
    if (t < bft::HIST_BINS) hist[t] = 0ull;
    if (resume_q && t < 2u) resume_q[t] = 0u;
}
__global__ __launch_bounds__(256) void bft_l2_evict_kernel(const uint4* buf, uint64_t n16, uint32_t* sink) {
    uint32_t acc = 0;
    for (uint64_t i = blockIdx.x * 256ull + threadIdx.x; i < n16; i += (uint64_t)gridDim.x * 256ull) {
        const uint4 v = buf[i];
        acc ^= v.x ^ v.y ^ v.z ^ v.w;
    }
    if (acc == 0x9e3779b9u) *sink = acc;              // keeps the loads; the buffer is zero, so never taken
}

// the attribution pass's eviction after a kernel (a no-op unless BFTSIM_TESTING=1 and BFTSIM_PMC_EVICT=1)
static constexpr uint64_t EVICT_BYTES = 64ull << 20;
static hipError_t pmc_evict(bftsim* h, hipStream_t s) {
    if (!h->pmc_evict) return hipSuccess;
    if (!h->d_evict) return hipErrorNotInitialized;   // allocated and zeroed by bftsim_prepare
    hipLaunchKernelGGL(bft_l2_evict_kernel, dim3(2048), dim3(256), 0, s, (const uint4*)h->d_evict, EVICT_BYTES / 16,
                       (uint32_t*)(h->d_evict + EVICT_BYTES / 16));
    return hipGetLastError();
}

template <class T>
static void dev_free(T*& p) {
    (void)hipFree(p);
    p = nullptr;
}

// workgroups of a consensus kernel over n instances: 64 / seg instances per wave, or one per workgroup
static uint64_t launch_blocks(const bftsim* h, uint64_t n) {
    const uint64_t per_block = h->seg > 64 ? 1 : 64 / h->seg;
    return (n + per_block - 1) / per_block;
}

// A row-table set's device buffers for n instances; which ones depends on the mode alone (the configuration, the
// window, sfx_rows, backlog_bytes, the number of sets), so every set of a handle has the same ones. The set's events
// and its hint are not among them: they live as long as the handle.
static int alloc_set(bftsim* h, bftsim::RowSet& r, uint64_t n) {
    const bool n64 = h->seg == 64 && h->cfg.n == 64;
    HIPCHECK(h, hipMalloc(&r.ch, n * 4));
    HIPCHECK(h, hipMalloc(&r.flags, n * 4));
    HIPCHECK(h, hipMalloc(&r.ticks, n * 4));
    HIPCHECK(h, hipMalloc(&r.views, n * 8));
    HIPCHECK(h, hipMalloc(&r.rec, n * h->hcap * 16));
    HIPCHECK(h, hipMalloc(&r.hash, n * h->hcap * 32));
    HIPCHECK(h, hipMalloc(&r.hist, bft::HIST_BINS * sizeof(uint64_t)));
    HIPCHECK(h, hipMalloc(&r.rcs, launch_blocks(h, n) * bft::rcs_words(h->seg, h->rcs_k) * 4));
    if (h->backlog_bytes) HIPCHECK(h, hipMalloc(&r.backlog, h->backlog_bytes));
    if (n64) {                                         // FAST kernel hand-over buffers
        HIPCHECK(h, hipMalloc(&r.resume, n * 4));
        HIPCHECK(h, hipMalloc(&r.resume_q, (n + 2) * 4));
        HIPCHECK(h, hipMalloc(&r.save, (uint64_t)bft::SAVE_WORDS * n * 64 * 4));
    }
    if (h->sfx_rows) {                                 // a hash pass (runs without in-kernel hashes): its suffix rows
        HIPCHECK(h, hipMalloc(&r.sfx, (uint64_t)h->sfx_rows * n * bft::SFX_DEV_DW * 4ull));
        if (n64 && h->n_sets >= 2 && h->sfx_rows >= h->cfg.heights) {   // predicted chains of pipelined FAST launches
            HIPCHECK(h, hipMalloc(&r.byz, n * 8));                      // 
            HIPCHECK(h, hipMalloc(&r.bad, n * 4));
            HIPCHECK(h, hipMalloc(&r.pred, n * h->cfg.heights * 4ull));
        }
    } else if (n64 && !h->window) {
        // little-endian seeds at N = 64: the seed chain's predicted blocks
        HIPCHECK(h, hipMalloc(&r.spec, (uint64_t)(h->cfg.heights + 1u) * n * 4ull));
    }
    return BFTSIM_OK;
}

static void free_set(bftsim::RowSet& r) {
    dev_free(r.ch); dev_free(r.flags); dev_free(r.ticks); dev_free(r.views); dev_free(r.rec); dev_free(r.hash);
    dev_free(r.sfx); dev_free(r.spec); dev_free(r.byz); dev_free(r.bad); dev_free(r.pred);
    dev_free(r.hist); dev_free(r.rcs); dev_free(r.backlog); dev_free(r.resume); dev_free(r.resume_q); dev_free(r.save);
    r.busy = false;
}

static void trace_drop(bftsim* h) {
    if (!h->d_tkeep && !h->d_tfoff && h->trace_n == 0) return;   // the launch path: nothing kept, no HIP call
    (void)hipFree(h->d_tkeep); (void)hipFree(h->d_tfoff); (void)hipFree(h->d_twkeep);
    h->d_tkeep = nullptr; h->d_tfoff = nullptr; h->d_twkeep = nullptr; h->d_tif0 = nullptr;
    h->trace_n = h->trace_M = h->trace_F = 0;
    h->trace_has_twins = false;
    h->twin_counts[0] = h->twin_counts[1] = 0;
    h->trace_moff.clear(); h->trace_ioff.clear();
}

static int sync_all(bftsim* h);
static void free_bufs(bftsim* h) {
    trace_drop(h);
    // a pending chain batch must not outlive its rows: callers sync_all first; a caller that did not (destroy)
    // runs the batch and waits for it here
    if (h->n_pend) (void)sync_all(h);
    h->n_pend = 0;
    h->last_pipe = false;
    for (uint32_t k = 0; k < h->n_sets; ++k) free_set(h->sets[k]);
    h->n_sets = 0;
    h->cur_set = 0;
    dev_free(h->d_trace); dev_free(h->d_tips);
    dev_free(h->d_mlog); dev_free(h->d_mlog_n);
    dev_free(h->d_vsnap); dev_free(h->d_votes); dev_free(h->d_vsig); dev_free(h->d_vhas);
    h->vsig_n = 0;
    h->backlog_bytes = 0;
    h->cap_inst = 0;
    h->n_req = 0;
    h->last_n = 0;                    // nothing left to fetch: the buffers of the last launch are gone
    h->last_first = 0;
    h->last_set = 0;
}

static int flush_batch(bftsim* h, bool final = false);
static int sync_all(bftsim* h) {
    HIPCHECK(h, hipSetDevice(h->device));
    if (int rc = flush_batch(h, true)) return rc;
    HIPCHECK(h, hipStreamSynchronize(h->last_stream));
    for (uint32_t k = 0; k < bftsim::MAX_CS; ++k)
        if (h->cs[k]) HIPCHECK(h, hipStreamSynchronize(h->cs[k]));
    for (uint32_t k = 0; k < bftsim::MAX_HS; ++k)
        if (h->hstr[k]) HIPCHECK(h, hipStreamSynchronize(h->hstr[k]));
    return BFTSIM_OK;
}

#ifdef BFT_STAMPS
static uint64_t* g_stamps = nullptr;
static uint64_t g_stamp_waves = 0;
#endif

// ------------------------------------------------------------------------------ RCCL (multi-GPU)
// The one collective of the path: the run statistics of every rank summed over RCCL.
// librccl is opened on first use (the soname torch also loads, so one copy serves the process);
// the library itself stays loadable without it.
namespace {
struct Rccl {
    ncclResult_t (*get_id)(ncclUniqueId*) = nullptr;
    ncclResult_t (*init_rank)(ncclComm_t*, int, ncclUniqueId, int) = nullptr;
    ncclResult_t (*all_reduce)(const void*, void*, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t,
                               hipStream_t) = nullptr;
    ncclResult_t (*destroy)(ncclComm_t) = nullptr;
    const char* (*err)(ncclResult_t) = nullptr;
    bool ok = false;
    std::string why;
};
Rccl& rccl() {
    static Rccl r;
    static std::once_flag once;
    std::call_once(once, [] {
        void* lib = dlopen("librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
        if (!lib) lib = dlopen("/opt/rocm/lib/librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
        if (!lib) { r.why = std::string("dlopen librccl.so.1: ") + dlerror(); return; }
        r.get_id = (decltype(r.get_id))dlsym(lib, "ncclGetUniqueId");
        r.init_rank = (decltype(r.init_rank))dlsym(lib, "ncclCommInitRank");
        r.all_reduce = (decltype(r.all_reduce))dlsym(lib, "ncclAllReduce");
        r.destroy = (decltype(r.destroy))dlsym(lib, "ncclCommDestroy");
        r.err = (decltype(r.err))dlsym(lib, "ncclGetErrorString");
        r.ok = r.get_id && r.init_rank && r.all_reduce && r.destroy && r.err;
        if (!r.ok) r.why = "librccl.so.1 lacks an entry point";
    });
    return r;
}
// RCCL prints its version banner on stdout at initialisation; the callers' stdout carries results
// (bench.py's one JSON line), so the banner goes to stderr
struct StdoutToStderr {
    int saved;
    StdoutToStderr() {
        fflush(stdout);
        saved = dup(1);
        if (saved >= 0) dup2(2, 1);
    }
    ~StdoutToStderr() {
        fflush(stdout);
        if (saved >= 0) { dup2(saved, 1); close(saved); }
    }
};
void comm_destroy(ncclComm_t c) {
    if (rccl().ok) (void)rccl().destroy(c);
}

}  // namespace

// libbftsig (include/bftsig.h), next to this library, opened on first use (SigApi: bftsim_impl.h)
static void sig_api_anchor() {}
SigApi& sig_api() {
    static SigApi a;
    static std::once_flag once;
    std::call_once(once, [] {
        Dl_info di;
        std::string path = "libbftsig.so";
        if (dladdr((void*)&sig_api_anchor, &di) && di.dli_fname) {
            std::string self = di.dli_fname;
            size_t k = self.rfind('/');
            if (k != std::string::npos) path = self.substr(0, k + 1) + "libbftsig.so";
        }
        void* lib = dlopen(path.c_str(), RTLD_NOW | RTLD_GLOBAL);
        if (!lib) { a.why = std::string("dlopen ") + path + ": " + dlerror(); return; }
        a.create = (decltype(a.create))dlsym(lib, "bftsig_create");
        a.destroy = (decltype(a.destroy))dlsym(lib, "bftsig_destroy");
        a.last_error = (decltype(a.last_error))dlsym(lib, "bftsig_last_error");
        a.secret_to_address = (decltype(a.secret_to_address))dlsym(lib, "bftsig_secret_to_address");
        a.sign = (decltype(a.sign))dlsym(lib, "bftsig_sign");
        a.recover = (decltype(a.recover))dlsym(lib, "bftsig_recover");
        a.ok = a.create && a.destroy && a.last_error && a.secret_to_address && a.sign && a.recover;
        if (!a.ok) a.why = path + " lacks an entry point";
    });
    return a;
}

extern "C" {

#ifdef BFT_STAMPS
// diagnostic builds only: per-section cycle sums of the last launch, summed over waves, into out[0 .. cap);
// returns the number of sections the build stamps (bft::NSTAMP), so a caller sizes its buffer from the library
// (out = nullptr, cap = 0: the count alone) instead of a copy of the constant
int bftsim_debug_stamps(uint64_t* out, uint32_t cap) {
    if (!out || cap == 0) return bft::NSTAMP;
    std::vector<uint64_t> v(g_stamp_waves * bft::NSTAMP);
    if (hipDeviceSynchronize() != hipSuccess) return -2;
    if (hipMemcpy(v.data(), g_stamps, v.size() * 8, hipMemcpyDeviceToHost) != hipSuccess) return -2;
    const uint32_t m = cap < (uint32_t)bft::NSTAMP ? cap : (uint32_t)bft::NSTAMP;
    for (uint32_t k = 0; k < m; ++k) out[k] = 0;
    for (uint64_t w = 0; w < g_stamp_waves; ++w)
        for (uint32_t k = 0; k < m; ++k) out[k] += v[w * bft::NSTAMP + k];
    return bft::NSTAMP;
}
#endif

uint32_t bftsim_two_thirds_majority(uint32_t n) { return (2u * n) / 3u; }
uint32_t bftsim_seed_from_hash(const uint8_t hash[32], uint32_t n) { return n ? bft::seed_from_hash(hash, n) : 0; }
uint32_t bftsim_seed_from_hash_order(const uint8_t hash[32], uint32_t n, uint32_t order) {
    return n ? bft::seed_from_hash(hash, n, order == BFTSIM_SEED_LE) : 0;
}
uint32_t bftsim_calc_proposer(const uint8_t prev_hash[32], uint32_t n, uint64_t round) {
    if (n == 0) return 0;
    return (uint32_t)(((uint64_t)bft::seed_from_hash(prev_hash, n) + round % n) % n);
}
void bftsim_keccak256(const uint8_t* data, size_t len, uint8_t out[32]) { host_keccak(data, len, out); }
void bftsim_genesis_hash(const bftsim_config* cfg, uint8_t out[32]) { host_genesis_hash(cfg, out); }
int bftsim_check_message(uint32_t code, uint64_t msg_height, uint64_t core_height, uint32_t state) {
    if (code < 1 || code > 4 || state < 1 || state > 4 || msg_height >= (1ull << 32) || core_height >= (1ull << 32))
        return BFTSIM_EINVAL;
    return bft::check_message_class((int)code, (uint32_t)msg_height, (uint32_t)core_height, state);
}
int bftsim_view_cmp(uint64_t h1, uint64_t r1, uint64_t h2, uint64_t r2) {
    if (h1 != h2) return h1 < h2 ? -1 : 1;
    if (r1 != r2) return r1 < r2 ? -1 : 1;
    return 0;
}

const char* bftsim_last_error(bftsim_t* h) { return h ? h->err.c_str() : "null handle"; }

int bftsim_create(const bftsim_config* cfg, int hip_device, bftsim_t** out) {
    if (!cfg || !out) return BFTSIM_EINVAL;
    *out = nullptr;
    if (cfg->n < 1 || cfg->n > 256) return BFTSIM_EUNSUPPORTED;
    if (cfg->heights < 1 || cfg->heights > (1u << 20) || cfg->max_ticks < 1 || cfg->max_ticks > (1u << 28) ||
        !cfg->addresses || cfg->phase_cap < 1 || cfg->phase_cap > 255 || cfg->block_period < 1)
        return BFTSIM_EINVAL;
    for (uint32_t i = 1; i < cfg->n; ++i)
        if (memcmp(cfg->addresses + 20 * (i - 1), cfg->addresses + 20 * i, 20) >= 0) return BFTSIM_EINVAL;
    if (cfg->seed_byte_order > BFTSIM_SEED_LE || cfg->header_encoding != BFTSIM_ENC_RMP_COMPACT ||
        cfg->backlog_mode > BFTSIM_BACKLOG_REPLAY || cfg->reserved != 0)
        return BFTSIM_EINVAL;
    bftsim* h = new bftsim();
    h->cfg = *cfg;
    h->addresses.assign(cfg->addresses, cfg->addresses + 20 * cfg->n);
    h->cfg.addresses = h->addresses.data();
    h->device = hip_device;
    host_genesis_hash(&h->cfg, h->genesis_hash);
    h->genesis_seed = bft::seed_from_hash(h->genesis_hash, cfg->n, cfg->seed_byte_order == BFTSIM_SEED_LE);
    h->seg = bft::segment_size(cfg->n);
    h->hcap = cfg->heights + 64;
    *out = h;
    hipError_t e = hipSetDevice(hip_device);
    if (e != hipSuccess) return fail(h, BFTSIM_EHIP, std::string("hipSetDevice: ") + hipGetErrorString(e));
    HIPCHECK(h, hipMalloc(&h->d_addr, 20 * cfg->n));
    HIPCHECK(h, hipMemcpy(h->d_addr, h->addresses.data(), 20 * cfg->n, hipMemcpyHostToDevice));
    HIPCHECK(h, hipMalloc(&h->d_ghash, 32));
    HIPCHECK(h, hipMemcpy(h->d_ghash, h->genesis_hash, 32, hipMemcpyHostToDevice));
    HIPCHECK(h, hipMalloc(&h->d_stats, 16 * sizeof(unsigned long long)));
    for (uint32_t i = 0; i < bftsim::RING; ++i) {
        HIPCHECK(h, hipEventCreate(&h->ring[i].c0)); HIPCHECK(h, hipEventCreate(&h->ring[i].c1));
        HIPCHECK(h, hipEventCreate(&h->ring[i].h0)); HIPCHECK(h, hipEventCreate(&h->ring[i].h1));
        HIPCHECK(h, hipEventCreateWithFlags(&h->ring[i].sx, hipEventDisableTiming));
    }
    for (uint32_t i = 0; i < bftsim::MAX_SETS; ++i)
        HIPCHECK(h, hipEventCreateWithFlags(&h->sets[i].done, hipEventDisableTiming));
    return BFTSIM_OK;
}

void bftsim_destroy(bftsim_t* h) {
    if (!h) return;
    (void)hipSetDevice(h->device);
    free_bufs(h);
    (void)hipFree(h->d_addr); (void)hipFree(h->d_ghash); (void)hipFree(h->d_stats);
    (void)hipFree(h->d_red);
    (void)hipFree(h->d_evict);
    (void)hipFree(h->d_keys);
    if (h->comm) comm_destroy(h->comm);
    if (h->sig) sig_api().destroy(h->sig);
    for (uint32_t i = 0; i < bftsim::RING; ++i) {
        if (h->ring[i].c0) (void)hipEventDestroy(h->ring[i].c0);
        if (h->ring[i].c1) (void)hipEventDestroy(h->ring[i].c1);
        if (h->ring[i].h0) (void)hipEventDestroy(h->ring[i].h0);
        if (h->ring[i].h1) (void)hipEventDestroy(h->ring[i].h1);
        if (h->ring[i].sx) (void)hipEventDestroy(h->ring[i].sx);
    }
    for (uint32_t i = 0; i < bftsim::MAX_SETS; ++i) {
        if (h->sets[i].done) (void)hipEventDestroy(h->sets[i].done);
        h->sets[i].batch_done = nullptr;
        if (h->sets[i].entry) (void)hipEventDestroy(h->sets[i].entry);
        if (h->sets[i].hint) (void)hipHostFree(h->sets[i].hint);
    }
    for (uint32_t i = 0; i < bftsim::BATCH_EVS; ++i)
        if (h->batch_ev[i]) (void)hipEventDestroy(h->batch_ev[i]);
    for (uint32_t i = 0; i < bftsim::MAX_CS; ++i)
        if (h->cs[i]) (void)hipStreamDestroy(h->cs[i]);
    for (uint32_t i = 0; i < bftsim::MAX_HS; ++i)
        if (h->hstr[i]) (void)hipStreamDestroy(h->hstr[i]);
    delete h;
}

// What a launch runs. It follows from the configuration and the handle's switches, never from the row-table set the
// launch gets (every set has the same buffers, so set 0 answers for all):
//   need_seed  the consensus kernel hashes each block itself (no hash pass): proposers depend on the hashes, or the
//              rows are a ring (window);
//   fast       FAST + resume for N = 64: big-endian seeds (proposer 0, hashes in the post-pass) or little-endian seeds
//              (spec: the seed chain's predictions, else hashes in-kernel); not for windowed rows, traces or the opt-in
//              modes;
//   pipe       on the launch streams with a set of the ring; not with per-launch host state (traces, the crypto log,
//              which the next calls read from the last launch alone).
struct LaunchMode { bool need_seed, fast, spec, pipe; };
static LaunchMode launch_mode(const bftsim* h) {
    const bft::Params c = bft::params_from_config(h->cfg, h->seg, h->hcap, h->genesis_seed, 0, 1);
    const bool mlog = h->crypto && h->d_mlog;          // one message at a time (make_params)
    LaunchMode m;
    m.need_seed = c.need_seed || h->window;
    m.fast = h->fast && c.fast && !mlog && h->sets[0].save && !h->window && !h->h_trace && h->seg == 64 &&
             h->cfg.n == 64;
    m.spec = m.fast && m.need_seed && h->seed_spec && h->sets[0].spec;
    m.pipe = h->pipeline >= 2 && (!m.need_seed || m.spec) && h->n_sets >= 2 && !h->h_trace && !mlog;
    return m;
}

int bftsim_prepare(bftsim_t* h, uint64_t n) {
    if (!h || n == 0 || n > (1ull << 31)) return fail(h, BFTSIM_EINVAL, "bad instance count");
    HIPCHECK(h, hipSetDevice(h->device));
    trace_drop(h);
    if (n <= h->cap_inst) { h->n_req = n; return BFTSIM_OK; }
    if (h->last_n) if (int rc = sync_all(h)) return rc;   // the last launch may still use them
    free_bufs(h);
    HIPCHECK(h, hipMalloc(&h->d_tips, n * 32));
    if (h->crypto) {
        HIPCHECK(h, hipMalloc(&h->d_mlog, n * (uint64_t)h->mlog_cap * bft::MLOG_WORDS * 4));
        HIPCHECK(h, hipMalloc(&h->d_mlog_n, n * 4));
        HIPCHECK(h, hipMalloc(&h->d_vsnap, n * (uint64_t)h->seg * 8 * 4));
        HIPCHECK(h, hipMalloc(&h->d_votes, n * (uint64_t)h->hcap * 8 * 4));
    }
    // the switches of the tests and the A/B scripts, read only under BFTSIM_TESTING=1 (never the product path): a
    // 32-bit one clamped to [lo, hi], a 64-bit one as written; both say whether the variable was set
    const char* tst = getenv("BFTSIM_TESTING");
    const bool testing = tst && strcmp(tst, "1") == 0;
    auto knob = [&](const char* name, uint32_t& v, uint32_t lo, uint32_t hi) {
        const char* e = getenv(name);
        if (!testing || !e) return false;
        const uint32_t x = (uint32_t)atoi(e);
        v = x < lo ? lo : x > hi ? hi : x;
        return true;
    };
    auto knob64 = [&](const char* name, uint64_t& v) {
        const char* e = getenv(name);
        if (!testing || !e) return false;
        v = strtoull(e, nullptr, 10);
        return true;
    };
    uint32_t sfx_cap = 0;             // fewer heights per suffix-row chunk, so that small batches take the chunked path
    {
        knob64("BFTSIM_CHAIN_WAVE_MAX", h->chain_wave_max);
        knob64("BFTSIM_CHAIN_LANE_MIN", h->chain_lane_min);
        knob("BFTSIM_LAUNCH_STREAMS", h->n_cs, 1, bftsim::MAX_CS);
        knob("BFTSIM_CHAIN_GRID", h->chain_grid, 0, 1u << 20);
        knob("BFTSIM_CHAIN_INLINE", h->chain_inline, 0, 1);
        knob("BFTSIM_HASH_STREAMS", h->n_hs, 1, bftsim::MAX_HS);
        knob("BFTSIM_HASH_BATCH", h->hash_batch, 1, bftsim::MAX_BATCH);   // (bftsim_set_hash_batch)
        knob("BFTSIM_SFX_ROWS", sfx_cap, 0, 0x7fffffffu);
        uint32_t ss = h->seed_spec, hs = 0, pe = 0;
        knob("BFTSIM_SEED_SPEC", ss, 0, 1);
        h->seed_spec = ss != 0;
        // 0: off, any other value: at every size; 2: lossy schedules too (the tests of the repairs)
        if (knob("BFTSIM_HASH_SPEC", hs, 0, ~0u)) h->hash_spec_max = hs ? ~0ull : 0ull;
        h->spec_lossy = hs == 2;
        knob("BFTSIM_PMC_EVICT", pe, 0, 1);            // scripts/gpu_profile.sh's attribution pass
        h->pmc_evict = pe != 0;
        if (h->pmc_evict && !h->d_evict) {          // before any launch, so every eviction is the same dispatch
            HIPCHECK(h, hipMalloc(&h->d_evict, EVICT_BYTES + 16));
            HIPCHECK(h, hipMemset(h->d_evict, 0, EVICT_BYTES + 16));
        }
    }
    // the hash pass's suffix rows (runs without in-kernel hashes): every height in one chunk up to 2 GiB
    // per set, fewer heights per chunk beyond
    h->sfx_rows = 0;
    if (!launch_mode(h).need_seed) {
        uint64_t rows = (2ull << 30) / (n * bft::SFX_DEV_DW * 4ull);
        if (rows < 1) rows = 1;
        if (rows > h->cfg.heights) rows = h->cfg.heights;
        if (sfx_cap > 0 && sfx_cap < rows) rows = sfx_cap;   // tests only (BFTSIM_SFX_ROWS)
        if (rows * n >= (1ull << 32)) rows = ((1ull << 32) - 1) / n;
        h->sfx_rows = (uint32_t)rows;
    }
    if (h->cfg.backlog_mode == BFTSIM_BACKLOG_REPLAY)
        h->backlog_bytes = launch_blocks(h, n) * bft::backlog_words(h->seg) * 4;
    // the sets: one, or the ring of the pipelined mode. Counted before they are filled, so that a prepare that fails
    // half-way leaves nothing that free_bufs does not find
    h->n_sets = h->pipeline > 1 ? (uint32_t)h->pipeline : 1u;
    for (uint32_t k = 0; k < h->n_sets; ++k)
        if (int rc = alloc_set(h, h->sets[k], n)) return rc;
    // every stream of the pipelined mode now, while the HIP runtime still has hardware queues of its own to
    // give each (streams created later in a busy process can share one, which serializes their batches)
    if (h->sfx_rows && h->n_sets >= 2) {
        for (uint32_t k = 0; k < h->n_cs && k < bftsim::MAX_CS; ++k)
            if (!h->cs[k]) HIPCHECK(h, hipStreamCreateWithFlags(&h->cs[k], hipStreamNonBlocking));
        const uint32_t nh = h->n_hs > bftsim::N_HS_SPEC ? h->n_hs : bftsim::N_HS_SPEC;
        for (uint32_t k = 0; k < nh && k < bftsim::MAX_HS; ++k)
            if (!h->hstr[k]) HIPCHECK(h, hipStreamCreateWithFlags(&h->hstr[k], hipStreamNonBlocking));
    }
    h->cap_inst = n;
    h->n_req = n;
    return BFTSIM_OK;
}

int bftsim_set_window(bftsim_t* h, uint32_t window) {
    if (!h) return BFTSIM_EINVAL;
    if (window != 0 && (window < 64 || (window & (window - 1)) != 0 || window > (1u << 20)))
        return fail(h, BFTSIM_EINVAL, "window must be 0 or a power of two in [64, 2^20]");
    if (window == h->window) return BFTSIM_OK;
    if (h->last_stream) if (int rc = sync_all(h)) return rc;   // pending chains use the buffers freed below
    h->window = window;
    h->hcap = window ? window : h->cfg.heights + 64;
    (void)hipSetDevice(h->device);
    free_bufs(h);                                   // row tables are re-sized by the next prepare
    return BFTSIM_OK;
}

int bftsim_set_rcs_capacity(bftsim_t* h, uint32_t rounds) {
    if (!h) return BFTSIM_EINVAL;
    if (rounds < 1 || rounds > bft::RCS_MAX_K) return fail(h, BFTSIM_EINVAL, "RoundChangeSet capacity must be 1..4096");
    if (rounds == h->rcs_k) return BFTSIM_OK;
    if (h->last_stream) if (int rc = sync_all(h)) return rc;
    h->rcs_k = rounds;
    (void)hipSetDevice(h->device);
    free_bufs(h);                                   // the tables are re-sized by the next prepare
    return BFTSIM_OK;
}

int bftsim_set_fast(bftsim_t* h, int on) {
    if (!h) return BFTSIM_EINVAL;
    h->fast = on != 0;
    return BFTSIM_OK;
}

int bftsim_set_trace(bftsim_t* h, uint64_t* host_out, uint32_t trace_ticks) {
    if (!h) return BFTSIM_EINVAL;
    h->h_trace = host_out;
    h->trace_ticks = host_out ? trace_ticks : 0;
    return BFTSIM_OK;
}

// The launch parameters of instances [first, first + n) on row-table set r. Whatever reads a launch's results builds
// them again over the last launch's set. The FAST kernels' hand-over fields are not filled here: only a FAST launch
// has them (run_consensus).
static bft::Params make_params(bftsim* h, const bftsim::RowSet& r, uint64_t first, uint64_t n) {
    bft::Params p = bft::params_from_config(h->cfg, h->seg, h->hcap, h->genesis_seed, first, n);
    p.addresses = h->d_addr;
    p.genesis_hash = h->d_ghash;
    p.committed_height = r.ch;
    p.flags = r.flags;
    p.ticks = r.ticks;
    p.views = r.views;
    p.rec = r.rec;
    p.hash = r.hash;
    p.trace = h->d_trace;
    p.trace_ticks = h->trace_ticks;
    p.hist = r.hist;
    p.rcs = r.rcs;
    p.rcs_k = h->rcs_k;
    p.chain_prio = bftsim::PRIO_RECORDED;
    p.chain_grid = h->chain_grid;
    p.chain_inline = h->chain_inline;
    p.backlog = r.backlog;
    if (h->crypto && h->d_mlog) {
        p.mlog = h->d_mlog;
        p.mlog_n = h->d_mlog_n;
        p.mlog_cap = h->mlog_cap;
        for (int k = 0; k < 4; ++k) p.forged[k] = h->forged[k];
        p.vsnap = h->d_vsnap;
        p.votes = h->d_votes;
        p.fast = 0;                  // one message at a time: the commit set at the commit instant (votes)
    }
    if (h->window) {
        p.window_mask = h->window - 1;
        p.rows = h->window;
        p.hcap = h->cfg.heights + 64;               // height limit; rows live in the ring
        p.need_seed = 1;                            // hashes in-kernel: no post-pass over a ring
    }
    return p;
}

// which chain kernel hashes a batch of launches of n instances (the wave kernel has no predicted / repair mode)
static uint32_t chain_kind(const bftsim* h, uint64_t n, bool spec) {
    if (n >= h->chain_lane_min && 4ull * n < (1ull << 24)) return bft::CHAIN_KERNEL_LANE;   // its 24-bit offsets
    if (!spec && n <= h->chain_wave_max) return bft::CHAIN_KERNEL_WAVE;
    return bft::CHAIN_KERNEL_PAIR;
}

// predicted chains are for lossless schedules (no drops, no proposer crashes), where the canonical tick
// commits every height; with drops most instances leave it early and the predicted chains would mostly be repaired
// (drop64: 22.6 ms of chain kernels per launch against 0.7)
static bool predictable(const bftsim* h, const bft::Params& p) {
    return (p.thr16 == 0 && p.crash_on == 0) || h->spec_lossy;
}

static uint32_t clear_blocks(uint64_t n_rec) {   // bft_clear_kernel's grid: grid-stride, at least one block
    const uint64_t b = (n_rec + 255u) / 256u;
    return (uint32_t)(b < 1 ? 1 : b > 4096 ? 4096 : b);
}

// a launch's kernel times into the sums that bftsim_kernel_ms_sum reports, once its kernels are done
static int fold_ev(bftsim* h, bftsim::LaunchEv& ev) {
    HIPCHECK(h, hipEventSynchronize(ev.has_hash ? ev.h1 : ev.c1));
    float a = 0, b = 0;
    HIPCHECK(h, hipEventElapsedTime(&a, ev.c0, ev.c1));
    if (ev.has_hash) HIPCHECK(h, hipEventElapsedTime(&b, ev.h0, ev.h1));
    h->acc_c += a; h->acc_h += b; h->acc_n += 1;
    ev.pending = false;
    return BFTSIM_OK;
}

// stream t's work so far is the last that uses the set: its next launch waits for it
static int set_done(bftsim* h, bftsim::RowSet& r, hipStream_t t) {
    HIPCHECK(h, hipEventRecord(r.done, t));
    r.batch_done = nullptr;
    r.busy = true;
    return BFTSIM_OK;
}

// A launch, step 1: its row-table set and its stream. Unpipelined: set 0 on the caller's stream s, once the pipelined
// launches before it are done (they may still use set 0); the ring's cursor stays. Pipelined: the next set in the
// ring, once its last launch's chains are done (a launch of it still waiting in the hash batch is flushed first), on
// the next launch stream, after the caller's earlier work on s.
static int choose_set(bftsim* h, const LaunchMode& m, hipStream_t& s, uint32_t& set) {
    set = 0;
    if (!m.pipe) {
        if (h->last_pipe) {
            if (int rc = sync_all(h)) return rc;
            h->last_pipe = false;
        }
        return BFTSIM_OK;
    }
    set = h->cur_set = (h->cur_set + 1) % h->n_sets;
    for (uint32_t i = 0; i < h->n_pend; ++i)
        if (h->pend[i].set == set) { if (int rc = flush_batch(h)) return rc; break; }
    bftsim::RowSet& r = h->sets[set];
    if (!r.entry) HIPCHECK(h, hipEventCreateWithFlags(&r.entry, hipEventDisableTiming));
    HIPCHECK(h, hipEventRecord(r.entry, s));
    h->cur_cs = (h->cur_cs + 1) % (m.spec ? bftsim::N_CS_SEEDED : h->n_cs);
    if (!h->cs[h->cur_cs]) HIPCHECK(h, hipStreamCreateWithFlags(&h->cs[h->cur_cs], hipStreamNonBlocking));
    s = h->cs[h->cur_cs];
    HIPCHECK(h, hipStreamWaitEvent(s, r.entry, 0));
    if (r.busy) HIPCHECK(h, hipStreamWaitEvent(s, r.batch_done ? r.batch_done : r.done, 0));
    h->last_pipe = true;
    return BFTSIM_OK;
}

// Step 2: the set's state zeroed, then the consensus kernels on stream s, between the launch's events c0 and c1
static int run_consensus(bftsim* h, const LaunchMode& m, bftsim::RowSet& r, hipStream_t s, bftsim::LaunchEv& ev,
                         bft::Params& p) {
    const uint64_t n = p.n_instances;
    // the histogram and (FAST launches) the hand-over flags and queue zeroed by one dispatch; the record rows too,
    // except for FAST launches: the FAST and resume bodies read a row only once they have recorded it (canon_blk,
    // canon_seed, refresh_tip_from_table: rows <= the canonical height), and every reader after the launch stops at
    // the committed height (fetch, export, tips, chains, the predicted chains' check) -- 43 MB of writes per cfg3
    // launch saved
    const uint64_t n_rec = m.fast ? 0 : n * h->hcap;
    hipLaunchKernelGGL(bft_clear_kernel, dim3(clear_blocks(n_rec > n ? n_rec : n)), dim3(256), 0, s, (uint4*)r.rec,
                       n_rec, r.hist, m.fast ? r.resume : nullptr, (uint32_t)n, m.fast ? r.resume_q : nullptr);
    HIPCHECK(h, hipGetLastError());
    if (r.backlog) HIPCHECK(h, hipMemsetAsync(r.backlog, 0, h->backlog_bytes, s));
    const dim3 grid((uint32_t)launch_blocks(h, n));
    const size_t lds = bft::lds_bytes(h->seg, p.need_seed != 0);
    HIPCHECK(h, hipEventRecord(ev.c0, s));
    if (m.fast) {
        // FAST kernel over every instance, then the full kernel over the ones it handed over
        p.resume_flags = r.resume;
        p.resume_q = r.resume_q;
        p.save = r.save;
        p.save_stride = n * 64;
        if (!r.hint) {
            HIPCHECK(h, hipHostMalloc((void**)&r.hint, 4, hipHostMallocMapped | hipHostMallocCoherent));
            *r.hint = 0xffffffffu;                    // unknown: the full grid, or another set's last count
            for (uint32_t k = 0; k < h->n_sets; ++k)  // (the grid only paces the persistent waves)
                if (h->sets[k].hint && &h->sets[k] != &r && *h->sets[k].hint != 0xffffffffu) {
                    *r.hint = __atomic_load_n(h->sets[k].hint, __ATOMIC_RELAXED);
                    break;
                }
        }
        p.resume_hint = r.hint;
        if (m.spec) {                                    // the predicted blocks first (little-endian seeds)
            p.spec = r.spec;
            HIPCHECK(h, bft::launch_seed_chain((uint32_t)n, s, p));
            HIPCHECK(h, pmc_evict(h, s));
        }
        HIPCHECK(h, bft::launch_fast(grid, s, p));
        HIPCHECK(h, pmc_evict(h, s));
        HIPCHECK(h, bft::launch_resume(grid, lds, s, p));
        HIPCHECK(h, pmc_evict(h, s));
    } else {
        const bool ext = p.backlog_replay || p.mlog;   // the opt-in modes' kernel build (MODE_EXT)
        HIPCHECK(h, bft::launch_general(p.need_seed != 0, ext, h->seg, grid, lds, s, p));
        HIPCHECK(h, pmc_evict(h, s));
    }
    HIPCHECK(h, hipEventRecord(ev.c1, s));
    ev.has_hash = !p.need_seed;
    ev.pending = true;
    return BFTSIM_OK;
}

// Step 3 (runs without in-kernel hashes): the launch's hash pass, or its place in the batch whose chains one kernel
// runs (flush_batch). s: the launch's stream; ev: its events, the ring's last
static int run_hash_pass(bftsim* h, const LaunchMode& m, uint32_t set, hipStream_t s, bftsim::LaunchEv& ev,
                         const bft::Params& p, uint64_t first) {
    bftsim::RowSet& r = h->sets[set];
    const uint64_t n = p.n_instances;
    const uint32_t H = h->cfg.heights, K = h->sfx_rows;
    // Where the suffix rows go depends on how long the consensus kernel runs against the chains
    // (A/B, profiles/r03/ab_sfx): the N = 64 FAST kernel is short, so a full-chip pass by a thread per
    // (instance, height) runs on the launch stream right behind it; the general kernels run far longer
    // than the chains, so a thread per instance over its heights runs on the hash stream beside them.
    if (m.pipe && K >= H && m.fast) {
        // big-endian seeds: predicted chains
        const bool hspec = r.byz && n < h->hash_spec_max && predictable(h, p);
        if (!hspec) {
            // suffix rows now (unless the lane chains encode them); the chains in the next batch (flush_batch)
            if (!(h->chain_inline && chain_kind(h, n, false) == bft::CHAIN_KERNEL_LANE)) {
                HIPCHECK(h, bft::launch_hash_suffix((uint32_t)n, 1, K, r.sfx, false, s, p));
                HIPCHECK(h, pmc_evict(h, s));
            }
            HIPCHECK(h, hipEventRecord(ev.sx, s));
        }
        ev.has_hash = false;                          // the batch's last launch carries the chain time
        // one chain kernel runs every pending launch with the batch's sizes (suffix-row stride, grid):
        // a launch of another size starts a batch of its own
        if (h->n_pend > 0 && (h->batch_p.n_instances != p.n_instances || h->batch_spec != hspec))
            if (int rc = flush_batch(h)) return rc;
        if (h->n_pend == 0) {
            h->batch_p = p;
            h->batch_spec = hspec;
            h->cur_hs = (h->cur_hs + 1) % (hspec ? bftsim::N_HS_SPEC : h->n_hs);   // the batch's hash stream
            if (!h->hstr[h->cur_hs]) HIPCHECK(h, hipStreamCreateWithFlags(&h->hstr[h->cur_hs], hipStreamNonBlocking));
            h->batch_hs = h->cur_hs;
        }
        h->pend[h->n_pend++] = {set, (h->ring_head - 1) % bftsim::RING, (uint32_t)first, h->cur_cs};
        if (h->n_pend >= h->hash_batch) return flush_batch(h);
        return BFTSIM_OK;
    }
    // one launch's hash pass: on a hash stream (pipelined) or the launch stream; chunks of K heights
    // share the suffix rows (suffix and chain kernels in order on one stream)
    hipStream_t t = s;
    if (m.pipe) {
        h->cur_hs = (h->cur_hs + 1) % h->n_hs;
        if (!h->hstr[h->cur_hs]) HIPCHECK(h, hipStreamCreateWithFlags(&h->hstr[h->cur_hs], hipStreamNonBlocking));
        t = h->hstr[h->cur_hs];
        HIPCHECK(h, hipStreamWaitEvent(t, ev.c1, 0));
    }
    HIPCHECK(h, hipEventRecord(ev.h0, t));
    const uint32_t kind = chain_kind(h, n, false);
    for (uint32_t x0 = 1; x0 <= H; x0 += K) {
        if (!(h->chain_inline && kind == bft::CHAIN_KERNEL_LANE)) {
            HIPCHECK(h, bft::launch_hash_suffix((uint32_t)n, x0, K, r.sfx, !m.fast, t, p));
            HIPCHECK(h, pmc_evict(h, t));
        }
        HIPCHECK(h, bft::launch_hash_chain((uint32_t)n, x0, K, r.sfx, kind, t, p));
        HIPCHECK(h, pmc_evict(h, t));
    }
    HIPCHECK(h, hipEventRecord(ev.h1, t));
    return m.pipe ? set_done(h, r, t) : BFTSIM_OK;
}

int bftsim_launch(bftsim_t* h, uint64_t first, void* stream) {
    if (!h || h->cap_inst == 0 || h->n_req == 0) return fail(h, BFTSIM_EINVAL, "bftsim_prepare not called");
    const uint64_t n = h->n_req;
    if (first + n > (1ull << 32)) return fail(h, BFTSIM_EINVAL, "instance ids must fit in 32 bits");
    {   // the device current already (the common case): hipGetDevice is a thread-local read, hipSetDevice is not
        int d = -1;
        if (hipGetDevice(&d) != hipSuccess || d != h->device) HIPCHECK(h, hipSetDevice(h->device));
    }
    hipStream_t s = (hipStream_t)stream;
    if (h->h_trace) {
        if (h->d_trace) (void)hipFree(h->d_trace);
        h->d_trace = nullptr;
        size_t tb = n * (size_t)h->trace_ticks * h->cfg.n * 8;
        HIPCHECK(h, hipMalloc(&h->d_trace, tb));
        HIPCHECK(h, hipMemsetAsync(h->d_trace, 0, tb, s));
    }
#ifdef BFT_STAMPS
    {   // on the caller's stream, ahead of the launch's entry event
        static uint64_t* d_st = nullptr;
        static uint64_t cap = 0;
        uint64_t waves = launch_blocks(h, n);
        if (waves > cap) { (void)hipFree(d_st); HIPCHECK(h, hipMalloc(&d_st, waves * 8 * bft::NSTAMP)); cap = waves; }
        HIPCHECK(h, hipMemsetAsync(d_st, 0, waves * 8 * bft::NSTAMP, s));
        g_stamps = d_st;
        g_stamp_waves = waves;
    }
#endif
    const LaunchMode m = launch_mode(h);
    uint32_t set = 0;
    if (int rc = choose_set(h, m, s, set)) return rc;
    bftsim::RowSet& r = h->sets[set];
    bft::Params p = make_params(h, r, first, n);
#ifdef BFT_STAMPS
    p.stamps = g_stamps;
#endif
    bftsim::LaunchEv& ev = h->ring[h->ring_head % bftsim::RING];
    if (ev.pending) if (int rc = fold_ev(h, ev)) return rc;   // 64 launches unread: fold the oldest in
    h->ring_head += 1;
    if (int rc = run_consensus(h, m, r, s, ev, p)) return rc;
    if (!m.need_seed) {
        if (int rc = run_hash_pass(h, m, set, s, ev, p, first)) return rc;
    } else if (m.pipe) {                                // no hash pass: the set is free once this launch is done
        if (int rc = set_done(h, r, s)) return rc;
    }
    h->last_n = n;
    h->vsig_n = 0;
    trace_drop(h);
    h->last_first = first;
    h->last_set = set;
    h->last_stream = s;
    return BFTSIM_OK;
}

// the chains of the pending launches as one kernel on the next hash stream, after each launch's suffix rows
// `final`: the flush of bftsim_sync (the last launches of a burst), whose chains are the burst's tail
static int flush_batch(bftsim* h, bool final) {
    if (h->n_pend == 0) return BFTSIM_OK;
    hipStream_t t = h->hstr[h->batch_hs];           // chosen at the batch's first launch
    // A final batch of recorded chains (lossless schedules with predictions off, BFTSIM_HASH_SPEC=0: lane chains that
    // start once the last launch's consensus kernel is done and take ~2 ms) runs as predicted lane-pair chains
    // instead: they start now, beside the launches' consensus kernels, and only the check and the repairs are left
    // behind them. With predictions on (the default) every batch is predicted already (§4j).
    const bool conv = final && !h->batch_spec && h->sets[h->pend[0].set].byz != nullptr && predictable(h, h->batch_p);
    const bool spec = h->batch_spec || conv;
    bft::ChainSets cs{};
    cs.count = h->n_pend;
    // a launch stream runs its launches in order, so the last pending launch of each launch stream stands for the
    // others: per stream one wait on its sx (recorded after the consensus kernels and, unless the lane chains encode
    // them, the suffix rows) instead of one wait per launch
    int32_t last_on[bftsim::MAX_CS];
    for (uint32_t k = 0; k < bftsim::MAX_CS; ++k) last_on[k] = -1;
    for (uint32_t i = 0; i < h->n_pend; ++i) last_on[h->pend[i].cs] = (int32_t)i;
    if (!spec) {
        for (uint32_t k = 0; k < bftsim::MAX_CS; ++k)
            if (last_on[k] >= 0) HIPCHECK(h, hipStreamWaitEvent(t, h->ring[h->pend[last_on[k]].ev].sx, 0));
    } else {
        // predicted chains need only their sets free, not the launch streams' earlier kernels: the caller's work
        // before the last pending launch (its entry event: the caller's stream is in order) and each distinct
        // previous hash pass of the sets
        HIPCHECK(h, hipStreamWaitEvent(t, h->sets[h->pend[h->n_pend - 1].set].entry, 0));
        hipEvent_t seen[bftsim::MAX_BATCH];
        uint32_t ns = 0;
        for (uint32_t i = 0; i < h->n_pend; ++i) {
            const bftsim::RowSet& r = h->sets[h->pend[i].set];
            if (!r.busy) continue;
            const hipEvent_t e = r.batch_done ? r.batch_done : r.done;
            bool dup = false;
            for (uint32_t j = 0; j < ns; ++j) dup |= seen[j] == e;
            if (dup) continue;
            seen[ns++] = e;
            HIPCHECK(h, hipStreamWaitEvent(t, e, 0));
        }
    }
    for (uint32_t i = 0; i < h->n_pend; ++i) {
        const bftsim::RowSet& r = h->sets[h->pend[i].set];
        cs.sfx[i] = r.sfx; cs.ch[i] = r.ch; cs.hash[i] = r.hash;
        cs.rec[i] = r.rec; cs.byz[i] = r.byz; cs.bad[i] = r.bad; cs.pred[i] = r.pred; cs.first[i] = h->pend[i].first;
    }
    bftsim::LaunchEv& last = h->ring[h->pend[h->n_pend - 1].ev];
    bft::Params p = h->batch_p;
    HIPCHECK(h, hipEventRecord(last.h0, t));
    if (spec) {
        // a converted final batch on lane pairs (its chains are the burst's tail: latency)
        const uint32_t kind = conv ? bft::CHAIN_KERNEL_PAIR : chain_kind(h, p.n_instances, true);
        p.chain_prio = kind == bft::CHAIN_KERNEL_LANE ? bftsim::PRIO_SPEC_LANE : bftsim::PRIO_SPEC_PAIR;
        // the predicted blocks' suffix rows and chains, which need nothing of the consensus kernels (one suffix
        // pass for the whole batch: per launch on a stream of their own they fell behind the launches); once
        // every launch's consensus kernel is done, the check of its recorded blocks against the predictions, and
        // the chains again from the first height that differs
        // (inline lane chains predict, mask and encode each block themselves: no suffix pass)
        if (!(kind == bft::CHAIN_KERNEL_LANE && h->chain_inline)) {
            HIPCHECK(h, bft::launch_spec_suffix(p.n_instances, cs, t, p));
            HIPCHECK(h, pmc_evict(h, t));
        }
        p.chain_mode = bft::CHAIN_PREDICTED;
        HIPCHECK(h, bft::launch_hash_chain_batch(p.n_instances, cs, kind, t, p));
        HIPCHECK(h, pmc_evict(h, t));
        for (uint32_t k = 0; k < bftsim::MAX_CS; ++k)   // every launch's consensus kernels (per launch stream)
            if (last_on[k] >= 0) HIPCHECK(h, hipStreamWaitEvent(t, h->ring[h->pend[last_on[k]].ev].c1, 0));
        HIPCHECK(h, bft::launch_spec_verify(p.n_instances, cs, t, p));
        HIPCHECK(h, pmc_evict(h, t));
        p.chain_mode = bft::CHAIN_REPAIR;
        HIPCHECK(h, bft::launch_hash_chain_batch(p.n_instances, cs, kind, t, p));
    } else {
        p.chain_mode = bft::CHAIN_RECORDED;
        HIPCHECK(h, bft::launch_hash_chain_batch(p.n_instances, cs, chain_kind(h, p.n_instances, false), t, p));
    }
    HIPCHECK(h, pmc_evict(h, t));
    HIPCHECK(h, hipEventRecord(last.h1, t));
    last.has_hash = true;
    hipEvent_t& bd = h->batch_ev[h->batch_ev_head++ % bftsim::BATCH_EVS];
    if (!bd) HIPCHECK(h, hipEventCreateWithFlags(&bd, hipEventDisableTiming));
    HIPCHECK(h, hipEventRecord(bd, t));
    for (uint32_t i = 0; i < h->n_pend; ++i) {
        bftsim::RowSet& r = h->sets[h->pend[i].set];
        r.batch_done = bd;
        r.busy = true;
    }
    h->n_pend = 0;
    return BFTSIM_OK;
}

int bftsim_set_hash_batch(bftsim_t* h, uint32_t launches) {
    if (!h) return BFTSIM_EINVAL;
    if (launches < 1 || launches > bftsim::MAX_BATCH) return fail(h, BFTSIM_EINVAL, "hash batch must be 1..32 launches");
    if (int rc = flush_batch(h)) return rc;
    h->hash_batch = launches;
    return BFTSIM_OK;
}

int bftsim_set_pipeline(bftsim_t* h, int on) {
    if (!h) return BFTSIM_EINVAL;
    if (on < 0 || on > (int)bftsim::MAX_SETS) return fail(h, BFTSIM_EINVAL, "pipeline depth must be 0..32");
    const int depth = on == 0 ? 0 : on == 1 ? 2 : on;
    if (depth == h->pipeline) return BFTSIM_OK;
    int rc = h->last_stream ? sync_all(h) : BFTSIM_OK;
    if (rc) return rc;
    h->pipeline = depth;
    (void)hipSetDevice(h->device);
    free_bufs(h);                                   // re-sized (one or two sets) by the next prepare
    return BFTSIM_OK;
}

int bftsim_kernel_ms_sum(bftsim_t* h, double* consensus_ms, double* hash_ms, uint32_t* launches) {
    if (!h) return BFTSIM_EINVAL;
    if (int rc = flush_batch(h)) return rc;           // a pending batch's chain time goes to its last launch
    for (uint32_t i = 0; i < bftsim::RING; ++i) {
        bftsim::LaunchEv& ev = h->ring[i];
        if (ev.pending) if (int rc = fold_ev(h, ev)) return rc;
    }
    if (consensus_ms) *consensus_ms = h->acc_c;
    if (hash_ms) *hash_ms = h->acc_h;
    if (launches) *launches = h->acc_n;
    h->acc_c = h->acc_h = 0;
    h->acc_n = 0;
    return BFTSIM_OK;
}

int bftsim_sync(bftsim_t* h) {
    if (!h) return BFTSIM_EINVAL;
    if (!h->last_stream) return BFTSIM_OK;
    return sync_all(h);
}

int bftsim_last_kernel_ms(bftsim_t* h, float* cms, float* hms) {
    if (!h || h->ring_head == 0) return BFTSIM_EINVAL;
    if (int rc = flush_batch(h)) return rc;           // the last launch's chains may still be pending
    bftsim::LaunchEv& ev = h->ring[(h->ring_head - 1) % bftsim::RING];
    HIPCHECK(h, hipEventSynchronize(ev.has_hash ? ev.h1 : ev.c1));
    float a = 0, b = 0;
    HIPCHECK(h, hipEventElapsedTime(&a, ev.c0, ev.c1));
    if (ev.has_hash) HIPCHECK(h, hipEventElapsedTime(&b, ev.h0, ev.h1));
    if (cms) *cms = a;
    if (hms) *hms = b;
    return BFTSIM_OK;
}

// the fetch family writes one row per launched instance into caller buffers: refuse a short buffer
// before anything is written (include/bftsim.h bftsim_launched_count)
static int check_launched(bftsim* h, uint64_t capacity, const char* what) {
    if (h->last_n == 0) return fail(h, BFTSIM_EINVAL, std::string(what) + ": nothing launched");
    if (capacity < h->last_n)
        return fail(h, BFTSIM_EINVAL, std::string(what) + ": buffers hold " + std::to_string(capacity) +
                                          " instances, the last launch has " + std::to_string(h->last_n));
    return BFTSIM_OK;
}

int bftsim_launched_count(bftsim_t* h, uint64_t* first, uint64_t* n) {
    if (!h) return BFTSIM_EINVAL;
    if (first) *first = h->last_n ? h->last_first : 0;
    if (n) *n = h->last_n;
    return BFTSIM_OK;
}

int bftsim_fetch(bftsim_t* h, bftsim_result* out) {
    if (!h || !out) return BFTSIM_EINVAL;
    if (h->window) return fail(h, BFTSIM_EINVAL, "windowed run: per-height rows are not kept (bftsim_fetch_summary)");
    if (int rc = check_launched(h, out->capacity, "bftsim_fetch")) return rc;
    if (int rc = sync_all(h)) return rc;
    const bftsim::RowSet& r = h->sets[h->last_set];
    uint64_t n = h->last_n;
    uint32_t H = h->cfg.heights, hc = h->hcap;
    std::vector<uint32_t> ch32(n);
    HIPCHECK(h, hipMemcpy(ch32.data(), r.ch, n * 4, hipMemcpyDeviceToHost));
    for (uint64_t i = 0; i < n; ++i) out->committed_height[i] = ch32[i];
    HIPCHECK(h, hipMemcpy(out->flags, r.flags, n * 4, hipMemcpyDeviceToHost));
    HIPCHECK(h, hipMemcpy(out->ticks, r.ticks, n * 4, hipMemcpyDeviceToHost));
    HIPCHECK(h, hipMemcpy(out->views, r.views, n * 8, hipMemcpyDeviceToHost));
    std::vector<uint32_t> rec(n * hc * 4);
    std::vector<uint8_t> hs(n * hc * 32);
    HIPCHECK(h, hipMemcpy(rec.data(), r.rec, rec.size() * 4, hipMemcpyDeviceToHost));
    HIPCHECK(h, hipMemcpy(hs.data(), r.hash, hs.size(), hipMemcpyDeviceToHost));
    for (uint64_t i = 0; i < n; ++i) {
        uint32_t ch = out->committed_height[i];
        for (uint32_t x = 1; x <= H; ++x) {
            uint64_t o = i * H + (x - 1);
            const uint32_t* row = &rec[(i * hc + x) * 4];
            bool ok = x <= ch;
            out->round[o] = ok ? (uint16_t)row[0] : 0;
            out->proposer[o] = ok ? (uint16_t)(row[1] & 0xffffu) : 0;
            out->variant[o] = ok ? (uint8_t)((row[1] >> 16) & 1u) : 0;
            out->time_tick[o] = ok ? row[2] : 0;
            if (ok) memcpy(out->block_hash + o * 32, &hs[(i * hc + x) * 32], 32);
            else memset(out->block_hash + o * 32, 0, 32);
        }
    }
    if (h->h_trace && h->d_trace) {
        size_t tb = n * (size_t)h->trace_ticks * h->cfg.n * 8;
        HIPCHECK(h, hipMemcpy(h->h_trace, h->d_trace, tb, hipMemcpyDeviceToHost));
    }
    return BFTSIM_OK;
}

int bftsim_export_headers(bftsim_t* h, uint64_t capacity, uint8_t* hdr, uint32_t* hdr_len) {
    if (!h || !hdr || !hdr_len) return BFTSIM_EINVAL;
    if (h->window) return fail(h, BFTSIM_EINVAL, "windowed run: per-height rows are not kept");
    if (int rc = check_launched(h, capacity, "bftsim_export_headers")) return rc;
    if (int rc = sync_all(h)) return rc;
    const uint64_t n = h->last_n, H = h->cfg.heights, cnt = n * H;
    bft::Params p = make_params(h, h->sets[h->last_set], h->last_first, n);
    DevMem d_out, d_len;
    HIPCHECK(h, d_out.alloc(cnt * BFTSIM_HEADER_SLOT));
    HIPCHECK(h, d_len.alloc(cnt * 4));
    hipLaunchKernelGGL(bft::bft_export_kernel, dim3((uint32_t)((cnt + 255) / 256)), dim3(256), 0, h->last_stream, p,
                       d_out.as<uint8_t>(), d_len.as<uint32_t>());
    HIPCHECK(h, hipGetLastError());
    HIPCHECK(h, hipStreamSynchronize(h->last_stream));
    HIPCHECK(h, hipMemcpy(hdr, d_out.p, cnt * BFTSIM_HEADER_SLOT, hipMemcpyDeviceToHost));
    HIPCHECK(h, hipMemcpy(hdr_len, d_len.p, cnt * 4, hipMemcpyDeviceToHost));
    return BFTSIM_OK;
}

int bftsim_run(bftsim_t* h, uint64_t first, uint64_t n, bftsim_result* out) {
    if (!h || !out) return BFTSIM_EINVAL;
    if (out->capacity < n)
        return fail(h, BFTSIM_EINVAL, "bftsim_run: result buffers hold " + std::to_string(out->capacity) +
                                          " instances, " + std::to_string(n) + " requested");
    for (;;) {
        int rc = bftsim_prepare(h, n);
        if (rc) return rc;
        if ((rc = bftsim_launch(h, first, nullptr))) return rc;
        if ((rc = bftsim_fetch(h, out))) return rc;
        // the RoundChangeSet is unbounded in the reference (round_change_set.rs:11-35): an overflowing
        // batch is run again at twice the capacity
        bool over = false;
        for (uint64_t i = 0; i < n && !over; ++i) over = (out->flags[i] & BFTSIM_FLAG_RCS_OVERFLOW) != 0;
        if (!over || h->rcs_k >= bft::RCS_MAX_K) return BFTSIM_OK;
        const uint32_t k = 2u * h->rcs_k < bft::RCS_MAX_K ? 2u * h->rcs_k : bft::RCS_MAX_K;
        // the larger tables must fit beside everything else, or the flagged results stand (bftsim.h)
        const uint64_t grow = launch_blocks(h, n) * (bft::rcs_words(h->seg, k) - bft::rcs_words(h->seg, h->rcs_k)) * 4;
        size_t free_b = 0, total_b = 0;
        HIPCHECK(h, hipMemGetInfo(&free_b, &total_b));
        if (grow > free_b / 10 * 9) return BFTSIM_OK;
        if ((rc = bftsim_set_rcs_capacity(h, k))) return rc;
    }
}

int bftsim_fetch_summary(bftsim_t* h, uint64_t capacity, uint64_t* committed_height, uint32_t* flags, uint32_t* ticks,
                         uint64_t* views, uint8_t* tip_hash) {
    if (!h) return BFTSIM_EINVAL;
    if (int rc = check_launched(h, capacity, "bftsim_fetch_summary")) return rc;
    if (int rc = sync_all(h)) return rc;                // the hash pass may run on its own stream
    const bftsim::RowSet& r = h->sets[h->last_set];
    uint64_t n = h->last_n;
    if (tip_hash) {
        bft::Params p = make_params(h, r, h->last_first, n);
        hipLaunchKernelGGL(bft::bft_tip_kernel, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, h->last_stream, p,
                           h->d_tips);
        HIPCHECK(h, hipGetLastError());
    }
    HIPCHECK(h, hipStreamSynchronize(h->last_stream));
    if (committed_height) {
        std::vector<uint32_t> ch32(n);
        HIPCHECK(h, hipMemcpy(ch32.data(), r.ch, n * 4, hipMemcpyDeviceToHost));
        for (uint64_t i = 0; i < n; ++i) committed_height[i] = ch32[i];
    }
    if (flags) HIPCHECK(h, hipMemcpy(flags, r.flags, n * 4, hipMemcpyDeviceToHost));
    if (ticks) HIPCHECK(h, hipMemcpy(ticks, r.ticks, n * 4, hipMemcpyDeviceToHost));
    if (views) HIPCHECK(h, hipMemcpy(views, r.views, n * 8, hipMemcpyDeviceToHost));
    if (tip_hash) HIPCHECK(h, hipMemcpy(tip_hash, h->d_tips, n * 32, hipMemcpyDeviceToHost));
    return BFTSIM_OK;
}

int bftsim_comm_available(void) {
    Rccl& r = rccl();
    return r.ok ? BFTSIM_OK : BFTSIM_EUNSUPPORTED;
}

int bftsim_comm_unique_id(uint8_t out[128]) {
    static_assert(sizeof(ncclUniqueId) == 128, "NCCL_UNIQUE_ID_BYTES");
    if (!out) return BFTSIM_EINVAL;
    Rccl& r = rccl();
    if (!r.ok) return BFTSIM_EUNSUPPORTED;
    ncclUniqueId id;
    StdoutToStderr quiet;
    if (r.get_id(&id) != ncclSuccess) return BFTSIM_EHIP;
    memcpy(out, &id, 128);
    return BFTSIM_OK;
}

int bftsim_comm_init(bftsim_t* h, int world_size, int rank, const uint8_t unique_id[128]) {
    if (!h || !unique_id || world_size < 1 || rank < 0 || rank >= world_size)
        return fail(h, BFTSIM_EINVAL, "bftsim_comm_init: bad world / rank");
    Rccl& r = rccl();
    if (!r.ok) return fail(h, BFTSIM_EUNSUPPORTED, r.why);
    HIPCHECK(h, hipSetDevice(h->device));
    if (h->comm) { comm_destroy(h->comm); h->comm = nullptr; }
    ncclUniqueId id;
    memcpy(&id, unique_id, 128);
    ncclResult_t e;
    {
        StdoutToStderr quiet;
        e = r.init_rank(&h->comm, world_size, id, rank);
    }
    if (e != ncclSuccess) { h->comm = nullptr; return fail(h, BFTSIM_EHIP, std::string("ncclCommInitRank: ") + r.err(e)); }
    if (!h->d_red) HIPCHECK(h, hipMalloc(&h->d_red, sizeof(bftsim_stats)));
    return BFTSIM_OK;
}

// bftsim_stats of the last launch of every rank, summed (every field is a count): the device image of
// the local statistics, one ncclAllReduce(sum, uint64) over xGMI on the launch stream, one copy back
int bftsim_stats_allreduce(bftsim_t* h, bftsim_stats* out) {
    if (!h || !out) return BFTSIM_EINVAL;
    if (!h->comm) return fail(h, BFTSIM_EINVAL, "bftsim_comm_init not called");
    if (h->last_n == 0) return fail(h, BFTSIM_EINVAL, "nothing launched");
    static_assert(sizeof(bftsim_stats) == (11 + bft::HIST_BINS) * 8, "bftsim_stats: a flat array of uint64 counts");
    HIPCHECK(h, hipSetDevice(h->device));
    bft::Params p = make_params(h, h->sets[h->last_set], h->last_first, h->last_n);
    hipStream_t s = h->last_stream;
    HIPCHECK(h, hipMemsetAsync(h->d_stats, 0, 16 * 8, s));
    uint32_t g = (uint32_t)((h->last_n + 255) / 256);
    hipLaunchKernelGGL(bft::bft_stats_kernel, dim3(g), dim3(256), 0, s, p, h->d_stats);
    HIPCHECK(h, hipGetLastError());
    HIPCHECK(h, hipMemcpyAsync(h->d_red, h->d_stats, 11 * 8, hipMemcpyDeviceToDevice, s));
    HIPCHECK(h, hipMemcpyAsync(h->d_red + 11, h->sets[h->last_set].hist, bft::HIST_BINS * 8, hipMemcpyDeviceToDevice,
                               s));
    Rccl& r = rccl();
    ncclResult_t e;
    {
        StdoutToStderr quiet;
        e = r.all_reduce(h->d_red, h->d_red, sizeof(bftsim_stats) / 8, ncclUint64, ncclSum, h->comm, s);
    }
    if (e != ncclSuccess) return fail(h, BFTSIM_EHIP, std::string("ncclAllReduce: ") + r.err(e));
    HIPCHECK(h, hipMemcpyAsync(out, h->d_red, sizeof(bftsim_stats), hipMemcpyDeviceToHost, s));
    HIPCHECK(h, hipStreamSynchronize(s));
    return BFTSIM_OK;
}

int bftsim_set_crypto(bftsim_t* h, const uint8_t* secrets32, const uint8_t* forged, uint32_t log_cap) {
    if (!h) return BFTSIM_EINVAL;
    const uint32_t n = h->cfg.n;
    if (h->last_stream) if (int rc = sync_all(h)) return rc;   // pending chains use the buffers freed below
    if (!secrets32) {                                  // off
        h->crypto = false;
        free_bufs(h);
        return BFTSIM_OK;
    }
    if (h->window) return fail(h, BFTSIM_EINVAL, "real-crypto mode needs the per-height rows (window 0)");
    SigApi& a = sig_api();
    if (!a.ok) return fail(h, BFTSIM_EUNSUPPORTED, a.why);
    HIPCHECK(h, hipSetDevice(h->device));
    if (!h->sig && a.create(h->device, &h->sig) != 0) return fail(h, BFTSIM_EHIP, "bftsig_create failed");
    // the forged key of validator v: keccak(secret_v), a valid key that is not a validator's
    std::vector<uint8_t> keys((size_t)2 * n * 32);
    memcpy(keys.data(), secrets32, (size_t)n * 32);
    for (uint32_t v = 0; v < n; ++v) host_keccak(secrets32 + 32u * v, 32, keys.data() + (size_t)(n + v) * 32);
    if (!h->d_keys) HIPCHECK(h, hipMalloc(&h->d_keys, (size_t)2 * 256 * 32));
    HIPCHECK(h, hipMemcpy(h->d_keys, keys.data(), keys.size(), hipMemcpyHostToDevice));
    // every secret must derive the validator address of its index (the sorted validator set)
    DevMem d_addr, d_ok;
    HIPCHECK(h, d_addr.alloc((size_t)n * 20));
    HIPCHECK(h, d_ok.alloc(n));
    if (a.secret_to_address(h->sig, h->d_keys, n, nullptr, d_addr.as<uint8_t>(), d_ok.as<uint8_t>(), nullptr) != 0)
        return fail(h, BFTSIM_EHIP, std::string("bftsig_secret_to_address: ") + a.last_error(h->sig));
    std::vector<uint8_t> addr((size_t)n * 20), ok(n);
    HIPCHECK(h, hipDeviceSynchronize());
    HIPCHECK(h, hipMemcpy(addr.data(), d_addr.p, addr.size(), hipMemcpyDeviceToHost));
    HIPCHECK(h, hipMemcpy(ok.data(), d_ok.p, n, hipMemcpyDeviceToHost));
    for (uint32_t v = 0; v < n; ++v)
        if (!ok[v] || memcmp(addr.data() + 20u * v, h->addresses.data() + 20u * v, 20) != 0)
            return fail(h, BFTSIM_EINVAL, "secret " + std::to_string(v) + " does not derive validator address " +
                                              std::to_string(v));
    for (int k = 0; k < 4; ++k) h->forged[k] = 0;
    if (forged)
        for (uint32_t v = 0; v < n; ++v)
            if (forged[v]) h->forged[v >> 6] |= 1ull << (v & 63u);
    h->mlog_cap = log_cap ? log_cap : h->cfg.heights * (4u * n + 8u) + 64u * n;
    h->crypto = true;
    free_bufs(h);                                      // the log is allocated by the next prepare
    return BFTSIM_OK;
}

}  // extern "C"

// The twins of the trace a verify is keeping (bftsim_set_trace_twins, SPEC.md §11f), on the verify's
// stream and in buffers of their own: the pass's arrays `a` are read, never written. tk: what the handle takes over
// (the merged index and the twins' digests, signatures and seals); ta: what the trace's twin kernels read.
namespace {
struct TwinKeep {
    DevMem keep;
    const uint64_t* if0 = nullptr;
    std::vector<uint64_t> if0_host;
    uint64_t T = 0, counts[2] = {0, 0};
};
}  // namespace
static int twins_build(bftsim* h, const bft::Params& p, const bft::CryptoArgs& a, uint64_t n, uint64_t M, hipStream_t s,
                       TwinKeep& tk, bft::TwinArgs& ta) {
    namespace tw = bft::twins;
    SigApi& sa = sig_api();
    if (M + 1 > 0x7fffffffull) return fail(h, BFTSIM_EINVAL, "trace twins: too many messages for one scan");
    auto up = [](uint64_t b) { return (b + 15) & ~15ull; };
    DevMem idx, tmp, work;
    Events ev;
    HIPCHECK(h, ev.create(6));
    HIPCHECK(h, idx.alloc(up(n * 32) + 2 * up((M + 1) * 4) + 16));
    tw::Args t{};
    t.mlog = a.mlog; t.cap = a.cap; t.n_val = a.n_val; t.seed = p.seed; t.first_instance = p.first_instance;
    t.byz_count = p.byz_count; t.n_inst = n; t.M = M; t.moff = a.moff; t.mref = a.mref; t.key = a.key;
    uint8_t* q = idx.as<uint8_t>();
    t.byz = (uint64_t*)q; q += up(n * 32);
    t.mark = (uint32_t*)q; q += up((M + 1) * 4);
    uint32_t* scan = (uint32_t*)q; q += up((M + 1) * 4);
    t.counts = (unsigned long long*)q;
    size_t tb = 0;
    HIPCHECK(h, hipcub::DeviceScan::ExclusiveSum(nullptr, tb, t.mark, scan, (int)(M + 1)));
    HIPCHECK(h, tmp.alloc(tb ? tb : 16));
    HIPCHECK(h, hipMemsetAsync(t.counts, 0, 8, s));
    HIPCHECK(h, hipEventRecord(ev[0], s));
    HIPCHECK(h, tw::launch_mark(t, s));
    HIPCHECK(h, hipcub::DeviceScan::ExclusiveSum(tmp.p, tb, t.mark, scan, (int)(M + 1), s));
    uint32_t T32 = 0;
    unsigned long long packed = 0;
    HIPCHECK(h, hipMemcpyAsync(&T32, scan + M, 4, hipMemcpyDeviceToHost, s));
    HIPCHECK(h, hipMemcpyAsync(&packed, t.counts, 8, hipMemcpyDeviceToHost, s));
    HIPCHECK(h, hipStreamSynchronize(s));
    const uint64_t T = T32, Tx = T ? T : 1;
    tk.counts[0] = packed & 0xffffffffull;
    tk.counts[1] = packed >> 32;
    if (tk.counts[0] + tk.counts[1] != T) return fail(h, BFTSIM_EHIP, "trace twins: the marks' counts and their scan disagree");
    // kept: tslot, if0, fmap, tmsg, traw, tmsg_k, tsigs, tseals; temporary: the twins' keys and digests
    HIPCHECK(h, tk.keep.alloc(up((M + 1) * 4) + up((n + 1) * 8) + up((M + T) * 8) + up(Tx * 8) + up(Tx * 32) + up(Tx * 4) +
                              2 * up(Tx * 65)));
    HIPCHECK(h, work.alloc(2 * up(Tx * 4) + 2 * up(Tx * 32) + up(Tx) + 16));
    q = tk.keep.as<uint8_t>();
    t.tslot = (uint32_t*)q; q += up((M + 1) * 4);
    t.if0 = (uint64_t*)q; q += up((n + 1) * 8);
    t.fmap = (uint64_t*)q; q += up((M + T) * 8);
    t.tmsg = (uint64_t*)q; q += up(Tx * 8);
    t.raw = q; q += up(Tx * 32);
    t.msg_k = (uint32_t*)q; q += up(Tx * 4);
    uint8_t* tsigs = q; q += up(Tx * 65);
    uint8_t* tseals = q;
    q = work.as<uint8_t>();
    t.tkey = (uint32_t*)q; q += up(Tx * 4);
    t.seal_key = (uint32_t*)q; q += up(Tx * 4);
    t.sign_dig = q; q += up(Tx * 32);
    t.seal_dig = q; q += up(Tx * 32);
    uint8_t* ok = q; q += up(Tx);
    t.ncm = (uint32_t*)q;
    t.seals = tseals;
    t.T = T;
    HIPCHECK(h, hipMemcpyAsync(t.tslot, scan, (M + 1) * 4, hipMemcpyDeviceToDevice, s));
    HIPCHECK(h, hipMemsetAsync(t.ncm, 0, 4, s));
    HIPCHECK(h, tw::launch_merge(t, s));
    HIPCHECK(h, hipEventRecord(ev[1], s));
    HIPCHECK(h, tw::launch_prep(p, t, s));
    HIPCHECK(h, hipEventRecord(ev[2], s));
    uint32_t ncm = 0;
    tk.if0_host.resize(n + 1);
    HIPCHECK(h, hipMemcpyAsync(&ncm, t.ncm, 4, hipMemcpyDeviceToHost, s));
    HIPCHECK(h, hipMemcpyAsync(tk.if0_host.data(), t.if0, (n + 1) * 8, hipMemcpyDeviceToHost, s));
    HIPCHECK(h, hipStreamSynchronize(s));
    if (ncm > T) return fail(h, BFTSIM_EHIP, "trace twins: more Commit twins than twins");
    // commit seals first: they are part of the Commit's sign payload
    if (ncm && sa.sign(h->sig, h->d_keys, t.seal_key, t.seal_dig, ncm, tseals, ok, s) != 0)
        return fail(h, BFTSIM_EHIP, std::string("bftsig_sign (twin seals): ") + sa.last_error(h->sig));
    HIPCHECK(h, hipEventRecord(ev[3], s));
    HIPCHECK(h, tw::launch_digest(p, t, s));
    HIPCHECK(h, hipEventRecord(ev[4], s));
    if (T && sa.sign(h->sig, h->d_keys, t.tkey, t.sign_dig, T, tsigs, ok, s) != 0)
        return fail(h, BFTSIM_EHIP, std::string("bftsig_sign (twins): ") + sa.last_error(h->sig));
    HIPCHECK(h, hipEventRecord(ev[5], s));
    HIPCHECK(h, hipStreamSynchronize(s));
    float ms[5];
    for (int k = 0; k < 5; ++k) HIPCHECK(h, hipEventElapsedTime(&ms[k], ev[k], ev[k + 1]));
    h->twin_ms[0] = ms[0];
    h->twin_ms[1] = ms[1] + ms[3];
    h->twin_ms[2] = ms[2] + ms[4];
    tk.T = T;
    tk.if0 = t.if0;
    ta.fmap = t.fmap; ta.tslot = t.tslot; ta.traw = t.raw; ta.tmsg_k = t.msg_k; ta.tsigs = tsigs; ta.tseals = tseals;
    return BFTSIM_OK;
}

extern "C" {
int bftsim_crypto_verify(bftsim_t* h, bftsim_crypto_report* out, uint64_t capacity, uint8_t* inst_checksum,
                         uint32_t* inst_messages) {
    if (!h || !out) return BFTSIM_EINVAL;
    if (!h->crypto) return fail(h, BFTSIM_EINVAL, "bftsim_set_crypto not called");
    if (h->last_n == 0 || !h->d_mlog) return fail(h, BFTSIM_EINVAL, "nothing launched");
    if (inst_checksum || inst_messages)
        if (int rc = check_launched(h, capacity, "bftsim_crypto_verify")) return rc;
    if (int rc = sync_all(h)) return rc;
    SigApi& sa = sig_api();
    const uint64_t n = h->last_n;
    hipStream_t s = h->last_stream;
    std::vector<uint32_t> cnt(n);
    HIPCHECK(h, hipMemcpy(cnt.data(), h->d_mlog_n, n * 4, hipMemcpyDeviceToHost));
    std::vector<uint64_t> off(n);
    uint64_t M = 0, over = 0;
    for (uint64_t i = 0; i < n; ++i) {
        off[i] = M;
        if (cnt[i] > h->mlog_cap) ++over;
        M += cnt[i] < h->mlog_cap ? cnt[i] : h->mlog_cap;
        if (inst_messages) inst_messages[i] = cnt[i];
    }
    memset(out, 0, sizeof *out);
    out->log_overflows = over;
    if (over) return fail(h, BFTSIM_EINVAL, "broadcast log overflow: raise log_cap (bftsim_set_crypto)");
    // device arrays of the pass (one allocation)
    const uint64_t Mx = M ? M : 1;
    const uint64_t sz_msg = 8 + 32 + 4 + 4 + 32 + 65 + 20 + 1, sz_cm = 32 + 32 + 4 + 65 + 1 + 20 + 4;
    // trace keep (bftsim_set_trace_keep): what the export reads lives in an allocation of its own that the handle
    // takes over; off: the same allocations as ever
    trace_drop(h);
    const bool keep = h->trace_keep;
    if (keep) off.push_back(M);
    DevMem pool, kpool;
    if (keep) HIPCHECK(h, kpool.alloc((n + 1) * 8 + Mx * (8 + 32 + 4 + 65 + 65) + 6 * 16));
    // with keep on the six kept arrays (182 B per message) are not in the temporary pool
    const uint64_t bytes = n * 8 + Mx * (sz_msg + sz_cm - (keep ? 8 + 32 + 4 + 65 + 65 : 0)) + n * 32 + 64 + 256;
    HIPCHECK(h, pool.alloc(bytes));
    uint8_t *q = pool.as<uint8_t>(), *kq = kpool.as<uint8_t>();
    auto take = [&](uint64_t b, bool kept = false) {
        uint8_t*& c = kept && keep ? kq : q;
        uint8_t* r = c;
        c += (b + 15) & ~15ull;
        return r;
    };
    bft::CryptoArgs a{};
    a.mlog = h->d_mlog; a.mlog_n = h->d_mlog_n; a.cap = h->mlog_cap; a.n_val = h->cfg.n;
    for (int k = 0; k < 4; ++k) a.forged[k] = h->forged[k];
    uint64_t* d_off = (uint64_t*)take(off.size() * 8, true); a.moff = d_off;
    a.mref = (uint64_t*)take(Mx * 8, true); a.raw = take(Mx * 32, true); a.key = (uint32_t*)take(Mx * 4);
    a.msg_k = (uint32_t*)take(Mx * 4, true); a.sign_dig = take(Mx * 32); a.sigs = take(Mx * 65, true);
    a.rec_addr = take(Mx * 20); a.rec_ok = take(Mx);
    a.seal_dig = take(Mx * 32); a.seal_raw = take(Mx * 32); a.seal_key = (uint32_t*)take(Mx * 4);
    a.seals = take(Mx * 65, true); a.seal_ok = take(Mx); uint8_t* seal_addr = take(Mx * 20);
    uint8_t* sig_ok = take(Mx);
    a.ncm = (uint32_t*)take(4); a.inst_ck = (uint32_t*)take(n * 32); a.counts = (unsigned long long*)take(64);
    HIPCHECK(h, hipMemcpyAsync(d_off, off.data(), off.size() * 8, hipMemcpyHostToDevice, s));
    HIPCHECK(h, hipMemsetAsync(a.ncm, 0, 4, s));
    HIPCHECK(h, hipMemsetAsync(a.inst_ck, 0, n * 32, s));
    HIPCHECK(h, hipMemsetAsync(a.counts, 0, 64, s));
    bft::Params p = make_params(h, h->sets[h->last_set], h->last_first, n);
    if (M) {
        // the votes of the last verify go first: whatever fails below, bftsim_export_ledger finds none
        (void)hipFree(h->d_vsig); (void)hipFree(h->d_vhas);
        h->d_vsig = nullptr; h->d_vhas = nullptr; h->vsig_n = 0;
        uint32_t ncm = 0;
        hipLaunchKernelGGL(bft::bft_crypto_prep_kernel, dim3((uint32_t)n), dim3(64), 0, s, p, a);
        HIPCHECK(h, hipGetLastError());
        HIPCHECK(h, hipMemcpyAsync(&ncm, a.ncm, 4, hipMemcpyDeviceToHost, s));
        HIPCHECK(h, hipStreamSynchronize(s));
        // commit seals first: they are part of the Commit's sign payload
        if (ncm && sa.sign(h->sig, h->d_keys, a.seal_key, a.seal_dig, ncm, a.seals, sig_ok, s) != 0)
            return fail(h, BFTSIM_EHIP, std::string("bftsig_sign (seals): ") + sa.last_error(h->sig));
        const uint32_t g = (uint32_t)((M + 63) / 64);
        hipLaunchKernelGGL(bft::bft_crypto_digest_kernel, dim3(g), dim3(64), 0, s, p, a, M);
        HIPCHECK(h, hipGetLastError());
        if (sa.sign(h->sig, h->d_keys, a.key, a.sign_dig, M, a.sigs, sig_ok, s) != 0)
            return fail(h, BFTSIM_EHIP, std::string("bftsig_sign: ") + sa.last_error(h->sig));
        // the receivers: recover every message's signer, and every seal (verify_commit)
        if (sa.recover(h->sig, a.sign_dig, a.sigs, M, nullptr, a.rec_addr, a.rec_ok, s) != 0)
            return fail(h, BFTSIM_EHIP, std::string("bftsig_recover: ") + sa.last_error(h->sig));
        if (ncm && sa.recover(h->sig, a.seal_raw, a.seals, ncm, nullptr, seal_addr, a.seal_ok, s) != 0)
            return fail(h, BFTSIM_EHIP, std::string("bftsig_recover (seals): ") + sa.last_error(h->sig));
        hipLaunchKernelGGL(bft::bft_crypto_check_kernel, dim3(g), dim3(64), 0, s, p, a, M);
        HIPCHECK(h, hipGetLastError());
        // the votes of every committed block, kept for bftsim_export_ledger
        const uint64_t vs = n * (uint64_t)h->cfg.heights * h->cfg.n;
        HIPCHECK(h, hipMalloc(&h->d_vsig, vs * 65));
        HIPCHECK(h, hipMalloc(&h->d_vhas, vs));
        HIPCHECK(h, hipMemsetAsync(h->d_vhas, 0, vs, s));
        hipLaunchKernelGGL(bft::bft_crypto_votes_kernel, dim3(g), dim3(64), 0, s, p, a, M, h->d_vsig, h->d_vhas,
                           h->ledger_votes == BFTSIM_VOTES_SEALS ? 1u : 0u);
        HIPCHECK(h, hipGetLastError());
        h->vsig_n = n;
    }
    bft::TwinArgs ta{};
    TwinKeep tk;
    const bool twins = keep && h->trace_twins && M;
    if (twins)
        if (int rc = twins_build(h, p, a, n, M, s, tk, ta)) return rc;
    unsigned long long c[8] = {0};
    HIPCHECK(h, hipMemcpyAsync(c, a.counts, 64, hipMemcpyDeviceToHost, s));
    if (inst_checksum) HIPCHECK(h, hipMemcpyAsync(inst_checksum, a.inst_ck, n * 32, hipMemcpyDeviceToHost, s));
    HIPCHECK(h, hipStreamSynchronize(s));
    if (keep) {
        h->d_tkeep = kpool.release<uint8_t>();
        h->trace_args = bft::TraceArgs{h->d_mlog, h->mlog_cap, a.moff, a.mref, a.raw, a.msg_k, a.sigs, a.seals};
        h->twin_args = ta;
        h->trace_n = n;
        h->trace_M = M;
        h->trace_F = M + tk.T;
        h->trace_moff = off;
        h->d_tif0 = a.moff;
        if (twins) {
            h->d_twkeep = tk.keep.release<uint8_t>();
            h->trace_has_twins = true;
            h->trace_moff.swap(tk.if0_host);
            h->d_tif0 = tk.if0;
            h->twin_counts[0] = tk.counts[0];
            h->twin_counts[1] = tk.counts[1];
        }
    }
    out->messages = c[0];
    out->seals = c[1];
    out->forged = c[2];
    out->recovered_as_sender = c[3];
    out->mismatches = c[4];
    out->seal_errors = c[5];
    out->signatures = c[0] + c[1];
    out->recoveries = c[0] + c[1];
    return BFTSIM_OK;
}

int bftsim_export_ledger(bftsim_t* h, uint64_t capacity, uint8_t* hdr, uint64_t slot_bytes, uint32_t* hdr_len) {
    if (!h || !hdr || !hdr_len) return BFTSIM_EINVAL;
    if (!h->crypto || h->vsig_n == 0 || h->vsig_n != h->last_n)
        return fail(h, BFTSIM_EINVAL, "no votes: bftsim_crypto_verify after the launch first");
    if (int rc = check_launched(h, capacity, "bftsim_export_ledger")) return rc;
    if (slot_bytes < bftsim_ledger_slot_bytes(h->cfg.n)) return fail(h, BFTSIM_EINVAL, "slot_bytes too small");
    if (int rc = sync_all(h)) return rc;
    const uint64_t n = h->last_n, H = h->cfg.heights, cnt = n * H;
    bft::Params p = make_params(h, h->sets[h->last_set], h->last_first, n);
    DevMem d_out, d_len;
    HIPCHECK(h, d_out.alloc(cnt * slot_bytes));
    HIPCHECK(h, d_len.alloc(cnt * 4));
    hipLaunchKernelGGL(bft::bft_export_votes_kernel, dim3((uint32_t)((cnt + 63) / 64)), dim3(64), 0, h->last_stream, p,
                       h->d_vsig, h->d_vhas, d_out.as<uint8_t>(), slot_bytes, d_len.as<uint32_t>());
    HIPCHECK(h, hipGetLastError());
    HIPCHECK(h, hipStreamSynchronize(h->last_stream));
    HIPCHECK(h, hipMemcpy(hdr, d_out.p, cnt * slot_bytes, hipMemcpyDeviceToHost));
    HIPCHECK(h, hipMemcpy(hdr_len, d_len.p, cnt * 4, hipMemcpyDeviceToHost));
    return BFTSIM_OK;
}

uint64_t bftsim_ledger_slot_bytes(uint32_t n) { return ((uint64_t)BFTSIM_HEADER_SLOT + 3 + (uint64_t)n * 133 + 7) & ~7ull; }

// ---- the trace (SPEC.md §11b)
int bftsim_set_trace_keep(bftsim_t* h, int on) {
    if (!h) return BFTSIM_EINVAL;
    h->trace_keep = on != 0;
    if (!on) {
        HIPCHECK(h, hipSetDevice(h->device));
        trace_drop(h);
    }
    return BFTSIM_OK;
}

}  // extern "C"

// the kept trace's passes, which the analysers' *_last_trace entry points run too (declared in bftsim_impl.h)
int trace_ready(bftsim* h, const char* what) {
    if (!h->crypto) return fail(h, BFTSIM_EINVAL, std::string(what) + ": bftsim_set_crypto not called");
    if (!h->trace_keep) return fail(h, BFTSIM_EINVAL, std::string(what) + ": bftsim_set_trace_keep is off");
    if (h->trace_n == 0 || h->trace_n != h->last_n)
        return fail(h, BFTSIM_EINVAL, std::string(what) + ": no trace kept: bftsim_crypto_verify after the launch first");
    return BFTSIM_OK;
}

// size pass + scan over every kept message, once per verify: d_tfoff and the host's per-instance offsets
int trace_size_pass(bftsim* h) {
    if (h->d_tfoff) return BFTSIM_OK;
    const uint64_t n = h->trace_n, M = h->trace_F;               // every frame: the messages and their twins
    if (M + 1 > 0x7fffffffull) return fail(h, BFTSIM_EINVAL, "trace: too many messages for one scan");
    HIPCHECK(h, hipSetDevice(h->device));
    hipStream_t s = h->last_stream;
    DevMem foff, len_buf, tmp;
    Events ev;
    size_t tb = 0;
    HIPCHECK(h, foff.alloc((M + 1 + n + 1) * 8 + 16));
    HIPCHECK(h, len_buf.alloc((M + 1) * 8));
    uint64_t *d = foff.as<uint64_t>(), *lens = len_buf.as<uint64_t>();
    HIPCHECK(h, hipcub::DeviceScan::ExclusiveSum(nullptr, tb, lens, d, (int)(M + 1)));
    HIPCHECK(h, tmp.alloc(tb ? tb : 16));
    HIPCHECK(h, ev.create(2));
    std::vector<uint64_t> ioff(n + 1);
    bft::Params p = make_params(h, h->sets[h->last_set], h->last_first, n);
    HIPCHECK(h, hipEventRecord(ev[0], s));
    if (h->trace_has_twins)
        hipLaunchKernelGGL(bft::bft_trace_size_kernel<true>, dim3((uint32_t)((M + 1 + 63) / 64)), dim3(64), 0, s, p,
                           h->trace_args, M, lens, bft::TwinOpt<true>{h->twin_args});
    else
        hipLaunchKernelGGL(bft::bft_trace_size_kernel<false>, dim3((uint32_t)((M + 1 + 63) / 64)), dim3(64), 0, s, p,
                           h->trace_args, M, lens, bft::TwinOpt<false>{});
    HIPCHECK(h, hipGetLastError());
    HIPCHECK(h, hipcub::DeviceScan::ExclusiveSum(tmp.p, tb, lens, d, (int)(M + 1), s));
    hipLaunchKernelGGL(bft::bft_trace_inst_kernel, dim3((uint32_t)((n + 1 + 255) / 256)), dim3(256), 0, s,
                       h->d_tif0, d, n + 1, d + M + 1);
    HIPCHECK(h, hipGetLastError());
    HIPCHECK(h, hipEventRecord(ev[1], s));
    HIPCHECK(h, hipMemcpyAsync(ioff.data(), d + M + 1, (n + 1) * 8, hipMemcpyDeviceToHost, s));
    HIPCHECK(h, hipStreamSynchronize(s));
    HIPCHECK(h, hipEventElapsedTime(&h->trace_ms[0], ev[0], ev[1]));
    h->d_tfoff = foff.release<uint64_t>();
    h->trace_ioff.swap(ioff);
    return BFTSIM_OK;
}

// emit pass: frames [m0, m1) of the kept trace (messages, and their twins where it has them) into d_out, complete when it returns. The two passes must agree on
// every frame's length; `what` names the caller in the error. t0 / t1 (or null): recorded around the kernel alone.
int trace_emit(bftsim* h, const char* what, uint64_t m0, uint64_t m1, uint8_t* d_out, hipEvent_t t0,
                      hipEvent_t t1) {
    hipStream_t s = h->last_stream;
    uint32_t* d_err = (uint32_t*)(h->d_tfoff + h->trace_F + 1 + h->trace_n + 1);
    uint32_t err = 0;
    HIPCHECK(h, hipMemsetAsync(d_err, 0, 4, s));
    if (t0) HIPCHECK(h, hipEventRecord(t0, s));
    if (m1 > m0) {
        bft::Params p = make_params(h, h->sets[h->last_set], h->last_first, h->trace_n);
        if (h->trace_has_twins)
            hipLaunchKernelGGL(bft::bft_trace_emit_kernel<true>, dim3((uint32_t)((m1 - m0 + 63) / 64)), dim3(64), 0, s, p,
                               h->trace_args, m0, m1, h->d_tfoff, d_out, d_err, bft::TwinOpt<true>{h->twin_args});
        else
            hipLaunchKernelGGL(bft::bft_trace_emit_kernel<false>, dim3((uint32_t)((m1 - m0 + 63) / 64)), dim3(64), 0, s, p,
                               h->trace_args, m0, m1, h->d_tfoff, d_out, d_err, bft::TwinOpt<false>{});
        HIPCHECK(h, hipGetLastError());
    }
    if (t1) HIPCHECK(h, hipEventRecord(t1, s));
    HIPCHECK(h, hipMemcpyAsync(&err, d_err, 4, hipMemcpyDeviceToHost, s));
    HIPCHECK(h, hipStreamSynchronize(s));
    if (err)
        return fail(h, BFTSIM_EHIP, std::string(what) + ": " + std::to_string(err) +
                                        " frames whose emitted length differs from the counted one");
    return BFTSIM_OK;
}

extern "C" {

int bftsim_trace_sizes(bftsim_t* h, uint64_t capacity, uint32_t* inst_frames, uint64_t* inst_bytes) {
    if (!h) return BFTSIM_EINVAL;
    if (int rc = trace_ready(h, "bftsim_trace_sizes")) return rc;
    if (int rc = check_launched(h, capacity, "bftsim_trace_sizes")) return rc;
    if (int rc = trace_size_pass(h)) return rc;
    for (uint64_t i = 0; i < h->trace_n; ++i) {
        if (inst_frames) inst_frames[i] = (uint32_t)(h->trace_moff[i + 1] - h->trace_moff[i]);
        if (inst_bytes) inst_bytes[i] = h->trace_ioff[i + 1] - h->trace_ioff[i];
    }
    return BFTSIM_OK;
}

int bftsim_export_trace(bftsim_t* h, uint64_t inst_begin, uint64_t inst_count, uint8_t* stream, uint64_t stream_cap,
                        uint64_t* frame_off, uint64_t frame_cap, uint32_t* frame_meta, uint64_t* inst_frame0) {
    if (!h) return BFTSIM_EINVAL;
    if (!frame_off) return fail(h, BFTSIM_EINVAL, "bftsim_export_trace: null frame_off");
    if (int rc = trace_ready(h, "bftsim_export_trace")) return rc;
    const uint64_t n = h->trace_n;
    if (inst_begin > n || inst_count > n - inst_begin)
        return fail(h, BFTSIM_EINVAL, "bftsim_export_trace: instances [" + std::to_string(inst_begin) + ", +" +
                                          std::to_string(inst_count) + ") outside the last launch of " + std::to_string(n));
    if (int rc = trace_size_pass(h)) return rc;
    const uint64_t m0 = h->trace_moff[inst_begin], m1 = h->trace_moff[inst_begin + inst_count];
    const uint64_t frames = m1 - m0, bytes = h->trace_ioff[inst_begin + inst_count] - h->trace_ioff[inst_begin];
    if (frame_cap < frames)
        return fail(h, BFTSIM_EINVAL, "bftsim_export_trace: frame_cap " + std::to_string(frame_cap) + " < " +
                                          std::to_string(frames) + " frames");
    if (stream_cap < bytes || (bytes && !stream))
        return fail(h, BFTSIM_EINVAL, "bftsim_export_trace: stream_cap " + std::to_string(stream_cap) + " < " +
                                          std::to_string(bytes) + " bytes");
    HIPCHECK(h, hipSetDevice(h->device));
    hipStream_t s = h->last_stream;
    DevMem d_out, d_meta;
    Events ev;
    HIPCHECK(h, d_out.alloc(bytes + 16));
    if (frame_meta && frames) HIPCHECK(h, d_meta.alloc(frames * 16));
    HIPCHECK(h, ev.create(4));
    if (d_meta.p) {
        if (h->trace_has_twins)
            hipLaunchKernelGGL(bft::bft_trace_meta_kernel<true>, dim3((uint32_t)((frames + 255) / 256)), dim3(256), 0, s,
                               h->trace_args, m0, m1, (uint32_t)inst_begin, d_meta.as<uint32_t>(),
                               bft::TwinOpt<true>{h->twin_args});
        else
            hipLaunchKernelGGL(bft::bft_trace_meta_kernel<false>, dim3((uint32_t)((frames + 255) / 256)), dim3(256), 0, s,
                               h->trace_args, m0, m1, (uint32_t)inst_begin, d_meta.as<uint32_t>(), bft::TwinOpt<false>{});
        HIPCHECK(h, hipGetLastError());
    }
    if (int rc = trace_emit(h, "bftsim_export_trace", m0, m1, d_out.as<uint8_t>(), ev[0], ev[1])) return rc;
    // the passes agreed on every frame: only now is anything written to the caller's buffers
    HIPCHECK(h, hipEventRecord(ev[2], s));
    if (bytes) HIPCHECK(h, hipMemcpyAsync(stream, d_out.p, bytes, hipMemcpyDeviceToHost, s));
    HIPCHECK(h, hipMemcpyAsync(frame_off, h->d_tfoff + m0, (frames + 1) * 8, hipMemcpyDeviceToHost, s));
    if (d_meta.p) HIPCHECK(h, hipMemcpyAsync(frame_meta, d_meta.p, frames * 16, hipMemcpyDeviceToHost, s));
    HIPCHECK(h, hipEventRecord(ev[3], s));
    HIPCHECK(h, hipStreamSynchronize(s));
    HIPCHECK(h, hipEventElapsedTime(&h->trace_ms[1], ev[0], ev[1]));
    HIPCHECK(h, hipEventElapsedTime(&h->trace_ms[2], ev[2], ev[3]));
    const uint64_t base = frame_off[0];
    for (uint64_t k = 0; k <= frames; ++k) frame_off[k] -= base;
    if (inst_frame0)
        for (uint64_t i = 0; i <= inst_count; ++i) inst_frame0[i] = h->trace_moff[inst_begin + i] - m0;
    return BFTSIM_OK;
}

int bftsim_trace_last_ms(bftsim_t* h, float* size_ms, float* emit_ms, float* copy_ms) {
    return h ? last_ms(h->trace_ms, {size_ms, emit_ms, copy_ms}) : BFTSIM_EINVAL;
}

// ---- twins (SPEC.md §11f)
int bftsim_set_trace_twins(bftsim_t* h, int on) {
    if (!h) return BFTSIM_EINVAL;
    if (on != 0 && on != 1) return fail(h, BFTSIM_EINVAL, "bftsim_set_trace_twins: 0 or 1");
    h->trace_twins = on == 1;                      // read by the next keeping bftsim_crypto_verify
    return BFTSIM_OK;
}

int bftsim_trace_twin_counts(bftsim_t* h, uint64_t* pp_twins, uint64_t* vote_twins) {
    if (!h) return BFTSIM_EINVAL;
    if (int rc = trace_ready(h, "bftsim_trace_twin_counts")) return rc;
    if (pp_twins) *pp_twins = h->twin_counts[0];
    if (vote_twins) *vote_twins = h->twin_counts[1];
    return BFTSIM_OK;
}

int bftsim_trace_twins_last_ms(bftsim_t* h, float* index_ms, float* digest_ms, float* sign_ms) {
    return h ? last_ms(h->twin_ms, {index_ms, digest_ms, sign_ms}) : BFTSIM_EINVAL;
}

int bftsim_stats_get(bftsim_t* h, bftsim_stats* out) {
    if (!h || !out) return BFTSIM_EINVAL;
    if (h->last_n == 0) return fail(h, BFTSIM_EINVAL, "nothing launched");
    HIPCHECK(h, hipSetDevice(h->device));
    bft::Params p = make_params(h, h->sets[h->last_set], h->last_first, h->last_n);
    HIPCHECK(h, hipMemsetAsync(h->d_stats, 0, 16 * 8, h->last_stream));
    uint32_t g = (uint32_t)((h->last_n + 255) / 256);
    hipLaunchKernelGGL(bft::bft_stats_kernel, dim3(g), dim3(256), 0, h->last_stream, p, h->d_stats);
    HIPCHECK(h, hipGetLastError());
    unsigned long long st[16];
    uint64_t hist[bft::HIST_BINS];
    HIPCHECK(h, hipMemcpyAsync(st, h->d_stats, sizeof st, hipMemcpyDeviceToHost, h->last_stream));
    HIPCHECK(h, hipMemcpyAsync(hist, h->sets[h->last_set].hist, sizeof hist, hipMemcpyDeviceToHost, h->last_stream));
    HIPCHECK(h, hipStreamSynchronize(h->last_stream));
    out->instances = st[0];
    out->committed_heights = st[1];
    out->views = st[2];
    out->ticks = st[3];
    for (int i = 0; i < 7; ++i) out->flagged[i] = st[4 + i];
    for (int i = 0; i < 65; ++i) out->round_hist[i] = hist[i];
    for (int i = 0; i < 65; ++i) out->latency_hist[i] = hist[65 + i];
    return BFTSIM_OK;
}

}  // extern "C"
