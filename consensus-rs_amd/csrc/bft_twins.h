// bft_twins.h — trace twins (SPEC.md §11f): the second frame of every equivocating broadcast. A Byzantine validator
// sends variant 0 of its block to some receivers and variant 1 to the others, and its votes count for both; the
// broadcast log, and so the trace, holds one entry for each. With twins on the kept trace carries the message for the
// other variant immediately behind its original. The steps, shared by the host and the GPU:
//   byz_mask     the Byzantine validators of an instance, drawn as the kernels draw them (SPEC.md §5)
//   needs_twin   the mark of one log entry: none, a PrePrepare's twin, a vote's twin
//   merge_put    after the exclusive scan of the marks: the merged frame index, frame -> (message, is-twin), and the
//                message of every twin slot
//   frame0       the first frame of an instance
// and, for the digests of a twin (device and host alike), the block digest of a logged block id as the run left it.
#pragma once
#include "bft_common.h"

namespace bft {

// parent hash of the block at height x as the run left it: the canonical row x-1 (genesis at 1); a
// height above the committed chain + 1 has no known parent and uses 0^32 (SPEC.md §11)
BFT_FN void crypto_parent(const Params& p, uint32_t il, uint32_t x, uint32_t prev[8]) {
    const uint32_t ch = p.committed_height[il];
    if (x <= 1) {
        for (int i = 0; i < 8; ++i)
            prev[i] = (uint32_t)p.genesis_hash[4 * i] | ((uint32_t)p.genesis_hash[4 * i + 1] << 8) |
                      ((uint32_t)p.genesis_hash[4 * i + 2] << 16) | ((uint32_t)p.genesis_hash[4 * i + 3] << 24);
    } else if (x - 1 <= ch) {
        const uint32_t* ph = (const uint32_t*)(p.hash + ((uint64_t)il * p.rows + (x - 1)) * 32);
        for (int i = 0; i < 8; ++i) prev[i] = ph[i];
    } else {
        for (int i = 0; i < 8; ++i) prev[i] = 0;
    }
}
// Subject digest of a logged block id: the canonical row's hash when the block is the committed one
// at its height, else the hash of its header over crypto_parent
BFT_FN void crypto_block_digest(const Params& p, uint32_t il, uint64_t b, uint8_t* hbuf, uint8_t out[32]) {
    const uint32_t x = blk_h(b), prop = blk_prop(b), var = blk_var(b);
    if (!blk_valid(b) || x == 0) { for (int i = 0; i < 32; ++i) out[i] = 0; return; }
    if (x <= p.committed_height[il]) {
        const uint32_t* row = p.rec + ((uint64_t)il * p.rows + x) * 4;
        if ((row[1] & 0xffffu) == prop && ((row[1] >> 16) & 1u) == var) {
            const uint8_t* hs = p.hash + ((uint64_t)il * p.rows + x) * 32;
            for (int i = 0; i < 32; ++i) out[i] = hs[i];
            return;
        }
    }
    uint32_t prev[8], w[8];
    crypto_parent(p, il, x, prev);
    const uint64_t time = p.genesis_time + (uint64_t)p.block_period * ((uint64_t)blk_T(b) + 1ull);
    lane_block_hash(hbuf, prev, p.addresses + 20u * prop, p.seed, p.first_instance + il, x, prop, var, time, w);
    for (int i = 0; i < 32; ++i) out[i] = (uint8_t)(w[i >> 2] >> (8 * (i & 3)));
}

namespace twins {

constexpr uint32_t META_TWIN = 1u << 16;      // frame_meta word 2 of a twin: its original's flags with this bit
constexpr uint64_t BLK_FLIP = 1ull << 33;     // the other variant of a block id
constexpr uint64_t F_TWIN = 1ull << 63;       // merged index entry: message | F_TWIN for a twin
constexpr uint32_t MARK_NONE = 0, MARK_PP = 1, MARK_VOTE = 2;

// The Byzantine validators of instance `inst` among n (SPEC.md §5: partial Fisher-Yates, as Wave::init_byzantine);
// perm: n bytes of scratch, byte i at perm[i * stride]
BFT_FN void byz_mask(uint64_t seed, uint32_t inst, uint32_t n, uint32_t f, uint8_t* perm, uint32_t stride, uint64_t out[4]) {
    for (uint32_t i = 0; i < n; ++i) perm[i * stride] = (uint8_t)i;
    for (int k = 0; k < 4; ++k) out[k] = 0;
    if (f > n) f = n;
    for (uint32_t i = 0; i < f; ++i) {
        uint32_t w[4];
        philox(seed, inst, i, 0, DOM_BYZ, w);
        const uint32_t j = i + w[0] % (n - i);
        const uint8_t t = perm[i * stride]; perm[i * stride] = perm[j * stride]; perm[j * stride] = t;
        const uint32_t v = perm[i * stride];
        out[(v >> 6) & 3u] |= 1ull << (v & 63u);
    }
}

// The mark of log entry e (MLOG_WORDS words): an equivocating PrePrepare; or a wildcard Prepare / Commit (an
// old-block Commit too) of a valid block above height 0 whose proposer is Byzantine: only such a block has a second
// variant
BFT_FN uint32_t needs_twin(const uint32_t* e, const uint64_t byz[4]) {
    const uint32_t code = (e[1] >> 8) & 0xffu, fl = e[6];
    if (code == (uint32_t)MT_PREPREPARE) return (fl & MLOG_EQUIV) ? MARK_PP : MARK_NONE;
    if ((code != (uint32_t)MT_PREPARE && code != (uint32_t)MT_COMMIT) || !(fl & MLOG_WILD)) return MARK_NONE;
    const uint64_t b = (uint64_t)e[4] | ((uint64_t)e[5] << 32);
    if (!blk_valid(b) || blk_h(b) == 0) return MARK_NONE;
    const uint32_t prop = blk_prop(b);
    return prop < 256u && ((byz[prop >> 6] >> (prop & 63u)) & 1ull) ? MARK_VOTE : MARK_NONE;
}

// Message m with `before` twins ahead of it (the exclusive scan of the 0 / 1 marks): its frame, and its twin's
// behind it. fmap: [messages + twins], tmsg: [twins]; every entry is written exactly once over all m
BFT_FN void merge_put(uint64_t m, uint32_t before, bool marked, uint64_t* fmap, uint64_t* tmsg) {
    fmap[m + before] = m;
    if (marked) {
        fmap[m + before + 1] = m | F_TWIN;
        tmsg[before] = m;
    }
}
// first frame of the instance whose first message is m0 (m0 = messages for the end)
BFT_FN uint64_t frame0(uint64_t m0, const uint32_t* tslot) { return m0 + tslot[m0]; }

#if defined(__HIPCC__)
struct Args {
    const uint32_t* mlog;
    uint32_t cap, n_val;
    uint64_t seed;
    uint32_t first_instance, byz_count;
    uint64_t n_inst, M, T;
    const uint64_t* moff;             // [n_inst + 1]
    const uint64_t* mref;             // [M]
    const uint32_t* key;              // [M] the originals' signing keys
    uint64_t* byz;                    // [n_inst][4]
    uint32_t* mark;                   // [M + 1] 0 / 1 (mark[M] = 0: the scan's last entry is the total)
    uint32_t* tslot;                  // [M + 1] twins before message m
    unsigned long long* counts;       // PrePrepare twins | vote twins << 32
    uint64_t* fmap;                   // [M + T]
    uint64_t* tmsg;                   // [T]
    uint64_t* if0;                    // [n_inst + 1] first frame of each instance
    // per twin
    uint8_t* raw;                     // Subject digest
    uint32_t* tkey;
    uint32_t* msg_k;                  // a Commit twin's seal index
    uint8_t* sign_dig;
    // per Commit twin
    uint32_t* ncm;
    uint32_t* seal_key;
    uint8_t* seal_dig;
    const uint8_t* seals;
};
hipError_t launch_mark(const Args& a, hipStream_t s);
hipError_t launch_merge(const Args& a, hipStream_t s);
hipError_t launch_prep(const Params& p, const Args& a, hipStream_t s);
hipError_t launch_digest(const Params& p, const Args& a, hipStream_t s);
#endif

}  // namespace twins
}  // namespace bft
