// bft_audit.h — the observer of a trace (SPEC.md §11c): what a node following the wire does with every frame, and
// the vote tally over the accepted ones. Shared by the host build (tests/emu/audit_host.cpp) and the GPU kernels
// (kern_audit.hip). Composed from the decoders of bft_wire.h / bft_wire_block.h and the emitters of bft_crypto.h /
// bft_wire_block.h: a frame is decoded, its unsigned payload rebuilt from the decoded fields and hashed, and one
// fixed-size record written per frame:
//   Subject frames (Prepare, Commit, RoundChange): wire::decode_frame, crypto::sign_digest, crypto::seal_digest
//   Preprepare frames: wire::decode_pp_frame, wire::emit_pp_gossip / emit_header into a bounded buffer (pp_record)
// The recoveries (libbftsig on the GPU, the C oracle in the host build) sit between the record and classify().
#pragma once
#include "bft_common.h"
#include "bft_crypto.h"
#include "bft_wire.h"
#include "bft_wire_block.h"

namespace bft {
namespace audit {

// per-frame status (include/bftsim.h, SPEC.md §11c): the first matching row wins
enum : uint32_t { ST_OK = 0, ST_UNDECODABLE = 1, ST_UNRECOVERABLE = 2, ST_NOT_VALIDATOR = 3, ST_SEAL_BAD = 4, ST_SEAL_FOREIGN = 5 };
constexpr uint32_t NONE = 0xffffffffu;
constexpr uint32_t MAX_SPAN = 1u << 20;       // a longer span is undecodable unread (no decodable frame comes near it)
constexpr uint32_t ROUND_NONE = 0xffffu, ROUND_MAX = 0xfffeu;   // cert_round: none / the largest round it can hold

// the records of the decode pass, structure of arrays over the frames; `seal_dig` / `seal` are the dense list of
// the decodable Commits (slot seal_k[frame])
struct Recs {
    uint8_t* st;          // [F] ST_OK so far, or ST_UNDECODABLE
    uint8_t* code;        // [F] MessageType 1..4 (0: undecodable)
    uint32_t* hx;         // [F] height if 1..max_heights, else 0
    uint64_t* round;      // [F]
    uint8_t* digest;      // [F][32] Subject.digest, or Keccak-256 of a Preprepare's header with votes nil
    uint8_t* sdig;        // [F][32] sign digest
    uint8_t* sig;         // [F][65] zero when undecodable (never recovers)
    uint32_t* seal_k;     // [F] slot in the dense seal list, or NONE
    uint32_t* pp_want;    // [F] Preprepare: the rightful proposer's index if header.proposer is its address, else NONE
    uint8_t* seal_dig;    // [C][32] keccak(0x03 || digest)
    uint8_t* seal;        // [C][65]
};

BFT_FN void put32(uint8_t* dst, const uint8_t* src) { for (int i = 0; i < 32; ++i) dst[i] = src[i]; }
BFT_FN void put65(uint8_t* dst, const uint8_t* src) { for (int i = 0; i < 65; ++i) dst[i] = src[i]; }

BFT_FN void rec_undecodable(const Recs& r, uint64_t i) {
    r.st[i] = (uint8_t)ST_UNDECODABLE; r.code[i] = 0; r.hx[i] = 0; r.round[i] = 0; r.seal_k[i] = NONE; r.pp_want[i] = NONE;
    for (int k = 0; k < 32; ++k) { r.digest[32 * i + k] = 0; r.sdig[32 * i + k] = 0; }
    for (int k = 0; k < 65; ++k) r.sig[65 * i + k] = 0;
}
BFT_FN uint32_t height_in_range(uint64_t h, uint32_t max_heights) { return h >= 1 && h <= max_heights ? (uint32_t)h : 0u; }

// a decoded Subject frame -> its record (kbuf: 136 bytes). False: undecodable by the observer's rules (signature
// None, a Commit without a seal, another message with one). A Commit's seal goes to the dense list by seal_record.
BFT_FN bool subject_record(const wire::Decoded& d, uint32_t max_heights, uint8_t* kbuf, const Recs& r, uint64_t i) {
    const bool commit = d.code == (uint32_t)MT_COMMIT;
    if (!d.has_sig || (d.has_seal != 0) != commit) return false;
    r.st[i] = (uint8_t)ST_OK; r.code[i] = (uint8_t)d.code;
    r.hx[i] = height_in_range(d.height, max_heights);
    r.round[i] = d.round; r.seal_k[i] = NONE; r.pp_want[i] = NONE;
    put32(r.digest + 32 * i, d.digest);
    put65(r.sig + 65 * i, d.sig);
    crypto::sign_digest(kbuf, d.code, d.create_time, d.round, d.height, d.digest, nullptr, 0, commit ? d.seal : nullptr,
                        r.sdig + 32 * i);
    return true;
}
BFT_FN void seal_record(const wire::Decoded& d, uint8_t* kbuf, const Recs& r, uint64_t i, uint32_t k) {
    r.seal_k[i] = k;
    crypto::seal_digest(kbuf, d.digest, r.seal_dig + 32ull * k);
    put65(r.seal + 65ull * k, d.seal);
}
// Keccak-256 of len bytes through the absorber (kbuf: 136 bytes): one absorb site however long the message
BFT_FN void keccak_bytes(const uint8_t* p, uint32_t len, uint8_t* kbuf, uint8_t* out) {
    crypto::KSink k(kbuf);
    for (uint32_t j = 0; j < len; ++j) k.put(p[j]);
    k.finish(out);
}
// the largest unsigned payload of a decodable Preprepare: every field at its BFTWIRE_MAX_*, each byte a 2-byte uint
constexpr uint32_t PP_BUF = 6912;
// a decoded Preprepare frame -> its record; pp is restored before returning. The emitters count into a bounded
// buffer (mbuf: PP_BUF bytes), which is hashed in one loop: the block-carrying emitters have hundreds of byte sites,
// and an absorber behind each would be a Keccak-f behind each
BFT_FN bool pp_record(bftwire_preprepare& pp, uint32_t has_seal, const uint8_t* addresses, uint32_t n, bool seed_le,
                      uint32_t max_heights, uint8_t* kbuf, uint8_t* mbuf, const Recs& r, uint64_t i) {
    if (!pp.has_sig || has_seal) return false;
    uint32_t hl = 0, pl = 0;
    {   // the block's digest: its header with votes nil (SPEC.md §7)
        const uint32_t nv = pp.block.n_votes;
        pp.block.n_votes = BFTWIRE_NONE;
        wire::emit_header(wire::BufE{mbuf, &hl, PP_BUF}, pp.block);
        pp.block.n_votes = nv;
    }
    if (hl > PP_BUF) return false;
    keccak_bytes(mbuf, hl, kbuf, r.digest + 32 * i);
    wire::emit_pp_gossip(wire::BufE{mbuf, &pl, PP_BUF}, pp, false);
    if (pl > PP_BUF) return false;
    keccak_bytes(mbuf, pl, kbuf, r.sdig + 32 * i);
    r.st[i] = (uint8_t)ST_OK; r.code[i] = (uint8_t)MT_PREPREPARE;
    r.hx[i] = height_in_range(pp.height, max_heights);
    r.round[i] = pp.round; r.seal_k[i] = NONE;
    put65(r.sig + 65 * i, pp.signature);
    // the proposer of (prev_hash, round), by the rule of bftsim_calc_proposer under the handle's seed order
    const uint32_t w = (uint32_t)(((uint64_t)seed_from_hash(pp.block.prev_hash, n, seed_le) + pp.round % n) % n);
    bool same = true;
    for (int k = 0; k < 20; ++k) same = same && addresses[20u * w + k] == pp.block.proposer[k];
    r.pp_want[i] = same ? w : NONE;
    return true;
}

// index of a 20-byte address in the ascending validator table, or -1
BFT_FN int32_t find_validator(const uint8_t* addresses, uint32_t n, const uint8_t* a) {
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        int c = 0;
        for (int k = 0; k < 20 && c == 0; ++k) c = (int)addresses[20u * mid + k] - (int)a[k];
        if (c == 0) return (int32_t)mid;
        if (c < 0) lo = mid + 1; else hi = mid;
    }
    return -1;
}
// the final status of frame i from its record and the recoveries; *signer: validator index for 0, 4, 5, else -1
BFT_FN uint32_t classify(const Recs& r, uint64_t i, const uint8_t* addresses, uint32_t n, const uint8_t* rec_addr,
                         const uint8_t* rec_ok, const uint8_t* seal_addr, const uint8_t* seal_ok, int32_t* signer) {
    *signer = -1;
    if (r.st[i] != ST_OK) return ST_UNDECODABLE;
    if (!rec_ok[i]) return ST_UNRECOVERABLE;
    const int32_t v = find_validator(addresses, n, rec_addr + 20 * i);
    if (v < 0) return ST_NOT_VALIDATOR;
    *signer = v;
    if (r.code[i] != (uint8_t)MT_COMMIT) return ST_OK;
    const uint32_t k = r.seal_k[i];
    if (!seal_ok[k]) return ST_SEAL_BAD;
    for (int b = 0; b < 20; ++b)
        if (seal_addr[20ull * k + b] != rec_addr[20 * i + b]) return ST_SEAL_FOREIGN;
    return ST_OK;
}

// ---------------------------------------------------------------- the tally (per instance, in frame order)
// A key (height, round, digest) lives in slot `s` of its instance's table in insertion order: nothing is evicted.
enum : uint32_t { KEY_PROPOSED = 1, KEY_RIGHTFUL = 2, KEY_CERT = 4 };
enum : uint32_t { TALLY_CERTIFY = 1, TALLY_CONFLICT = 2 };
struct Key {
    uint64_t digest[4];
    uint64_t round;
    uint64_t voters[4];
    uint32_t height, flags, proposer, pad;
};
struct Vote {                       // an accepted Preprepare or Commit with a height in range
    uint64_t digest[4];
    uint64_t round;
    uint32_t hx, code, signer, want;
};
BFT_FN bool same_digest(const uint64_t* a, const uint64_t* b) { return ((a[0] ^ b[0]) | (a[1] ^ b[1]) | (a[2] ^ b[2]) | (a[3] ^ b[3])) == 0; }
// how slot k relates to a vote: 1 its key, 2 a certificate at its height, 4 that certificate carries its digest
BFT_FN uint32_t key_relation(const Key& k, const Vote& v) {
    if (k.height != v.hx) return 0;
    const bool deq = same_digest(k.digest, v.digest), cert = (k.flags & KEY_CERT) != 0;
    return (deq && k.round == v.round ? 1u : 0u) | (cert ? 2u : 0u) | (cert && deq ? 4u : 0u);
}
// the vote into its key (fresh: the slot is new). has_cert: the height already has a certificate (of another digest:
// Commits carrying the certified one never get here). Returns TALLY_* for the caller's certificate row and counters.
BFT_FN uint32_t tally_apply(Key& k, bool fresh, const Vote& v, uint32_t quorum, bool has_cert) {
    if (fresh) {
        for (int i = 0; i < 4; ++i) { k.digest[i] = v.digest[i]; k.voters[i] = 0; }
        k.round = v.round; k.height = v.hx; k.flags = 0; k.proposer = NONE; k.pad = 0;
    }
    if (v.code == (uint32_t)MT_PREPREPARE) {
        k.flags |= KEY_PROPOSED | (v.signer == v.want ? (uint32_t)KEY_RIGHTFUL : 0u);
        k.proposer = v.signer;
        return 0;
    }
    const uint64_t bit = 1ull << (v.signer & 63u);
    uint64_t& w = k.voters[(v.signer >> 6) & 3u];
    if (w & bit) return 0;
    w |= bit;
    uint32_t pc = 0;
    for (int i = 0; i < 4; ++i) pc += (uint32_t)__builtin_popcountll(k.voters[i]);
    if (pc != quorum + 1u) return 0;            // only the vote that crosses the quorum acts
    if (has_cert) return TALLY_CONFLICT;
    k.flags |= KEY_CERT;
    return TALLY_CERTIFY;
}
BFT_FN uint32_t cert_flags(const Key& k) { return ((k.flags & KEY_PROPOSED) ? 1u : 0u) | ((k.flags & KEY_RIGHTFUL) ? 2u : 0u); }
BFT_FN uint16_t cert_round(const Key& k) { return (uint16_t)(k.round < ROUND_MAX ? k.round : ROUND_MAX); }

// ---------------------------------------------------------------- the GPU passes (kern_audit.hip)
// frame k of the pass spans stream[foff[k] - base, foff[k + 1] - base); no byte outside a frame's span is read
struct DecodeArgs {
    const uint8_t* stream;
    const uint64_t* foff;
    uint64_t base, frames;
    const uint8_t* addresses;
    uint32_t n, seed_le, max_heights;
    Recs r;
    uint32_t* n_seals;                // the dense seal list's length
};
// the report's counters on the device
enum : uint32_t { CNT_STATUS = 0, CNT_CODE = 6, CNT_OUT_OF_RANGE = 10, CNT_CERTIFIED = 11, CNT_CONFLICTS = 12,
                  CNT_KEY_OVERFLOWS = 13, CNT_WORDS = 16 };
struct ClassifyArgs {
    Recs r;
    uint64_t frames;
    const uint8_t* addresses;
    uint32_t n;
    const uint8_t *rec_addr, *rec_ok, *seal_addr, *seal_ok;
    uint8_t* status;                  // [F]
    int32_t* signer;                  // [F]
    unsigned long long* counts;       // [CNT_WORDS]
};
struct TallyArgs {
    Recs r;
    const uint8_t* status;
    const int32_t* signer;
    const uint64_t* inst_frame0;      // [inst + 1]
    uint64_t inst;
    Key* keys;                        // [inst][key_cap]
    uint32_t key_cap, max_heights, quorum;
    uint32_t* inst_flags;             // [inst]
    uint16_t* cert_round;             // [inst * max_heights], preset to ROUND_NONE
    uint8_t* cert_digest;             // x32
    uint64_t* cert_voters;            // x4
    uint32_t* cert_frame;
    uint8_t* cert_flags;
    unsigned long long* counts;
};
#if defined(__HIPCC__)
hipError_t launch_decode(const DecodeArgs& a, hipStream_t s);
hipError_t launch_classify(const ClassifyArgs& a, hipStream_t s);
hipError_t launch_tally(const TallyArgs& a, hipStream_t s);
#endif

}  // namespace audit
}  // namespace bft
