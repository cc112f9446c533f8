// bft_timeline.h — the chronicler of a trace (SPEC.md §11h): over the Prepare and RoundChange frames
// the observer accepts, per height the first prepare certificate, the round-change quorums, and three verdicts that
// join them to the observer's commit certificate. Shared by the host build (tests/emu/timeline_host.cpp) and the GPU
// kernels (kern_timeline.hip). It reads the observer's records (bft_audit.h: code, hx, round, digest), statuses,
// signers and certificate rows, and writes none of them.
//   walk   per instance, in frame order: a table of keys in insertion order, nothing evicted. A Prepare key is
//          (height, round, digest), a RoundChange key (height, round): the digest of a RoundChange is never read
//          (round_change.rs:78-92). The vote that takes a key's distinct voters past the quorum marks the key and
//          writes the height's row.
//   rows   per (instance, height): the flags, from the row, the certificate row and the instance's marked keys.
#pragma once
#include "bft_audit.h"

namespace bft {
namespace timeline {

using audit::NONE;
using audit::ROUND_MAX;
using audit::ROUND_NONE;
enum : uint32_t { FLAG_KEY_OVERFLOW = 1 };                                        // include/bftsim.h BFTSIM_TIMELINE_KEY_OVERFLOW
enum : uint32_t { ROW_PREPARED_FIRST = 1, ROW_CERT_UNPREPARED = 2, ROW_LOCKED_OPEN = 4 };   // BFTSIM_TIMELINE_*
enum : uint32_t { CNT_PREPARE_FRAMES = 0, CNT_RC_FRAMES = 1, CNT_OUT_OF_RANGE = 2, CNT_PREPARED = 3, CNT_RC_QUORUMS = 4,
                  CNT_RC_HEIGHTS = 5, CNT_PREPARED_FIRST = 6, CNT_CERT_UNPREPARED = 7, CNT_LOCKED_OPEN = 8,
                  CNT_KEY_OVERFLOWS = 9, CNT_WORDS = 12 };

struct Key {
    uint64_t digest[4];               // a RoundChange key: zero, never compared
    uint64_t round;
    uint64_t voters[4];
    uint32_t height, code;            // MT_PREPARE or MT_ROUND_CHANGE
    uint32_t quorate, qframe;         // the key reached its quorum, at this frame of the instance
};
static_assert(sizeof(Key) == 88, "table layout");

// the rows, [inst * max_heights] each; prep_round, rc_max_round and rc_top_round preset to ROUND_NONE, the rest to 0
struct Rows {
    uint16_t* prep_round;
    uint8_t* prep_digest;             // x32
    uint64_t* prep_voters;            // x4
    uint32_t* prep_frame;
    uint16_t *prep_quorums, *rc_quorums, *rc_max_round;
    uint32_t* rc_max_frame;
    uint16_t* rc_top_round;
    uint32_t* rc_frames;
    uint8_t* flags;
};
// the observer's certificate rows
struct Certs {
    const uint16_t* round;
    const uint8_t* digest;            // x32
    const uint32_t* frame;
};

BFT_FN uint32_t default_cap(uint32_t max_heights) { return 4u * max_heights + 64u; }
BFT_FN uint16_t clip(uint64_t round) { return (uint16_t)(round < ROUND_MAX ? round : ROUND_MAX); }
BFT_FN uint16_t sat_inc(uint16_t x) { return (uint16_t)(x < 0xffffu ? x + 1u : x); }
// the frames that count: accepted by the observer, Prepare or RoundChange; hx (0: the height is out of range) decides
// between the table and out_of_range
BFT_FN bool counts(uint32_t status, uint32_t code) {
    return (status == audit::ST_OK || status == audit::ST_SEAL_FOREIGN) && (code == (uint32_t)MT_PREPARE || code == (uint32_t)MT_ROUND_CHANGE);
}
// digest: the frame's row of the records, 8-byte aligned; read for a Prepare only
BFT_FN bool key_is(const Key& k, uint32_t code, uint32_t hx, uint64_t round, const uint64_t* digest) {
    if (k.code != code || k.height != hx || k.round != round) return false;
    return code != (uint32_t)MT_PREPARE || audit::same_digest(k.digest, digest);
}
BFT_FN void key_put(Key& k, uint32_t code, uint32_t hx, uint64_t round, const uint64_t* digest) {
    const bool prep = code == (uint32_t)MT_PREPARE;
    for (int i = 0; i < 4; ++i) { k.digest[i] = prep ? digest[i] : 0ull; k.voters[i] = 0; }
    k.round = round; k.height = hx; k.code = code; k.quorate = 0; k.qframe = 0;
}
// the vote of `signer` (below 256) at frame `rel` of the instance into its key. True for the one vote that takes the
// key past the quorum; the voters stand as they are then, and later votes change nothing
BFT_FN bool key_vote(Key& k, uint32_t signer, uint32_t quorum, uint32_t rel) {
    if (k.quorate) return false;
    const uint64_t bit = 1ull << (signer & 63u);
    uint64_t& w = k.voters[(signer >> 6) & 3u];
    if (w & bit) return false;
    w |= bit;
    uint32_t pc = 0;
    for (int i = 0; i < 4; ++i) pc += (uint32_t)__builtin_popcountll(k.voters[i]);
    if (pc <= quorum) return false;
    k.quorate = 1; k.qframe = rel;
    return true;
}
// the row's single writer, on a Prepare key's quorum: the first one is described, every one counted
BFT_FN void row_prepare(const Rows& o, uint64_t row, uint64_t round, const uint64_t* digest, uint64_t w0, uint64_t w1,
                        uint64_t w2, uint64_t w3, uint32_t rel) {
    const uint16_t q = o.prep_quorums[row];
    o.prep_quorums[row] = sat_inc(q);
    if (q) return;
    o.prep_round[row] = clip(round);
    for (int i = 0; i < 4; ++i) ((uint64_t*)(o.prep_digest + 32 * row))[i] = digest[i];
    o.prep_voters[4 * row] = w0; o.prep_voters[4 * row + 1] = w1; o.prep_voters[4 * row + 2] = w2; o.prep_voters[4 * row + 3] = w3;
    o.prep_frame[row] = rel;
}
// on a RoundChange key's quorum. inst_round: the records' rounds from the instance's first frame on; the round of the
// greatest key so far is its completing frame's
BFT_FN void row_rc_quorum(const Rows& o, uint64_t row, uint64_t round, uint32_t rel, const uint64_t* inst_round) {
    const uint16_t q = o.rc_quorums[row];
    o.rc_quorums[row] = sat_inc(q);
    if (q && inst_round[o.rc_max_frame[row]] >= round) return;
    o.rc_max_round[row] = clip(round);
    o.rc_max_frame[row] = rel;
}
// on every RoundChange frame that found its key
BFT_FN void row_rc_frame(const Rows& o, uint64_t row, uint64_t round) {
    const uint16_t c = clip(round), t = o.rc_top_round[row];
    if (t == ROUND_NONE || c > t) o.rc_top_round[row] = c;
    o.rc_frames[row] += 1u;
}
// the flags of height x. cert_full_round: the round of the frame cert_frame, as the archiver reads it
BFT_FN uint32_t row_flags(const Key* keys, uint32_t nkeys, uint32_t x, bool prepared, bool has_cert, const uint64_t* cert_digest,
                          uint64_t cert_full_round, uint32_t cert_frame) {
    if (!has_cert) return prepared ? (uint32_t)ROW_LOCKED_OPEN : 0u;
    bool any = false, first = false;
    for (uint32_t s = 0; s < nkeys; ++s) {
        const Key& k = keys[s];
        if (k.code != (uint32_t)MT_PREPARE || k.height != x || !k.quorate || !audit::same_digest(k.digest, cert_digest)) continue;
        any = true;
        first = first || (k.round == cert_full_round && k.qframe < cert_frame);
    }
    return (first ? (uint32_t)ROW_PREPARED_FIRST : 0u) | (any ? 0u : (uint32_t)ROW_CERT_UNPREPARED);
}

// ---------------------------------------------------------------- the GPU passes (kern_timeline.hip)
struct Args {
    audit::Recs r;
    const uint8_t* status;            // [F]
    const int32_t* signer;            // [F]
    const uint64_t* inst_frame0;      // [inst + 1]
    uint64_t inst;
    uint32_t n, tl_cap, max_heights, quorum;
    Certs certs;
    Key* keys;                        // [inst][tl_cap]
    uint32_t* inst_nkeys;             // [inst]
    uint32_t* inst_flags;             // [inst]
    uint32_t* open_height;            // [inst]
    Rows rows;
    unsigned long long* counts;       // [CNT_WORDS]
};
#if defined(__HIPCC__)
hipError_t launch_walk(const Args& a, hipStream_t s);
hipError_t launch_rows(const Args& a, hipStream_t s);
#endif

}  // namespace timeline
}  // namespace bft
