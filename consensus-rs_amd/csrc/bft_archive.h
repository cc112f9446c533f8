// bft_archive.h — the archiver of a trace (SPEC.md §11e): from the observer's records and certificate rows
// (bft_audit.h) the ledger Header of every certified height with its commit seals, in bftsim_export_ledger's slot
// layout. Shared by the host build (tests/emu/archive_host.cpp) and the GPU kernels (kern_archive.hip):
//   pick   per frame: the table word an accepted PrePrepare or Commit competes for, smallest frame index wins
//   emit   per certified row: the picked PrePrepare frame decoded again, its 12 leading fields re-encoded
//          (wire::emit_header_front), then the votes: the seals of the picked Commit frames, as received
//   heights per instance: the prefix of OK slots
// The pick table has PICK_WORDS(quorum) words a row: word 0 the PrePrepare, word 1 + r the Commit of the voter of
// rank r in the certificate's bitmap. A certificate is written by the vote that makes popcount Q + 1 (tally_apply),
// so a bitmap holds exactly Q + 1 voters.
#pragma once
#include "bft_audit.h"

namespace bft {
namespace archive {

enum : uint32_t { AR_OK = 0, AR_NONE = 1, AR_NO_PROPOSAL = 2 };
using audit::NONE;
// the report's counters on the device
enum : uint32_t { CNT_STATUS = 0, CNT_VOTES = 3, CNT_FOREIGN = 4, CNT_ARCHIVED = 5, CNT_ERR = 6, CNT_WORDS = 8 };

BFT_FN uint32_t pick_words(uint32_t quorum) { return quorum + 2u; }

// the certificate rows of the tally, read-only
struct Certs {
    const uint16_t* round;            // [rows] ROUND_NONE: no certificate
    const uint8_t* digest;            // x32
    const uint64_t* voters;           // x4
    const uint32_t* frame;            // the completing frame, index within the instance
};

BFT_FN bool is_voter(const uint64_t* w, uint32_t v) { return ((w[(v >> 6) & 3u] >> (v & 63u)) & 1ull) != 0; }
// validators below v in the bitmap
BFT_FN uint32_t voter_rank(const uint64_t* w, uint32_t v) {
    uint32_t r = 0;
    for (uint32_t q = 0; q < (v >> 6); ++q) r += (uint32_t)__builtin_popcountll(w[q]);
    return r + (uint32_t)__builtin_popcountll(w[v >> 6] & ((1ull << (v & 63u)) - 1ull));
}
BFT_FN uint32_t voter_count(const uint64_t* w) {
    return (uint32_t)(__builtin_popcountll(w[0]) + __builtin_popcountll(w[1]) + __builtin_popcountll(w[2]) + __builtin_popcountll(w[3]));
}
// the validator of rank r in the bitmap (r < voter_count)
BFT_FN uint32_t voter_at(const uint64_t* w, uint32_t r) {
    uint32_t q = 0;
    for (; q < 3; ++q) {
        const uint32_t c = (uint32_t)__builtin_popcountll(w[q]);
        if (r < c) break;
        r -= c;
    }
    uint64_t m = w[q];
    for (uint32_t k = 0; k < r; ++k) m &= m - 1ull;
    return 64u * q + (uint32_t)__builtin_ctzll(m | (1ull << 63));
}
BFT_FN bool same32(const uint8_t* a, const uint8_t* b) {
    uint32_t d = 0;
    for (int i = 0; i < 32; ++i) d |= (uint32_t)(a[i] ^ b[i]);
    return d == 0;
}

// the pick table word frame k (of the instance whose first frame is f0 and first row is row0) competes for, or NONE:
// an accepted PrePrepare with its height's certified digest, or an accepted Commit with the certificate's digest, the
// full round of the completing frame and a signer in its bitmap
BFT_FN uint64_t pick_word(const audit::Recs& r, const uint8_t* status, const int32_t* signer, uint64_t k, uint64_t f0,
                          uint64_t row0, const Certs& c, uint32_t quorum) {
    const uint32_t st = status[k], code = r.code[k], hx = r.hx[k];
    if (!(st == audit::ST_OK || st == audit::ST_SEAL_FOREIGN) || hx == 0) return ~0ull;
    if (code != (uint32_t)MT_PREPREPARE && code != (uint32_t)MT_COMMIT) return ~0ull;
    const uint64_t row = row0 + (hx - 1u);
    if (c.round[row] == audit::ROUND_NONE || !same32(r.digest + 32 * k, c.digest + 32 * row)) return ~0ull;
    const uint64_t w0 = row * pick_words(quorum);
    if (code == (uint32_t)MT_PREPREPARE) return w0;
    const uint32_t v = (uint32_t)signer[k];
    const uint64_t* vw = c.voters + 4 * row;
    if (v > 255u || !is_voter(vw, v) || r.round[k] != r.round[f0 + c.frame[row]]) return ~0ull;
    const uint32_t rank = voter_rank(vw, v);
    return rank <= quorum ? w0 + 1u + rank : ~0ull;
}

// ---------------------------------------------------------------- the emit step
// the votes' array header (bft_export_votes_kernel's): 0x90 | n below 16, else 0xdc and 16 bits
BFT_FN uint32_t votes_head_len(uint32_t n) { return n < 16u ? 1u : 3u; }
BFT_FN void votes_head(const wire::BufE& e, uint32_t n) {
    if (n < 16u) e(0x90u | n);
    else { e(0xdc); e(n >> 8); e(n & 0xffu); }
}
// one vote: 0xdc 00 41, then 65 compact uints
BFT_FN uint32_t vote_len(const uint8_t* seal) {
    uint32_t n = 3u + 65u;
    for (int i = 0; i < 65; ++i) n += seal[i] >> 7;
    return n;
}
// the vote at slot[at...), every store bounded by cap; returns the bytes it takes
BFT_FN uint32_t write_vote(uint8_t* slot, uint32_t at, uint32_t cap, const uint8_t* seal) {
    uint32_t n = at;
    const wire::BufE e{slot, &n, cap};
    e(0xdc); e(0x00); e(65);
    for (int i = 0; i < 65; ++i) {
        const uint32_t b = seal[i];
        if (b >= 128u) e(0xcc);
        e(b);
    }
    return n - at;
}
// the header's 12 leading fields from frame p[0, span), re-encoded into slot[0, cap); the length they take (stores
// beyond cap are dropped, the length still counts them), or NONE when the frame no longer decodes (it did in the
// decode pass: the caller counts an error). seal_buf: 65 bytes
BFT_FN uint32_t emit_front(const uint8_t* p, uint64_t span, bftwire_preprepare& pp, uint8_t* seal_buf, uint8_t* slot,
                           uint32_t cap) {
    uint32_t has_seal = 0, n = 0;
    if (span > audit::MAX_SPAN || !wire::decode_pp_frame(p, (uint32_t)span, pp, &has_seal, seal_buf)) return NONE;
    wire::emit_header_front(wire::BufE{slot, &n, cap}, pp.block);
    return n;
}

// the status of a row from its certificate and its pick words
BFT_FN uint32_t row_status(const Certs& c, uint64_t row, const uint32_t* pick, uint32_t quorum) {
    if (c.round[row] == audit::ROUND_NONE) return AR_NONE;
    return pick[row * pick_words(quorum)] == NONE ? (uint32_t)AR_NO_PROPOSAL : (uint32_t)AR_OK;
}
// the largest x with slots 1..x all OK; *whole: the rest are NONE
BFT_FN uint64_t archived_height(const uint8_t* status, uint32_t H, bool* whole) {
    uint32_t x = 0;
    while (x < H && status[x] == AR_OK) ++x;
    bool w = true;
    for (uint32_t y = x; y < H; ++y) w = w && status[y] == AR_NONE;
    *whole = w;
    return x;
}

// ---------------------------------------------------------------- the GPU passes (kern_archive.hip)
struct Args {
    const uint8_t* stream;            // frame k = stream[foff[k] - base, foff[k + 1] - base)
    const uint64_t* foff;
    uint64_t base, frames;
    audit::Recs r;
    const uint8_t* status;            // [F] the observer's
    const int32_t* signer;            // [F]
    const uint64_t* inst_frame0;      // [inst + 1]
    uint64_t inst;
    uint32_t max_heights, quorum;
    Certs c;
    uint32_t* pick;                   // [rows][pick_words] preset to NONE
    uint8_t* hdr;                     // [rows][slot_bytes]
    uint64_t slot_bytes;
    uint32_t* hdr_len;                // [rows]
    uint8_t* out_status;              // [rows]
    uint32_t* pp_frame;               // [rows]
    uint16_t* n_votes;                // [rows]
    uint16_t* n_foreign;              // [rows] of those, from SEAL_FOREIGN frames
    uint64_t* height;                 // [inst]
    unsigned long long* counts;       // [CNT_WORDS]
};
#if defined(__HIPCC__)
hipError_t launch_pick(const Args& a, hipStream_t s);
hipError_t launch_emit(const Args& a, hipStream_t s);
hipError_t launch_heights(const Args& a, hipStream_t s);
#endif

}  // namespace archive
}  // namespace bft
