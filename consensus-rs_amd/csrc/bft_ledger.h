// bft_ledger.h — the importer of a ledger (SPEC.md §11d): what a syncing node runs on every Header it is handed,
// `verify_header(header, seal = true)` + `verify_seal` (src/consensus/backend.rs:319-367), as step functions shared by
// the host build (tests/emu/ledger_host.cpp) and the GPU kernels (kern_ledger.hip):
//   decode_header   one slot of bftsim_export_ledger's layout -> a fixed-size record: the fields with the primitives of
//                   bft_wire.h / bft_wire_block.h, the votes counted and checked where they lie (no bftwire_block: that
//                   caps votes at BFTWIRE_MAX_VOTES), the block hash = Keccak-256 of the fields re-encoded with votes nil
//                   (emit_header_front + nil), the seal digest keccak(0x03 || block hash) (types/votes.rs:94-101)
//   scatter_votes   the 65 bytes of every vote of a header into the dense vote list
//   tally_vote      a recovered vote into its header's voter bitmap
//   link_status     the final status, in the reference's order: height, parent, prev_hash, time, then verify_seal's
//                   votes None -> LackVotes, verify_signs -> InvalidSignature (BAD_VOTE, decided before the count),
//                   count -> LackVotes, proposer -> not a validator
// The recoveries (libbftsig on the GPU, the C oracle in the host build) sit between scatter_votes and tally_vote.
// A ledger header is flat bytes, so the cursor (wire::Mem) is a value; every decoded field goes straight to the record
// in memory and is read back by the emitter: a lane keeps no byte array of its own.
#pragma once
#include "bft_common.h"
#include "bft_crypto.h"
#include "bft_wire.h"
#include "bft_wire_block.h"
#include "bft_audit.h"

namespace bft {
namespace ledger {

// per-header status (include/bftsim.h BFTSIM_LEDGER_*): the first matching row wins
enum : uint32_t { ST_OK = 0, ST_ABSENT = 1, ST_UNDECODABLE = 2, ST_BAD_HEIGHT = 3, ST_NO_PARENT = 4, ST_BAD_PARENT = 5,
                  ST_BAD_TIME = 6, ST_LACK_VOTES = 7, ST_BAD_VOTE = 8, ST_BAD_PROPOSER = 9, ST_COUNT = 10 };
constexpr uint32_t NONE = 0xffffffffu;
constexpr uint32_t MAX_VOTES = 256;           // a header with more is undecodable (a set has at most 256 validators)

// a decoded header. `st` is ST_OK so far, ST_ABSENT or ST_UNDECODABLE; the other fields are zero unless ST_OK
struct Rec {
    uint64_t bloom, difficulty, height, gas_limit, gas_used, time;
    uint32_t extra_len;                       // NONE: extra None; else <= BFTWIRE_MAX_EXTRA
    uint32_t n_votes;                         // NONE: votes None (or fewer than 13 fields); else <= MAX_VOTES
    uint32_t voff;                            // offset of the first vote in the slot
    uint32_t st;
    uint8_t prev_hash[32], root[32], tx_hash[32], receipt_hash[32];
    uint8_t proposer[20];
    uint8_t extra[BFTWIRE_MAX_EXTRA];
    uint8_t pad[4];
    uint8_t bhash[32];                        // block hash (votes nil)
    uint8_t sdig[32];                         // keccak(0x03 || bhash): what every vote is recovered over
};

BFT_FN void rec_blank(Rec& r, uint32_t st) {
    r.bloom = r.difficulty = r.height = r.gas_limit = r.gas_used = r.time = 0;
    r.extra_len = NONE; r.n_votes = NONE; r.voff = 0; r.st = st;
    for (int k = 0; k < 32; ++k) { r.prev_hash[k] = 0; r.root[k] = 0; r.tx_hash[k] = 0; r.receipt_hash[k] = 0; r.bhash[k] = 0; r.sdig[k] = 0; }
    for (int k = 0; k < 20; ++k) r.proposer[k] = 0;
    for (int k = 0; k < (int)BFTWIRE_MAX_EXTRA; ++k) r.extra[k] = 0;
    for (int k = 0; k < 4; ++k) r.pad[k] = 0;
}
// one vote where it lies: an array of 65 integers 0..255
BFT_FN bool skip_vote(wire::Mem& m) {
    uint32_t n;
    if (!wire::rd_arr(m, n) || n != 65) return false;
    for (uint32_t i = 0; i < 65; ++i) {
        uint64_t v;
        if (!wire::rd_uint(m, v) || v > 255) return false;
    }
    return true;
}
// Header {prev_hash, proposer, root, tx_hash, receipt_hash, bloom, difficulty, height, gas_limit, gas_used, time,
// extra, votes} (types/block.rs:16-36); extra and votes are #[serde(default)]: 11 to 13 fields
BFT_FN bool parse_header(wire::Mem& m, Rec& r) {
    uint32_t hf, tag;
    if (!wire::rd_arr(m, hf) || hf < 11 || hf > 13) return false;
    if (!wire::rd_bytes_fixed(m, 32, r.prev_hash) || !m.get(tag) || !wire::rd_address_tag(m, tag, r.proposer)) return false;
    if (!wire::rd_bytes_fixed(m, 32, r.root) || !wire::rd_bytes_fixed(m, 32, r.tx_hash) ||
        !wire::rd_bytes_fixed(m, 32, r.receipt_hash))
        return false;
    if (!wire::rd_uint(m, r.bloom) || !wire::rd_uint(m, r.difficulty) || !wire::rd_uint(m, r.height) ||
        !wire::rd_uint(m, r.gas_limit) || !wire::rd_uint(m, r.gas_used) || !wire::rd_uint(m, r.time))
        return false;
    if (hf >= 12) {
        if (!m.get(tag)) return false;
        if (tag != 0xc0 && !wire::rd_bytes_var(m, tag, BFTWIRE_MAX_EXTRA, r.extra, r.extra_len)) return false;
    }
    if (hf >= 13) {
        if (!m.get(tag)) return false;
        if (tag != 0xc0) {
            uint32_t nv;
            if (!wire::rd_arr_tag(m, tag, nv) || nv > MAX_VOTES) return false;
            r.voff = m.i;
            for (uint32_t v = 0; v < nv; ++v)
                if (!skip_vote(m)) return false;
            r.n_votes = nv;
        }
    }
    return m.i == m.n;                            // no trailing bytes
}
// slot p of hdr_len bytes (slot_bytes available) -> r (kbuf: 136 bytes); returns the votes it adds to the dense list
BFT_FN uint32_t decode_header(const uint8_t* p, uint32_t hdr_len, uint64_t slot_bytes, uint8_t* kbuf, Rec& r) {
    rec_blank(r, hdr_len == 0 ? (uint32_t)ST_ABSENT : (uint32_t)ST_UNDECODABLE);
    if (hdr_len == 0 || hdr_len > slot_bytes) return 0;          // a length above the slot: nothing is read
    wire::Mem m{p, hdr_len, 0};
    if (!parse_header(m, r)) { rec_blank(r, ST_UNDECODABLE); return 0; }
    r.st = ST_OK;
    {
        crypto::KSink k(kbuf);
        const wire::KE e{&k};
        wire::emit_header_front(e, r);
        e(0xc0);                                  // votes: nil (block_hash() ignores them, types/block.rs:76-80)
        k.finish(r.bhash);
    }
    crypto::seal_digest(kbuf, r.bhash, r.sdig);
    return r.n_votes == NONE ? 0u : r.n_votes;
}
// the votes of header `hdr_index` (decoded: r.st == ST_OK, r.n_votes != NONE) into slots [base, base + n_votes)
BFT_FN void scatter_votes(const uint8_t* p, uint32_t hdr_len, const Rec& r, uint32_t hdr_index, uint64_t base, uint8_t* vsig,
                          uint32_t* vhdr, uint8_t* vdig) {
    wire::Mem m{p, hdr_len, r.voff};
    for (uint32_t v = 0; v < r.n_votes; ++v) {
        const uint64_t k = base + v;
        if (!wire::rd_bytes_fixed(m, 65, vsig + 65 * k))            // cannot fail: decode_header walked these bytes
            for (int j = 0; j < 65; ++j) vsig[65 * k + j] = 0;
        vhdr[k] = hdr_index;
        for (int j = 0; j < 32; ++j) vdig[32 * k + j] = r.sdig[j];
    }
}

// a header's votes after the recoveries
struct Tally {
    uint64_t voters[4];                       // validators whose seal recovered
    uint32_t dup;                             // votes of a validator already in `voters`
    uint32_t bad;                             // a vote that does not recover, or recovers outside the set
};
BFT_FN void tally_vote(Tally& t, int32_t v) {
    if (v < 0) { t.bad = 1; return; }
    const uint64_t bit = 1ull << ((uint32_t)v & 63u);
    uint64_t& w = t.voters[((uint32_t)v >> 6) & 3u];
    if (w & bit) t.dup += 1; else w |= bit;
}
// validator index of recovered vote k, or -1
BFT_FN int32_t vote_validator(const uint8_t* addresses, uint32_t n, const uint8_t* vaddr, const uint8_t* vok, uint64_t k) {
    return vok[k] ? audit::find_validator(addresses, n, vaddr + 20 * k) : -1;
}
BFT_FN uint32_t popc4(const uint64_t* w) {
    return (uint32_t)(__builtin_popcountll(w[0]) + __builtin_popcountll(w[1]) + __builtin_popcountll(w[2]) + __builtin_popcountll(w[3]));
}
BFT_FN bool same32(const uint8_t* a, const uint8_t* b) {
    uint32_t d = 0;
    for (int k = 0; k < 32; ++k) d |= (uint32_t)(a[k] ^ b[k]);
    return d == 0;
}
// the final status of the header in slot x (1-based) of an instance whose records are inst[0 .. H): the reference's
// order (backend.rs:320-366). The parent of x = 1 is the genesis; of x > 1 slot x - 1 as decoded, verified or not
BFT_FN uint32_t link_status(const Rec* inst, uint32_t x, const uint8_t* genesis_hash, uint64_t genesis_time,
                            uint32_t block_period, const uint64_t* voters, uint32_t bad, uint32_t quorum,
                            const uint8_t* addresses, uint32_t n) {
    const Rec& r = inst[x - 1];
    if (r.st != ST_OK) return r.st;
    if (r.height == 0 || r.height != x) return ST_BAD_HEIGHT;
    const uint8_t* phash = genesis_hash;
    uint64_t ptime = genesis_time;
    if (x > 1) {
        const Rec& p = inst[x - 2];
        if (p.st != ST_OK) return ST_NO_PARENT;
        phash = p.bhash;
        ptime = p.time;
    }
    if (!same32(r.prev_hash, phash)) return ST_BAD_PARENT;
    // time < parent.time + block_period; a sum past 2^64 is above every time
    if (ptime > ~0ull - block_period || r.time < ptime + block_period) return ST_BAD_TIME;
    if (r.n_votes == NONE) return ST_LACK_VOTES;
    if (bad) return ST_BAD_VOTE;
    if (popc4(voters) <= quorum) return ST_LACK_VOTES;              // distinct voters (SPEC.md §11d)
    if (audit::find_validator(addresses, n, r.proposer) < 0) return ST_BAD_PROPOSER;
    return ST_OK;
}
// the largest x with slots 1..x all OK; *whole: every non-absent slot is OK and the absent ones form a suffix
BFT_FN uint64_t verified_height(const uint8_t* status, uint32_t H, bool* whole) {
    uint32_t x = 0;
    while (x < H && status[x] == ST_OK) ++x;
    bool w = true;
    for (uint32_t y = x; y < H; ++y) w = w && status[y] == ST_ABSENT;
    *whole = w;
    return x;
}

// ---------------------------------------------------------------- the GPU passes (kern_ledger.hip)
enum : uint32_t { CNT_STATUS = 0, CNT_HEADERS = 10, CNT_DUP = 11, CNT_WHOLE = 12, CNT_WORDS = 16 };
enum : uint32_t { TALLY_LANE = 1, TALLY_WAVE = 2 };      // lane per header / wave per header
struct Args {
    const uint8_t* hdr;                       // [slots][slot_bytes]
    const uint32_t* hdr_len;                  // [slots]
    uint64_t slot_bytes, slots;
    uint32_t inst, H;
    const uint8_t* addresses;
    uint32_t n, quorum, block_period;
    const uint8_t* genesis_hash;
    uint64_t genesis_time;
    Rec* recs;                                // [slots]
    unsigned long long* vbase;                // [slots + 1] votes per header, then (scanned) first dense slot
    // dense, per vote
    uint64_t votes;
    uint8_t *vsig, *vdig, *vaddr, *vok;
    uint32_t* vhdr;
    // per header
    uint64_t* voters;                         // [slots][4]
    uint32_t* dup;
    uint8_t *bad, *status, *bhash;
    uint16_t* n_votes;
    uint64_t* vheight;                        // [inst]
    unsigned long long* counts;               // [CNT_WORDS]
};
#if defined(__HIPCC__)
hipError_t launch_decode(const Args& a, hipStream_t s);
hipError_t launch_scatter(const Args& a, hipStream_t s);
hipError_t launch_tally(const Args& a, uint32_t mapping, hipStream_t s);
hipError_t launch_link(const Args& a, hipStream_t s);
#endif

}  // namespace ledger
}  // namespace bft
