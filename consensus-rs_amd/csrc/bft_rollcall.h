// bft_rollcall.h — the roll call of a trace (SPEC.md §11i): per validator what it signed, and per view
// the wire proves started, who had to propose and whether it did. Shared by the host build (tests/emu/rollcall_host.cpp)
// and the GPU kernels (kern_rollcall.hip). It reads the observer's records, statuses, signers and certificate rows
// (bft_audit.h) and the chronicler's key table (bft_timeline.h), and writes none of them.
//   views  per instance: the due views, sorted by (height, round). A candidate is a height (its round 0) or a slot of
//          the chronicler's table (a quorate RoundChange key of a round above 0); keys are unique, so a view's place is
//          the number of smaller due candidates. Each view gets its proposer from its parent's hash.
//   walk   per instance over the frames: the validators' counters, and every counting PrePrepare against the views.
//          Then the outcomes, and the validators' due / proposed / missed / won.
//   gather the views of all instances into one list of records, by an exclusive scan of the instances' counts.
#pragma once
#include "bft_timeline.h"

namespace bft {
namespace rollcall {

using audit::NONE;
using audit::ROUND_NONE;
enum : uint32_t { OUT_PROPOSED = 1, OUT_MISSED = 2, OUT_UNATTRIBUTED = 3, OUT_WON = 0x100 };   // include/bftsim.h BFTSIM_ROLLCALL_*
enum : uint32_t { FLAG_PARTIAL = 1 };
enum : uint32_t { CNT_FRAMES = 0, CNT_OUT_OF_RANGE = 1, CNT_VIEWS = 2, CNT_OUTCOME = 3, CNT_WON = 6, CNT_SILENT = 7,
                  CNT_SILENT_INST = 8, CNT_PARTIAL_INST = 9, CNT_WORDS = 12 };
// a validator's counters while an instance is walked (the kernels keep them in LDS)
enum : uint32_t { ROW_FRAMES = 0, ROW_LAST_HEIGHT = 4, ROW_LAST_FRAME = 5, ROW_DUE = 6, ROW_PROPOSED = 7, ROW_MISSED = 8,
                  ROW_WON = 9, ROW_WORDS = 10 };

struct View {                         // a slot of an instance's view table
    uint64_t round;
    uint32_t height, proposer;        // NONE: unattributed
    uint32_t start_frame, pp_frame;
    uint32_t won, outcome;
};
static_assert(sizeof(View) == 32, "table layout");
struct Record {                       // include/bftsim.h bftsim_rollcall_record
    uint64_t round;
    uint32_t inst, height, proposer, outcome, start_frame, pp_frame;
};
static_assert(sizeof(Record) == 32, "ABI layout");
struct Cand {                         // a candidate view
    uint64_t round;
    uint32_t height, start_frame;
    bool due;
};

// the frames that count, their height in range or not: accepted by the observer, any of the four codes
BFT_FN bool counts(uint32_t status, uint32_t code) {
    return (status == audit::ST_OK || status == audit::ST_SEAL_FOREIGN) && code >= 1u && code <= 4u;
}
BFT_FN uint32_t view_cap(uint32_t max_heights, uint32_t tl_cap) { return max_heights + tl_cap; }
// candidate j of an instance: below max_heights the view (j + 1, 0), due at height 1 or above a certificate; from there
// the chronicler's slot j - max_heights, due when it is a quorate RoundChange key of a round above 0. row0: the
// instance's first certificate row
BFT_FN Cand cand_of(const timeline::Certs& certs, uint64_t row0, uint32_t max_heights, const timeline::Key* keys, uint32_t j) {
    Cand c;
    if (j < max_heights) {
        c.height = j + 1u; c.round = 0;
        const bool first = j == 0;
        c.due = first || certs.round[row0 + j - 1u] != ROUND_NONE;
        c.start_frame = first || !c.due ? NONE : certs.frame[row0 + j - 1u];
        return c;
    }
    const timeline::Key& k = keys[j - max_heights];
    c.height = k.height; c.round = k.round; c.start_frame = k.qframe;
    c.due = k.code == (uint32_t)MT_ROUND_CHANGE && k.quorate != 0 && k.round != 0;
    return c;
}
BFT_FN bool view_less(uint32_t ha, uint64_t ra, uint32_t hb, uint64_t rb) { return ha < hb || (ha == hb && ra < rb); }
// (seed(parent) + round mod n) mod n, bftsim_calc_proposer's rule under the seed order
BFT_FN uint32_t proposer_of(const uint8_t* parent, uint64_t round, uint32_t n, bool seed_le) {
    return (uint32_t)(((uint64_t)seed_from_hash(parent, n, seed_le) + round % n) % n);
}
// the view of a due candidate. Its parent is the genesis hash at height 1, else the certificate digest of the height
// below; without that certificate the view stays unattributed
BFT_FN void view_put(View& v, const Cand& c, const timeline::Certs& certs, uint64_t row0, const uint8_t* genesis, uint32_t n,
                     bool seed_le) {
    v.round = c.round; v.height = c.height; v.start_frame = c.start_frame; v.pp_frame = NONE; v.won = 0; v.outcome = 0;
    const uint8_t* parent = genesis;
    if (c.height > 1u) {
        const uint64_t below = row0 + c.height - 2u;
        parent = certs.round[below] != ROUND_NONE ? certs.digest + 32 * below : nullptr;
    }
    v.proposer = parent ? proposer_of(parent, c.round, n, seed_le) : NONE;
}
// a counting PrePrepare (hx, round, signer) at frame rel of its instance against a view. wins: its digest is that of
// the certificate of hx, whose completing frame names this round. In frame order the first match sets pp_frame
BFT_FN void view_pp(View& v, uint32_t hx, uint64_t round, uint32_t signer, uint32_t rel, bool wins) {
    if (v.height != hx || v.round != round || v.proposer != signer) return;
    if (rel < v.pp_frame) v.pp_frame = rel;
    if (wins) v.won = 1;
}
BFT_FN uint32_t outcome_of(const View& v) {
    if (v.proposer == NONE) return OUT_UNATTRIBUTED;
    if (v.pp_frame == NONE) return OUT_MISSED;
    return OUT_PROPOSED | (v.won ? (uint32_t)OUT_WON : 0u);
}
// a counting frame into its signer's counters (row: ROW_WORDS words, zero before the instance). The last frame is kept
// as index + 1, so that the greatest wins and zero means none; row_last_frame turns it back
BFT_FN void row_frame(uint32_t* row, uint32_t code, uint32_t hx, uint32_t rel) {
    row[ROW_FRAMES + code - 1u] += 1u;
    if (hx > row[ROW_LAST_HEIGHT]) row[ROW_LAST_HEIGHT] = hx;
    if (rel + 1u > row[ROW_LAST_FRAME]) row[ROW_LAST_FRAME] = rel + 1u;
}
BFT_FN uint32_t row_last_frame(uint32_t kept) { return kept - 1u; }
// the counter of the proposer's row that an attributed view's outcome adds to, beside ROW_DUE (and ROW_WON if it won)
BFT_FN uint32_t row_of_outcome(uint32_t outcome) { return (outcome & 0xffu) == (uint32_t)OUT_PROPOSED ? (uint32_t)ROW_PROPOSED : (uint32_t)ROW_MISSED; }
BFT_FN Record record_of(const View& v, uint32_t inst) {
    return Record{v.round, inst, v.height, v.proposer, v.outcome, v.start_frame, v.pp_frame};
}

// ---------------------------------------------------------------- the GPU passes (kern_rollcall.hip)
struct Rows {                         // [inst * n] each
    uint32_t* frames;                 // x4
    uint32_t *last_height, *last_frame, *due, *proposed, *missed, *won;
};
struct Args {
    audit::Recs r;
    const uint8_t* status;            // [F]
    const int32_t* signer;            // [F]
    const uint64_t* inst_frame0;      // [inst + 1]
    uint64_t inst;
    uint32_t n, tl_cap, max_heights, seed_le;
    const uint8_t* genesis;           // 32
    timeline::Certs certs;
    const timeline::Key* keys;        // [inst][tl_cap], the chronicler's
    const uint32_t* inst_nkeys;       // [inst]
    const uint32_t* tl_flags;         // [inst]
    View* views;                      // [inst][max_heights + tl_cap]
    uint32_t* inst_views;             // [inst + 1], the last one zero: the scan's input
    uint32_t* pos;                    // [inst + 1], the scan's output
    Rows rows;
    uint64_t* inst_silent;            // [inst][4]
    uint32_t* inst_flags;             // [inst]
    Record* recs;                     // [rec_cap]
    uint64_t rec_cap;
    unsigned long long* counts;       // [CNT_WORDS]
};
#if defined(__HIPCC__)
hipError_t launch_views(const Args& a, hipStream_t s);
hipError_t launch_walk(const Args& a, hipStream_t s);
hipError_t launch_gather(const Args& a, hipStream_t s);
#endif

}  // namespace rollcall
}  // namespace bft
