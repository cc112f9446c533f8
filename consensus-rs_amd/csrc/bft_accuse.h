// bft_accuse.h — the accuser of a trace (SPEC.md §11g): over the frames the observer accepts, the
// validators that signed two digests for one (code, height, round), each with the two frames that prove it. Shared by
// the host build (tests/emu/accuse_host.cpp) and the GPU kernels (kern_accuse.hip). It reads the observer's records
// (bft_audit.h: code, hx, round, digest), statuses and signers, and writes none of them.
//   walk     per instance, in frame order: a table of views (height, round) in insertion order, nothing evicted; per
//            view a direct-addressed `first[3][N]`: the group's first frame, NONE before it, DONE once the group has
//            its record. A frame of a group whose digest differs from its first frame's closes the group.
//   compact  the frames with a pair, in frame order, as 32-byte records.
#pragma once
#include "bft_audit.h"

namespace bft {
namespace accuse {

using audit::NONE;
constexpr uint32_t DONE = 0xfffffffeu;            // first[]: the group has its record (no frame index reaches it:
                                                  // a first frame that is compared again has one behind it)
enum : uint32_t { FLAG_VIEW_OVERFLOW = 1 };       // include/bftsim.h BFTSIM_ACCUSE_VIEW_OVERFLOW
enum : uint32_t { CNT_RECORDS = 0, CNT_CODE = 1, CNT_ACCUSED = 4, CNT_INSTANCES = 5, CNT_VIEW_OVERFLOWS = 6, CNT_WORDS = 8 };

struct View {
    uint64_t round;
    uint32_t height, pad;
};
struct Record {                                   // include/bftsim.h bftsim_accuse_record
    uint64_t round;
    uint32_t inst, height, signer, code, frame_a, frame_b;
};
static_assert(sizeof(View) == 16 && sizeof(Record) == 32, "table and record layout");

BFT_FN uint32_t default_view_cap(uint32_t max_heights) { return 2u * max_heights + 64u; }
// the frames that count: accepted by the observer, PrePrepare / Prepare / Commit, height in 1..max_heights
BFT_FN bool counts(uint32_t status, uint32_t code, uint32_t hx) {
    return (status == audit::ST_OK || status == audit::ST_SEAL_FOREIGN) && code >= 1u && code <= 3u && hx != 0u;
}
BFT_FN bool view_is(const View& v, uint32_t hx, uint64_t round) { return v.height == hx && v.round == round; }
BFT_FN void view_put(View& v, uint32_t hx, uint64_t round) { v.round = round; v.height = hx; v.pad = 0; }
// the group's cell within its view's first[3][n]
BFT_FN uint64_t cell(uint32_t slot, uint32_t code, uint32_t signer, uint32_t n) { return ((uint64_t)slot * 3u + (code - 1u)) * n + signer; }
// frame `rel` (index within the instance, `k` within the call) into its group's cell. Returns the group's first frame
// (within the instance) when this frame closes the group, else NONE. digest: the records' [F][32], 8-byte aligned.
BFT_FN uint32_t group_step(uint32_t* first, uint32_t rel, uint64_t k, const uint8_t* digest) {
    const uint32_t a = *first;
    if (a == NONE) { *first = rel; return NONE; }
    if (a == DONE) return NONE;
    const uint64_t* da = (const uint64_t*)(digest + 32 * (k - rel + a));
    const uint64_t* db = (const uint64_t*)(digest + 32 * k);
    if (audit::same_digest(da, db)) return NONE;
    *first = DONE;
    return a;
}
// the instance of frame k: the last i with inst_frame0[i] <= k (instances without frames are passed over)
BFT_FN uint64_t inst_of(const uint64_t* inst_frame0, uint64_t inst, uint64_t k) {
    uint64_t lo = 0, hi = inst;                   // inst_frame0[lo] <= k < inst_frame0[hi]
    while (hi - lo > 1) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (inst_frame0[mid] <= k) lo = mid; else hi = mid;
    }
    return lo;
}
BFT_FN void record_put(Record& r, const audit::Recs& recs, const int32_t* signer, uint64_t inst, uint32_t frame_a, uint64_t k) {
    r.round = recs.round[k]; r.inst = (uint32_t)inst; r.height = recs.hx[k]; r.signer = (uint32_t)signer[k];
    r.code = recs.code[k]; r.frame_a = frame_a; r.frame_b = (uint32_t)k;
}

// ---------------------------------------------------------------- the GPU passes (kern_accuse.hip)
struct Args {
    audit::Recs r;
    const uint8_t* status;            // [F]
    const int32_t* signer;            // [F]
    const uint64_t* inst_frame0;      // [inst + 1]
    uint64_t frames, inst;
    uint32_t n, view_cap;
    View* views;                      // [inst][view_cap]
    uint32_t* first;                  // [inst][view_cap][3][n], preset to NONE
    uint32_t* frame_pair;             // [F] preset to NONE; frame_a of the record whose frame_b this frame is (both
                                      // within the call)
    uint64_t* inst_accused;           // [inst][4]
    uint32_t* inst_flags;             // [inst]
    uint32_t* mark;                   // [F + 1]
    uint32_t* pos;                    // [F + 1] the exclusive scan of mark
    Record* records;                  // [rec_cap]
    uint64_t rec_cap;
    unsigned long long* counts;       // [CNT_WORDS]
};
#if defined(__HIPCC__)
hipError_t launch_walk(const Args& a, hipStream_t s);
hipError_t launch_mark(const Args& a, hipStream_t s);
hipError_t launch_gather(const Args& a, hipStream_t s);
#endif

}  // namespace accuse
}  // namespace bft
