// bftsim_observe.hip — the host code of libbftsim's trace analysers and of the ledger importer (include/bftsim.h): the
// observer (SPEC.md §11c), its continuations — archiver (§11e), accuser (§11g), chronicler (§11h), roll call (§11i) —
// with their entry points, and bftsim_verify_ledger (§11d). Cold paths on the owning types of bftsim_impl.h; their
// kernels are kern_audit / kern_archive / kern_accuse / kern_timeline / kern_rollcall / kern_ledger.hip.
//
// An analyser is one Cont: audit_device lays its piece out behind the observer's in one pool, runs its passes after
// the tally and lets it copy its results out after the observer's own. A new one costs a Cont and two entry points.
#include <hip/hip_runtime.h>

#include <stdlib.h>
#include <string.h>

#include <hipcub/hipcub.hpp>

#include <string>
#include <vector>

#include "bftsim_impl.h"
#include "bft_audit.h"
#include "bft_archive.h"
#include "bft_accuse.h"
#include "bft_timeline.h"
#include "bft_rollcall.h"
#include "bft_ledger.h"

namespace {
// a pool's layout: sized(b) is the offset of the next b bytes, each field rounded up to 32
struct Layout {
    uint64_t bytes = 0;
    uint64_t operator()(uint64_t b) { const uint64_t o = bytes; bytes += (b + 31) & ~31ull; return o; }
};
// the events round the phases of a call, within Events' capacity: start(k) makes k events and records the first,
// mark() the next; after a synchronise read(ms, n) gives the n times between neighbouring marks
struct Phases {
    Events ev;
    int n = 0;
    hipError_t start(int marks, hipStream_t s) {
        if (marks > Events::MAX) return hipErrorInvalidValue;
        if (hipError_t e = ev.create(marks); e != hipSuccess) return e;
        return mark(s);
    }
    hipError_t mark(hipStream_t s) { return n < Events::MAX ? hipEventRecord(ev[n++], s) : hipErrorInvalidValue; }
    hipError_t read(float* ms, int k) const {
        for (int j = 0; j < k; ++j)
            if (hipError_t e = hipEventElapsedTime(&ms[j], ev[j], ev[j + 1]); e != hipSuccess) return e;
        return hipSuccess;
    }
};
struct Back { void* dst; uint64_t off, b; };      // b bytes at p + off of a pool to the caller's dst
}  // namespace
// the copies back to the caller: null destinations (outputs not asked for) and empty ones are skipped
static int copy_back(bftsim* h, const uint8_t* p, std::initializer_list<Back> back, hipStream_t s) {
    for (const Back& k : back)
        if (k.dst && k.b) HIPCHECK(h, hipMemcpyAsync(k.dst, p + k.off, k.b, hipMemcpyDeviceToHost, s));
    return BFTSIM_OK;
}
// the same between two events, synchronised: *ms is the copies' device time
static int copy_back_timed(bftsim* h, const uint8_t* p, std::initializer_list<Back> back, hipStream_t s, float* ms) {
    Phases ph;
    HIPCHECK(h, ph.start(2, s));
    if (int rc = copy_back(h, p, back, s)) return rc;
    HIPCHECK(h, ph.mark(s));
    HIPCHECK(h, hipStreamSynchronize(s));
    HIPCHECK(h, ph.read(ms, 1));
    return BFTSIM_OK;
}

// libbftsig, opened as bftsim_set_crypto opens it; the observer needs no secrets
static int audit_sig(bftsim* h) {
    SigApi& a = sig_api();
    if (!a.ok) return fail(h, BFTSIM_EUNSUPPORTED, a.why);
    if (!h->sig && a.create(h->device, &h->sig) != 0) return fail(h, BFTSIM_EHIP, "bftsig_create failed");
    return BFTSIM_OK;
}

namespace {
// what the observer produced, on the device and alive while a continuation runs: it only reads them
struct Observed {
    const uint8_t* d_stream;          // frame k = d_stream[d_foff[k] - base, d_foff[k + 1] - base)
    const uint64_t* d_foff;
    uint64_t base, frames;
    bft::audit::Recs r;
    const uint8_t* d_status;
    const int32_t* d_signer;
    const uint64_t* d_if0;
    uint64_t inst;
    uint32_t max_heights;
    bft::archive::Certs certs;        // the certificate rows: round, digest, voters, frame
};
// a continuation of audit_device: an analyser run after the tally while the pool is alive. Its tables are one more
// piece of the pool, behind the observer's; the observer's two entry points pass none.
struct Cont {
    uint64_t bytes = 0;               // of its piece (layout)
    // its own refusals for these dimensions, then its piece's layout
    virtual int layout(bftsim* h, uint64_t frames, uint64_t inst, uint32_t max_heights) = 0;
    // its passes over its piece p, synchronised: nothing has reached the caller yet
    virtual int passes(bftsim* h, uint8_t* p, const Observed& o, hipStream_t s) = 0;
    // after the observer's own copies: its results to the caller, its report and its *_ms
    virtual int copy(bftsim* h, const uint8_t* p, const Observed& o, hipStream_t s) = 0;
};
}  // namespace
// a continuation's four phase times: the observer's passes, its own two, the observer's copies and its own
static void cont_ms(const bftsim* h, const float own[2], float copy_ms, float ms[4]) {
    ms[0] = h->audit_ms[0] + h->audit_ms[1] + h->audit_ms[2];
    ms[1] = own[0]; ms[2] = own[1]; ms[3] = h->audit_ms[3] + copy_ms;
}

// ---- the archiver (SPEC.md §11e): its tables and header slots
namespace {
struct ArchiveCont final : Cont {
    uint8_t* hdr;                     // the caller's
    uint64_t slot_bytes;
    uint32_t* hdr_len;
    const bftsim_archive_out* out;
    bftsim_archive_report* report;
    // the piece's layout: the device slot is the smallest the boundary admits
    uint64_t dslot, o_pick, o_hdr, o_len, o_status, o_pp, o_nv, o_nf, o_height, o_counts;
    unsigned long long counts[bft::archive::CNT_WORDS];
    float ms[2];                      // pick, emit + heights

    int layout(bftsim* h, uint64_t, uint64_t inst, uint32_t max_heights) override {
        namespace R = bft::archive;
        const uint64_t rows = inst * max_heights, Rx = rows ? rows : 1, Ix = inst ? inst : 1;
        if (rows >= (1ull << 31) - 1) return fail(h, BFTSIM_ENOMEM, "bftsim_archive: 2^31 header slots or more");
        dslot = bftsim_ledger_slot_bytes(h->cfg.n);
        Layout sized;
        o_pick = sized(Rx * R::pick_words(bftsim_two_thirds_majority(h->cfg.n)) * 4);
        o_hdr = sized(Rx * dslot);
        o_len = sized(Rx * 4); o_status = sized(Rx); o_pp = sized(Rx * 4); o_nv = sized(Rx * 2); o_nf = sized(Rx * 2);
        o_height = sized(Ix * 8); o_counts = sized(R::CNT_WORDS * 8);
        bytes = sized.bytes;
        return BFTSIM_OK;
    }
    int passes(bftsim* h, uint8_t* p, const Observed& o, hipStream_t s) override {
        namespace R = bft::archive;
        const R::Args a{o.d_stream, o.d_foff, o.base, o.frames, o.r, o.d_status, o.d_signer, o.d_if0, o.inst, o.max_heights,
                        bftsim_two_thirds_majority(h->cfg.n), o.certs, (uint32_t*)(p + o_pick), p + o_hdr, dslot,
                        (uint32_t*)(p + o_len), p + o_status, (uint32_t*)(p + o_pp), (uint16_t*)(p + o_nv),
                        (uint16_t*)(p + o_nf), (uint64_t*)(p + o_height), (unsigned long long*)(p + o_counts)};
        Phases ph;
        HIPCHECK(h, hipMemsetAsync(p + o_pick, 0xff, o_hdr - o_pick, s));             // NONE
        HIPCHECK(h, hipMemsetAsync(p + o_hdr, 0, bytes - o_hdr, s));                  // the slots' tails, the counters
        HIPCHECK(h, ph.start(3, s));
        HIPCHECK(h, R::launch_pick(a, s));
        HIPCHECK(h, ph.mark(s));
        HIPCHECK(h, R::launch_emit(a, s));
        HIPCHECK(h, R::launch_heights(a, s));
        HIPCHECK(h, ph.mark(s));
        HIPCHECK(h, hipMemcpyAsync(counts, p + o_counts, sizeof counts, hipMemcpyDeviceToHost, s));
        HIPCHECK(h, hipStreamSynchronize(s));
        HIPCHECK(h, ph.read(ms, 2));
        if (counts[R::CNT_ERR])        // a header above its slot, or an emit pass that disagrees with the pick pass
            return fail(h, BFTSIM_EHIP, "bftsim_archive: " + std::to_string(counts[R::CNT_ERR]) +
                                            " headers did not fit their slot or lost a picked frame");
        return BFTSIM_OK;
    }
    int copy(bftsim* h, const uint8_t* p, const Observed& o, hipStream_t s) override {
        namespace R = bft::archive;
        const uint64_t rows = o.inst * o.max_heights;
        Phases ph;
        HIPCHECK(h, ph.start(2, s));
        if (rows) {
            HIPCHECK(h, hipMemcpy2DAsync(hdr, slot_bytes, p + o_hdr, dslot, dslot, rows, hipMemcpyDeviceToHost, s));
            HIPCHECK(h, hipMemcpyAsync(hdr_len, p + o_len, rows * 4, hipMemcpyDeviceToHost, s));
        }
        if (out)
            if (int rc = copy_back(h, p, {{out->status, o_status, rows}, {out->pp_frame, o_pp, rows * 4},
                                          {out->n_votes, o_nv, rows * 2}, {out->archived_height, o_height, o.inst * 8}}, s))
                return rc;
        HIPCHECK(h, ph.mark(s));
        HIPCHECK(h, hipStreamSynchronize(s));
        float copy_ms = 0;
        HIPCHECK(h, ph.read(&copy_ms, 1));
        cont_ms(h, ms, copy_ms, h->archive_ms);
        bftsim_archive_report* rep = report;
        memset(rep, 0, sizeof *rep);
        rep->headers = counts[R::CNT_STATUS + R::AR_OK];
        for (int k = 0; k < 3; ++k) rep->by_status[k] = counts[R::CNT_STATUS + k];
        rep->votes = counts[R::CNT_VOTES];
        rep->foreign_seals = counts[R::CNT_FOREIGN];
        rep->archived_instances = counts[R::CNT_ARCHIVED];
        return BFTSIM_OK;
    }
};

// ---- the accuser (SPEC.md §11g): over the classify and tally passes' records, statuses and signers
struct AccuseCont final : Cont {
    uint32_t view_cap;
    const bftsim_accuse_out* out;     // the caller's
    bftsim_accuse_report* report;
    uint64_t rec_cap, o_views, o_first, o_pair, o_acc, o_flags, o_mark, o_pos, o_recs, o_counts, o_scan;
    size_t scan_bytes;
    unsigned long long counts[bft::accuse::CNT_WORDS];
    uint32_t total;                   // the scan's
    float ms[2];                      // walk, mark + scan + gather

    int layout(bftsim* h, uint64_t frames, uint64_t inst, uint32_t max_heights) override {
        namespace X = bft::accuse;
        const uint64_t Fx = frames ? frames : 1, Ix = inst ? inst : 1;
        if (view_cap == 0) view_cap = X::default_view_cap(max_heights);
        const uint64_t per_view = sizeof(X::View) + 12ull * h->cfg.n;
        if (view_cap > (1ull << 40) / per_view / Ix)
            return fail(h, BFTSIM_ENOMEM, "bftsim_accuse: view_cap x instances above 1 TiB of view tables");
        if (frames >= (1ull << 31) - 1) return fail(h, BFTSIM_ENOMEM, "bftsim_accuse: 2^31 frames or more");    // the scan's int
        rec_cap = out->records ? (out->rec_cap < frames ? out->rec_cap : frames) : 0;   // a frame closes one record at most
        Layout sized;
        o_views = sized(Ix * view_cap * sizeof(X::View));
        o_first = sized(Ix * view_cap * 12ull * h->cfg.n);
        o_pair = sized(Fx * 4);
        o_acc = sized(Ix * 32); o_flags = sized(Ix * 4);
        o_mark = sized((Fx + 1) * 4); o_pos = sized((Fx + 1) * 4);
        o_recs = sized((rec_cap ? rec_cap : 1) * sizeof(X::Record));
        o_counts = sized(X::CNT_WORDS * 8);
        scan_bytes = 0;
        HIPCHECK(h, hipcub::DeviceScan::ExclusiveSum(nullptr, scan_bytes, (uint32_t*)nullptr, (uint32_t*)nullptr, (int)(frames + 1)));
        o_scan = sized(scan_bytes ? scan_bytes : 1);
        bytes = sized.bytes;
        return BFTSIM_OK;
    }
    int passes(bftsim* h, uint8_t* p, const Observed& o, hipStream_t s) override {
        namespace X = bft::accuse;
        const X::Args a{o.r, o.d_status, o.d_signer, o.d_if0, o.frames, o.inst, h->cfg.n, view_cap, (X::View*)(p + o_views),
                        (uint32_t*)(p + o_first), (uint32_t*)(p + o_pair), (uint64_t*)(p + o_acc),
                        (uint32_t*)(p + o_flags), (uint32_t*)(p + o_mark), (uint32_t*)(p + o_pos),
                        (X::Record*)(p + o_recs), rec_cap, (unsigned long long*)(p + o_counts)};
        Phases ph;
        HIPCHECK(h, hipMemsetAsync(p + o_first, 0xff, o_acc - o_first, s));           // NONE: first and frame_pair
        HIPCHECK(h, hipMemsetAsync(p + o_acc, 0, o_mark - o_acc, s));                 // instances without a wave
        HIPCHECK(h, hipMemsetAsync(p + o_counts, 0, X::CNT_WORDS * 8, s));
        HIPCHECK(h, ph.start(3, s));
        HIPCHECK(h, X::launch_walk(a, s));
        HIPCHECK(h, ph.mark(s));
        HIPCHECK(h, X::launch_mark(a, s));
        HIPCHECK(h, hipcub::DeviceScan::ExclusiveSum(p + o_scan, scan_bytes, a.mark, a.pos, (int)(o.frames + 1), s));
        HIPCHECK(h, X::launch_gather(a, s));
        HIPCHECK(h, ph.mark(s));
        HIPCHECK(h, hipMemcpyAsync(counts, p + o_counts, sizeof counts, hipMemcpyDeviceToHost, s));
        HIPCHECK(h, hipMemcpyAsync(&total, a.pos + o.frames, 4, hipMemcpyDeviceToHost, s));
        HIPCHECK(h, hipStreamSynchronize(s));
        HIPCHECK(h, ph.read(ms, 2));
        if (total != counts[X::CNT_RECORDS])
            return fail(h, BFTSIM_EHIP, "bftsim_accuse: the scan's total disagrees with the walk's count");
        return BFTSIM_OK;
    }
    int copy(bftsim* h, const uint8_t* p, const Observed& o, hipStream_t s) override {
        namespace X = bft::accuse;
        const uint64_t written = total < rec_cap ? total : rec_cap;
        float copy_ms = 0;
        if (int rc = copy_back_timed(h, p, {{out->frame_pair, o_pair, o.frames * 4}, {out->inst_accused, o_acc, o.inst * 32},
                                            {out->inst_flags, o_flags, o.inst * 4},
                                            {out->records, o_recs, written * sizeof(X::Record)}}, s, &copy_ms))
            return rc;
        cont_ms(h, ms, copy_ms, h->accuse_ms);
        bftsim_accuse_report* rep = report;
        memset(rep, 0, sizeof *rep);
        rep->records = counts[X::CNT_RECORDS];
        for (int k = 0; k < 3; ++k) rep->by_code[k] = counts[X::CNT_CODE + k];
        rep->accused = counts[X::CNT_ACCUSED];
        rep->accused_instances = counts[X::CNT_INSTANCES];
        rep->view_overflows = counts[X::CNT_VIEW_OVERFLOWS];
        return BFTSIM_OK;
    }
};

// ---- the chronicler (SPEC.md §11h): over the records, statuses, signers and certificate rows
struct TimelineCont final : Cont {
    uint32_t tl_cap;
    const bftsim_timeline_out* out;   // the caller's
    bftsim_timeline_report* report;
    uint64_t o_keys, o_nkeys, o_flags, o_open, o_pround, o_rcmax, o_rctop, o_pdig, o_pvot, o_pframe, o_pq, o_rcq, o_rcmf,
        o_rcf, o_rflags, o_counts;
    unsigned long long counts[bft::timeline::CNT_WORDS];
    float ms[2];                      // walk, rows

    int layout(bftsim* h, uint64_t, uint64_t inst, uint32_t max_heights) override {
        namespace T = bft::timeline;
        const uint64_t rows = inst * max_heights, Rx = rows ? rows : 1, Ix = inst ? inst : 1;
        if (rows >= (1ull << 31) - 1) return fail(h, BFTSIM_ENOMEM, "bftsim_timeline: 2^31 rows or more");
        if (tl_cap == 0) tl_cap = T::default_cap(max_heights);
        if (tl_cap > (1ull << 40) / sizeof(T::Key) / Ix)
            return fail(h, BFTSIM_ENOMEM, "bftsim_timeline: tl_cap x instances above 1 TiB of key tables");
        Layout sized;
        o_keys = sized(Ix * tl_cap * sizeof(T::Key));
        o_nkeys = sized(Ix * 4); o_flags = sized(Ix * 4); o_open = sized(Ix * 4);
        o_pround = sized(Rx * 2); o_rcmax = sized(Rx * 2); o_rctop = sized(Rx * 2);                      // preset to ROUND_NONE
        o_pdig = sized(Rx * 32); o_pvot = sized(Rx * 32); o_pframe = sized(Rx * 4); o_pq = sized(Rx * 2);
        o_rcq = sized(Rx * 2); o_rcmf = sized(Rx * 4); o_rcf = sized(Rx * 4); o_rflags = sized(Rx);
        o_counts = sized(T::CNT_WORDS * 8);
        bytes = sized.bytes;
        return BFTSIM_OK;
    }
    int passes(bftsim* h, uint8_t* p, const Observed& o, hipStream_t s) override {
        namespace T = bft::timeline;
        const T::Rows rows{(uint16_t*)(p + o_pround), p + o_pdig, (uint64_t*)(p + o_pvot), (uint32_t*)(p + o_pframe),
                           (uint16_t*)(p + o_pq), (uint16_t*)(p + o_rcq), (uint16_t*)(p + o_rcmax),
                           (uint32_t*)(p + o_rcmf), (uint16_t*)(p + o_rctop), (uint32_t*)(p + o_rcf), p + o_rflags};
        const T::Args a{o.r, o.d_status, o.d_signer, o.d_if0, o.inst, h->cfg.n, tl_cap, o.max_heights,
                        bftsim_two_thirds_majority(h->cfg.n), T::Certs{o.certs.round, o.certs.digest, o.certs.frame},
                        (T::Key*)(p + o_keys), (uint32_t*)(p + o_nkeys), (uint32_t*)(p + o_flags),
                        (uint32_t*)(p + o_open), rows, (unsigned long long*)(p + o_counts)};
        Phases ph;
        HIPCHECK(h, hipMemsetAsync(p + o_nkeys, 0, o_pround - o_nkeys, s));
        HIPCHECK(h, hipMemsetAsync(p + o_pround, 0xff, o_pdig - o_pround, s));        // ROUND_NONE
        HIPCHECK(h, hipMemsetAsync(p + o_pdig, 0, bytes - o_pdig, s));                // the other rows, the counters
        HIPCHECK(h, ph.start(3, s));
        HIPCHECK(h, T::launch_walk(a, s));
        HIPCHECK(h, ph.mark(s));
        HIPCHECK(h, T::launch_rows(a, s));
        HIPCHECK(h, ph.mark(s));
        HIPCHECK(h, hipMemcpyAsync(counts, p + o_counts, sizeof counts, hipMemcpyDeviceToHost, s));
        HIPCHECK(h, hipStreamSynchronize(s));
        HIPCHECK(h, ph.read(ms, 2));
        return BFTSIM_OK;
    }
    // the results and the report to the caller, the four phase times to `times`: the timeline's entry points store
    // them as the last timeline call's, the roll call folds them into its own
    int copy_out(bftsim* h, const uint8_t* p, const Observed& ob, hipStream_t s, float times[4]) {
        namespace T = bft::timeline;
        const uint64_t rows = ob.inst * ob.max_heights, inst = ob.inst;
        const bftsim_timeline_out* o = out;
        float copy_ms = 0;
        if (int rc = copy_back_timed(h, p, {{o->prep_round, o_pround, rows * 2}, {o->prep_digest, o_pdig, rows * 32},
                                            {o->prep_voters, o_pvot, rows * 32}, {o->prep_frame, o_pframe, rows * 4},
                                            {o->prep_quorums, o_pq, rows * 2}, {o->rc_quorums, o_rcq, rows * 2},
                                            {o->rc_max_round, o_rcmax, rows * 2}, {o->rc_max_frame, o_rcmf, rows * 4},
                                            {o->rc_top_round, o_rctop, rows * 2}, {o->rc_frames, o_rcf, rows * 4},
                                            {o->flags, o_rflags, rows}, {o->inst_flags, o_flags, inst * 4},
                                            {o->open_height, o_open, inst * 4}}, s, &copy_ms))
            return rc;
        cont_ms(h, ms, copy_ms, times);
        bftsim_timeline_report* rep = report;
        memset(rep, 0, sizeof *rep);
        rep->prepare_frames = counts[T::CNT_PREPARE_FRAMES];
        rep->rc_frames = counts[T::CNT_RC_FRAMES];
        rep->out_of_range = counts[T::CNT_OUT_OF_RANGE];
        rep->prepared = counts[T::CNT_PREPARED];
        rep->rc_quorums = counts[T::CNT_RC_QUORUMS];
        rep->rc_heights = counts[T::CNT_RC_HEIGHTS];
        rep->prepared_first = counts[T::CNT_PREPARED_FIRST];
        rep->cert_unprepared = counts[T::CNT_CERT_UNPREPARED];
        rep->locked_open = counts[T::CNT_LOCKED_OPEN];
        rep->key_overflows = counts[T::CNT_KEY_OVERFLOWS];
        return BFTSIM_OK;
    }
    int copy(bftsim* h, const uint8_t* p, const Observed& o, hipStream_t s) override {
        return copy_out(h, p, o, s, h->timeline_ms);
    }
};

// ---- the roll call (SPEC.md §11i): the chronicler's piece first (its layout and passes), then its own passes over
// the chronicler's key tables, which it only reads
struct RollCont final : Cont {
    TimelineCont tc;                  // out and report: the caller's, or the stand-ins
    bftsim_timeline_out own_out;      // what the chronicler's piece writes when the caller takes none of it
    bftsim_timeline_report own_report;
    const bftsim_rollcall_out* out;   // the caller's
    bftsim_rollcall_report* report;
    uint64_t rec_cap, o_tl, o_views, o_nviews, o_pos, o_frames, o_lh, o_lf, o_due, o_prop, o_miss, o_won, o_silent, o_flags,
        o_recs, o_counts, o_scan;
    size_t scan_bytes;
    unsigned long long counts[bft::rollcall::CNT_WORDS];
    uint32_t total;                   // the scan's
    float ms[3];                      // views, walk, scan + gather

    int layout(bftsim* h, uint64_t frames, uint64_t inst, uint32_t max_heights) override {
        namespace R = bft::rollcall;
        if (int e = tc.layout(h, frames, inst, max_heights)) return e;
        const uint64_t Ix = inst ? inst : 1, rows = inst * h->cfg.n, Rx = rows ? rows : 1;
        const uint64_t vcap = R::view_cap(max_heights, tc.tl_cap);
        if (rows >= (1ull << 31) - 1) return fail(h, BFTSIM_ENOMEM, "bftsim_rollcall: 2^31 rows or more");
        if (vcap > (1ull << 40) / sizeof(R::View) / Ix)
            return fail(h, BFTSIM_ENOMEM, "bftsim_rollcall: views x instances above 1 TiB of view tables");
        const uint64_t most = Ix * vcap;                                               // every view of the call
        rec_cap = out->records ? (out->rec_cap < most ? out->rec_cap : most) : 0;
        Layout sized{tc.bytes};
        o_tl = 0;
        o_views = sized(most * sizeof(R::View));
        o_nviews = sized((inst + 1) * 4); o_pos = sized((inst + 1) * 4);
        o_frames = sized(Rx * 16); o_lh = sized(Rx * 4); o_lf = sized(Rx * 4); o_due = sized(Rx * 4);
        o_prop = sized(Rx * 4); o_miss = sized(Rx * 4); o_won = sized(Rx * 4);
        o_silent = sized(Ix * 32); o_flags = sized(Ix * 4);
        o_recs = sized((rec_cap ? rec_cap : 1) * sizeof(R::Record));
        o_counts = sized(R::CNT_WORDS * 8);
        scan_bytes = 0;
        HIPCHECK(h, hipcub::DeviceScan::ExclusiveSum(nullptr, scan_bytes, (uint32_t*)nullptr, (uint32_t*)nullptr, (int)(inst + 1)));
        o_scan = sized(scan_bytes ? scan_bytes : 1);
        bytes = sized.bytes;
        return BFTSIM_OK;
    }
    int passes(bftsim* h, uint8_t* p, const Observed& o, hipStream_t s) override {
        namespace R = bft::rollcall;
        if (int e = tc.passes(h, p + o_tl, o, s)) return e;
        const R::Rows rows{(uint32_t*)(p + o_frames), (uint32_t*)(p + o_lh), (uint32_t*)(p + o_lf), (uint32_t*)(p + o_due),
                           (uint32_t*)(p + o_prop), (uint32_t*)(p + o_miss), (uint32_t*)(p + o_won)};
        const R::Args a{o.r, o.d_status, o.d_signer, o.d_if0, o.inst, h->cfg.n, tc.tl_cap, o.max_heights,
                        h->cfg.seed_byte_order == BFTSIM_SEED_LE ? 1u : 0u, h->d_ghash,
                        bft::timeline::Certs{o.certs.round, o.certs.digest, o.certs.frame},
                        (const bft::timeline::Key*)(p + o_tl + tc.o_keys), (const uint32_t*)(p + o_tl + tc.o_nkeys),
                        (const uint32_t*)(p + o_tl + tc.o_flags), (R::View*)(p + o_views), (uint32_t*)(p + o_nviews),
                        (uint32_t*)(p + o_pos), rows, (uint64_t*)(p + o_silent), (uint32_t*)(p + o_flags),
                        (R::Record*)(p + o_recs), rec_cap, (unsigned long long*)(p + o_counts)};
        Phases ph;
        HIPCHECK(h, hipMemsetAsync(p + o_nviews, 0, o_recs - o_nviews, s));           // instances without a wave, the bitmaps' tails
        HIPCHECK(h, hipMemsetAsync(p + o_counts, 0, R::CNT_WORDS * 8, s));
        HIPCHECK(h, ph.start(4, s));
        HIPCHECK(h, R::launch_views(a, s));
        HIPCHECK(h, ph.mark(s));
        HIPCHECK(h, R::launch_walk(a, s));
        HIPCHECK(h, ph.mark(s));
        HIPCHECK(h, hipcub::DeviceScan::ExclusiveSum(p + o_scan, scan_bytes, a.inst_views, a.pos, (int)(o.inst + 1), s));
        HIPCHECK(h, R::launch_gather(a, s));
        HIPCHECK(h, ph.mark(s));
        HIPCHECK(h, hipMemcpyAsync(counts, p + o_counts, sizeof counts, hipMemcpyDeviceToHost, s));
        HIPCHECK(h, hipMemcpyAsync(&total, a.pos + o.inst, 4, hipMemcpyDeviceToHost, s));
        HIPCHECK(h, hipStreamSynchronize(s));
        HIPCHECK(h, ph.read(ms, 3));
        if (total != counts[R::CNT_VIEWS])
            return fail(h, BFTSIM_EHIP, "bftsim_rollcall: the scan's total disagrees with the walk's count");
        return BFTSIM_OK;
    }
    int copy(bftsim* h, const uint8_t* p, const Observed& ob, hipStream_t s) override {
        namespace R = bft::rollcall;
        float tl[4];                  // the chronicler's piece's times: the roll call's, not the last timeline call's
        if (int e = tc.copy_out(h, p + o_tl, ob, s, tl)) return e;
        const uint64_t inst = ob.inst, rows = inst * h->cfg.n, written = total < rec_cap ? total : rec_cap;
        const bftsim_rollcall_out* o = out;
        float copy_ms = 0;
        if (int rc = copy_back_timed(h, p, {{o->frames, o_frames, rows * 16}, {o->last_height, o_lh, rows * 4},
                                            {o->last_frame, o_lf, rows * 4}, {o->due, o_due, rows * 4},
                                            {o->proposed, o_prop, rows * 4}, {o->missed, o_miss, rows * 4},
                                            {o->won, o_won, rows * 4}, {o->inst_views, o_nviews, inst * 4},
                                            {o->inst_silent, o_silent, inst * 32}, {o->inst_flags, o_flags, inst * 4},
                                            {o->records, o_recs, written * sizeof(R::Record)}}, s, &copy_ms))
            return rc;
        h->rollcall_ms[0] = tl[0];
        h->rollcall_ms[1] = tl[1] + tl[2];
        for (int k = 0; k < 3; ++k) h->rollcall_ms[2 + k] = ms[k];
        h->rollcall_ms[5] = tl[3] + copy_ms;
        bftsim_rollcall_report* rep = report;
        memset(rep, 0, sizeof *rep);
        rep->frames = counts[R::CNT_FRAMES];
        rep->out_of_range = counts[R::CNT_OUT_OF_RANGE];
        rep->views = counts[R::CNT_VIEWS];
        for (int k = 0; k < 3; ++k) rep->by_outcome[k] = counts[R::CNT_OUTCOME + k];
        rep->won = counts[R::CNT_WON];
        rep->silent = counts[R::CNT_SILENT];
        rep->silent_instances = counts[R::CNT_SILENT_INST];
        rep->partial_instances = counts[R::CNT_PARTIAL_INST];
        return BFTSIM_OK;
    }
};
}  // namespace

// ---- the observer (SPEC.md §11c): decode, recoveries, classification and tally of a frame stream on the device
// the passes over a device stream: frame k = d_stream[d_foff[k] - base, d_foff[k + 1] - base), if0 on the host; then the
// continuation's, if any. report: null where a continuation's caller takes none. Every temporary is freed before
// returning; only the caller's buffers and the handle's *_ms are written.
static int audit_device(bftsim* h, const uint8_t* d_stream, const uint64_t* d_foff, uint64_t base, uint64_t frames,
                        const uint64_t* if0, uint64_t inst, uint32_t max_heights, uint32_t key_cap,
                        const bftsim_audit_out* out, bftsim_audit_report* report, hipStream_t s, float copy_in_ms,
                        Cont* cont = nullptr) {
    namespace A = bft::audit;
    SigApi& sa = sig_api();
    bftsim_audit_report own;
    if (!report) report = &own;
    if (key_cap == 0) key_cap = 4u * max_heights + 64u;
    const uint64_t F = frames, Fx = F ? F : 1, Ix = inst ? inst : 1, rows = inst * max_heights, Rx = rows ? rows : 1;
    if (key_cap > (1ull << 40) / sizeof(A::Key) / Ix)
        return fail(h, BFTSIM_ENOMEM, "bftsim_audit: key_cap x instances above 1 TiB of key tables");
    Layout sized;
    const uint64_t o_st = sized(Fx), o_code = sized(Fx), o_hx = sized(Fx * 4), o_round = sized(Fx * 8), o_dig = sized(Fx * 32),
                   o_sdig = sized(Fx * 32), o_sig = sized(Fx * 65), o_sk = sized(Fx * 4), o_want = sized(Fx * 4),
                   o_sldig = sized(Fx * 32), o_seal = sized(Fx * 65), o_raddr = sized(Fx * 20), o_rok = sized(Fx),
                   o_saddr = sized(Fx * 20), o_sok = sized(Fx), o_status = sized(Fx), o_signer = sized(Fx * 4),
                   o_if0 = sized((inst + 1) * 8), o_keys = sized(Ix * key_cap * sizeof(A::Key)), o_iflags = sized(Ix * 4),
                   o_cround = sized(Rx * 2), o_cdig = sized(Rx * 32), o_cvot = sized(Rx * 32), o_cframe = sized(Rx * 4),
                   o_cflags = sized(Rx), o_counts = sized(A::CNT_WORDS * 8), o_nseal = sized(4);
    const uint64_t o_cont = sized.bytes;                                           // the continuation's piece
    if (cont)
        if (int rc = cont->layout(h, F, inst, max_heights)) return rc;
    const uint64_t bytes = o_cont + (cont ? cont->bytes : 0);
    DevMem pool_mem;
    if (pool_mem.alloc(bytes) != hipSuccess)
        return fail(h, BFTSIM_ENOMEM, "bftsim_audit: " + std::to_string(bytes) + " bytes of device memory");
    uint8_t* pool = pool_mem.as<uint8_t>();
    A::Recs r{pool + o_st, pool + o_code, (uint32_t*)(pool + o_hx), (uint64_t*)(pool + o_round), pool + o_dig, pool + o_sdig,
              pool + o_sig, (uint32_t*)(pool + o_sk), (uint32_t*)(pool + o_want), pool + o_sldig, pool + o_seal};
    unsigned long long* d_counts = (unsigned long long*)(pool + o_counts);
    uint32_t* d_nseal = (uint32_t*)(pool + o_nseal);
    uint64_t* d_if0 = (uint64_t*)(pool + o_if0);
    uint8_t* d_status = pool + o_status;
    int32_t* d_signer = (int32_t*)(pool + o_signer);
    const Observed seen{d_stream, d_foff, base, F, r, d_status, d_signer, d_if0, inst, max_heights,
                        {(const uint16_t*)(pool + o_cround), pool + o_cdig, (const uint64_t*)(pool + o_cvot),
                         (const uint32_t*)(pool + o_cframe)}};
    Phases ph;
    HIPCHECK(h, hipMemcpyAsync(d_if0, if0, (inst + 1) * 8, hipMemcpyHostToDevice, s));
    HIPCHECK(h, hipMemsetAsync(d_counts, 0, A::CNT_WORDS * 8 + 4, s));            // the counters and n_seals
    HIPCHECK(h, hipMemsetAsync(pool + o_cround, 0xff, Rx * 2, s));                // ROUND_NONE
    HIPCHECK(h, hipMemsetAsync(pool + o_cdig, 0, o_counts - o_cdig, s));          // the other certificate rows
    HIPCHECK(h, hipMemsetAsync(pool + o_iflags, 0, Ix * 4, s));
    // decode
    uint32_t n_seals = 0;
    HIPCHECK(h, ph.start(5, s));
    HIPCHECK(h, A::launch_decode(A::DecodeArgs{d_stream, d_foff, base, F, h->d_addr, h->cfg.n,
                                               h->cfg.seed_byte_order == BFTSIM_SEED_LE ? 1u : 0u, max_heights, r, d_nseal}, s));
    HIPCHECK(h, ph.mark(s));
    HIPCHECK(h, hipMemcpyAsync(&n_seals, d_nseal, 4, hipMemcpyDeviceToHost, s));
    HIPCHECK(h, hipStreamSynchronize(s));
    // recoveries: every frame's signer, every decodable Commit's seal
    if (F && sa.recover(h->sig, r.sdig, r.sig, F, nullptr, pool + o_raddr, pool + o_rok, s) != 0)
        return fail(h, BFTSIM_EHIP, std::string("bftsig_recover: ") + sa.last_error(h->sig));
    if (n_seals && sa.recover(h->sig, r.seal_dig, r.seal, n_seals, nullptr, pool + o_saddr, pool + o_sok, s) != 0)
        return fail(h, BFTSIM_EHIP, std::string("bftsig_recover (seals): ") + sa.last_error(h->sig));
    HIPCHECK(h, ph.mark(s));
    // classification and tally
    HIPCHECK(h, A::launch_classify(A::ClassifyArgs{r, F, h->d_addr, h->cfg.n, pool + o_raddr, pool + o_rok, pool + o_saddr,
                                                   pool + o_sok, d_status, d_signer, d_counts}, s));
    HIPCHECK(h, A::launch_tally(A::TallyArgs{r, d_status, d_signer, d_if0, inst, (A::Key*)(pool + o_keys), key_cap, max_heights,
                                             bftsim_two_thirds_majority(h->cfg.n), (uint32_t*)(pool + o_iflags),
                                             (uint16_t*)(pool + o_cround), pool + o_cdig, (uint64_t*)(pool + o_cvot),
                                             (uint32_t*)(pool + o_cframe), pool + o_cflags, d_counts}, s));
    HIPCHECK(h, ph.mark(s));
    unsigned long long c[A::CNT_WORDS] = {0};
    HIPCHECK(h, hipMemcpyAsync(c, d_counts, sizeof c, hipMemcpyDeviceToHost, s));
    HIPCHECK(h, hipStreamSynchronize(s));
    if (cont)
        if (int rc = cont->passes(h, pool + o_cont, seen, s)) return rc;
    // every pass succeeded: only now the caller's buffers
    if (out)
        if (int rc = copy_back(h, pool, {{out->frame_status, o_status, F}, {out->frame_signer, o_signer, F * 4},
                                         {out->inst_flags, o_iflags, inst * 4}, {out->cert_round, o_cround, rows * 2},
                                         {out->cert_digest, o_cdig, rows * 32}, {out->cert_voters, o_cvot, rows * 32},
                                         {out->cert_frame, o_cframe, rows * 4}, {out->cert_flags, o_cflags, rows}}, s))
            return rc;
    HIPCHECK(h, ph.mark(s));
    HIPCHECK(h, hipStreamSynchronize(s));
    float ms[4] = {0, 0, 0, 0};
    HIPCHECK(h, ph.read(ms, 4));
    h->audit_ms[0] = ms[0]; h->audit_ms[1] = ms[1]; h->audit_ms[2] = ms[2]; h->audit_ms[3] = ms[3] + copy_in_ms;
    memset(report, 0, sizeof *report);
    report->frames = F;
    report->ok = c[A::CNT_STATUS + 0]; report->undecodable = c[A::CNT_STATUS + 1]; report->unrecoverable = c[A::CNT_STATUS + 2];
    report->not_validator = c[A::CNT_STATUS + 3]; report->seal_bad = c[A::CNT_STATUS + 4];
    report->seal_foreign = c[A::CNT_STATUS + 5];
    for (int k = 0; k < 4; ++k) report->by_code[k] = c[A::CNT_CODE + k];
    report->out_of_range = c[A::CNT_OUT_OF_RANGE];
    report->certified = c[A::CNT_CERTIFIED];
    report->conflicts = c[A::CNT_CONFLICTS];
    report->key_overflows = c[A::CNT_KEY_OVERFLOWS];
    report->recoveries = F + n_seals;
    return cont ? cont->copy(h, pool + o_cont, seen, s) : BFTSIM_OK;
}
static int audit_dims(bftsim* h, uint64_t frames, uint64_t inst, uint32_t max_heights, const char* what) {
    if (max_heights == 0 || max_heights > 65535u) return fail(h, BFTSIM_EINVAL, std::string(what) + ": max_heights outside 1..65535");
    if (frames >= (1ull << 32)) return fail(h, BFTSIM_EINVAL, std::string(what) + ": 2^32 frames or more");
    if (inst >= (1ull << 31)) return fail(h, BFTSIM_EINVAL, std::string(what) + ": 2^31 instances or more");
    return BFTSIM_OK;
}

// the observer over a host stream; cont: an analyser's continuation (none for bftsim_audit_trace)
static int audit_host_stream(bftsim* h, const uint8_t* stream, uint64_t stream_bytes, const uint64_t* frame_off, uint64_t frames,
                             const uint64_t* inst_frame0, uint64_t inst_count, uint32_t max_heights, uint32_t key_cap,
                             const bftsim_audit_out* out, bftsim_audit_report* report, Cont* cont = nullptr) {
    if (!frame_off || !inst_frame0 || (stream_bytes && !stream))
        return fail(h, BFTSIM_EINVAL, "bftsim_audit_trace: null stream, frame_off or inst_frame0");
    if (int rc = audit_dims(h, frames, inst_count, max_heights, "bftsim_audit_trace")) return rc;
    for (uint64_t k = 0; k < frames; ++k)
        if (frame_off[k] > frame_off[k + 1]) return fail(h, BFTSIM_EINVAL, "bftsim_audit_trace: frame_off decreases");
    if (frame_off[frames] != stream_bytes) return fail(h, BFTSIM_EINVAL, "bftsim_audit_trace: frame_off does not end at stream_bytes");
    for (uint64_t i = 0; i < inst_count; ++i)
        if (inst_frame0[i] > inst_frame0[i + 1]) return fail(h, BFTSIM_EINVAL, "bftsim_audit_trace: inst_frame0 decreases");
    if (inst_frame0[0] != 0 || inst_frame0[inst_count] != frames)
        return fail(h, BFTSIM_EINVAL, "bftsim_audit_trace: inst_frame0 does not run from 0 to frames");
    HIPCHECK(h, hipSetDevice(h->device));
    if (int rc = audit_sig(h)) return rc;
    hipStream_t s = h->last_stream;
    DevMem in_mem;
    const uint64_t sb = (stream_bytes + 15) & ~15ull;              // the frame offsets follow the padded stream
    if (in_mem.alloc(sb + 16 + (frames + 1) * 8) != hipSuccess)
        return fail(h, BFTSIM_ENOMEM, "bftsim_audit_trace: device memory for the stream");
    uint8_t* d_in = in_mem.as<uint8_t>();
    Phases ph;
    float copy_ms = 0;
    HIPCHECK(h, ph.start(2, s));
    if (stream_bytes) HIPCHECK(h, hipMemcpyAsync(d_in, stream, stream_bytes, hipMemcpyHostToDevice, s));
    HIPCHECK(h, hipMemcpyAsync(d_in + sb + 16, frame_off, (frames + 1) * 8, hipMemcpyHostToDevice, s));
    HIPCHECK(h, ph.mark(s));
    HIPCHECK(h, hipStreamSynchronize(s));
    HIPCHECK(h, ph.read(&copy_ms, 1));
    return audit_device(h, d_in, (const uint64_t*)(d_in + sb + 16), 0, frames, inst_frame0, inst_count, max_heights, key_cap,
                        out, report, s, copy_ms, cont);
}

// the observer over the kept trace of the last launch; cont as above
static int audit_kept_trace(bftsim* h, uint64_t inst_begin, uint64_t inst_count, uint32_t key_cap,
                            const bftsim_audit_out* out, bftsim_audit_report* report, Cont* cont = nullptr) {
    if (int rc = trace_ready(h, "bftsim_audit_last_trace")) return rc;
    const uint64_t n = h->trace_n;
    if (inst_begin > n || inst_count > n - inst_begin)
        return fail(h, BFTSIM_EINVAL, "bftsim_audit_last_trace: instances [" + std::to_string(inst_begin) + ", +" +
                                          std::to_string(inst_count) + ") outside the last launch of " + std::to_string(n));
    if (int rc = trace_size_pass(h)) return rc;
    const uint64_t m0 = h->trace_moff[inst_begin], m1 = h->trace_moff[inst_begin + inst_count];
    const uint64_t frames = m1 - m0, base = h->trace_ioff[inst_begin], bytes = h->trace_ioff[inst_begin + inst_count] - base;
    if (int rc = audit_dims(h, frames, inst_count, h->cfg.heights, "bftsim_audit_last_trace")) return rc;
    HIPCHECK(h, hipSetDevice(h->device));
    if (int rc = audit_sig(h)) return rc;
    hipStream_t s = h->last_stream;
    std::vector<uint64_t> if0(inst_count + 1);
    for (uint64_t i = 0; i <= inst_count; ++i) if0[i] = h->trace_moff[inst_begin + i] - m0;
    // the emit pass of bftsim_export_trace into a device stream that stays on the device
    DevMem d_out;
    if (d_out.alloc(((bytes + 15) & ~15ull) + 16) != hipSuccess)
        return fail(h, BFTSIM_ENOMEM, "bftsim_audit_last_trace: device memory for the stream");
    if (int rc = trace_emit(h, "bftsim_audit_last_trace", m0, m1, d_out.as<uint8_t>(), nullptr, nullptr)) return rc;
    return audit_device(h, d_out.as<uint8_t>(), h->d_tfoff + m0, base, frames, if0.data(), inst_count, h->cfg.heights,
                        key_cap, out, report, s, 0.f, cont);
}

// ---- the analysers' set-up, shared by an analyser's two entry points: its argument refusals (`what` names the entry
// point), then its continuation over the caller's buffers
static int archive_args(bftsim* h, ArchiveCont& ac, uint8_t* hdr, uint64_t slot_bytes, uint32_t* hdr_len,
                        const bftsim_archive_out* out, bftsim_archive_report* report, const char* what) {
    if (!hdr || !hdr_len) return fail(h, BFTSIM_EINVAL, std::string(what) + ": null hdr or hdr_len");
    if (slot_bytes < bftsim_ledger_slot_bytes(h->cfg.n)) return fail(h, BFTSIM_EINVAL, std::string(what) + ": slot_bytes too small");
    ac.hdr = hdr; ac.slot_bytes = slot_bytes; ac.hdr_len = hdr_len; ac.out = out; ac.report = report;
    return BFTSIM_OK;
}
static int accuse_args(bftsim* h, AccuseCont& xc, uint32_t view_cap, const bftsim_accuse_out* out, bftsim_accuse_report* report,
                       const char* what) {
    if (!out) return fail(h, BFTSIM_EINVAL, std::string(what) + ": null out");
    if (out->rec_cap && !out->records) return fail(h, BFTSIM_EINVAL, std::string(what) + ": rec_cap without records");
    xc.view_cap = view_cap; xc.out = out; xc.report = report;
    return BFTSIM_OK;
}
static int timeline_args(bftsim* h, TimelineCont& tc, uint32_t tl_cap, const bftsim_timeline_out* out,
                         bftsim_timeline_report* report, const char* what) {
    if (!out) return fail(h, BFTSIM_EINVAL, std::string(what) + ": null out");
    tc.tl_cap = tl_cap; tc.out = out; tc.report = report;
    return BFTSIM_OK;
}
static int rollcall_args(bftsim* h, RollCont& rc, uint32_t tl_cap, const bftsim_rollcall_out* out,
                         bftsim_rollcall_report* report, const bftsim_timeline_out* timeline_out,
                         bftsim_timeline_report* timeline_report, const char* what) {
    if (!out) return fail(h, BFTSIM_EINVAL, std::string(what) + ": null out");
    if (out->rec_cap && !out->records) return fail(h, BFTSIM_EINVAL, std::string(what) + ": rec_cap without records");
    if (h->cfg.n > 256u) return fail(h, BFTSIM_EINVAL, std::string(what) + ": more than 256 validators");
    rc.tc.tl_cap = tl_cap; rc.tc.out = timeline_out ? timeline_out : &rc.own_out;      // own_out: zeroed, it takes nothing
    rc.tc.report = timeline_report ? timeline_report : &rc.own_report;
    rc.out = out; rc.report = report;
    return BFTSIM_OK;
}

extern "C" {

int bftsim_audit_trace(bftsim_t* h, const uint8_t* stream, uint64_t stream_bytes, const uint64_t* frame_off, uint64_t frames,
                       const uint64_t* inst_frame0, uint64_t inst_count, uint32_t max_heights, uint32_t key_cap,
                       const bftsim_audit_out* out, bftsim_audit_report* report) {
    if (!h || !report) return BFTSIM_EINVAL;
    return audit_host_stream(h, stream, stream_bytes, frame_off, frames, inst_frame0, inst_count, max_heights, key_cap, out,
                             report);
}
int bftsim_audit_last_trace(bftsim_t* h, uint64_t inst_begin, uint64_t inst_count, uint32_t key_cap,
                            const bftsim_audit_out* out, bftsim_audit_report* report) {
    if (!h || !report) return BFTSIM_EINVAL;
    return audit_kept_trace(h, inst_begin, inst_count, key_cap, out, report);
}
int bftsim_audit_last_ms(bftsim_t* h, float* decode_ms, float* recover_ms, float* tally_ms, float* copy_ms) {
    return h ? last_ms(h->audit_ms, {decode_ms, recover_ms, tally_ms, copy_ms}) : BFTSIM_EINVAL;
}

// ---- the archiver's entry points (SPEC.md §11e): the observer's passes and refusals, then pick, emit and heights
int bftsim_archive_trace(bftsim_t* h, const uint8_t* stream, uint64_t stream_bytes, const uint64_t* frame_off, uint64_t frames,
                         const uint64_t* inst_frame0, uint64_t inst_count, uint32_t max_heights, uint32_t key_cap,
                         uint8_t* hdr, uint64_t slot_bytes, uint32_t* hdr_len, const bftsim_archive_out* out,
                         const bftsim_audit_out* audit_out, bftsim_audit_report* audit_report, bftsim_archive_report* report) {
    if (!h || !report) return BFTSIM_EINVAL;
    ArchiveCont ac{};
    if (int rc = archive_args(h, ac, hdr, slot_bytes, hdr_len, out, report, "bftsim_archive_trace")) return rc;
    return audit_host_stream(h, stream, stream_bytes, frame_off, frames, inst_frame0, inst_count, max_heights, key_cap,
                             audit_out, audit_report, &ac);
}
int bftsim_archive_last_trace(bftsim_t* h, uint64_t inst_begin, uint64_t inst_count, uint32_t key_cap, uint8_t* hdr,
                              uint64_t slot_bytes, uint32_t* hdr_len, const bftsim_archive_out* out,
                              const bftsim_audit_out* audit_out, bftsim_audit_report* audit_report,
                              bftsim_archive_report* report) {
    if (!h || !report) return BFTSIM_EINVAL;
    ArchiveCont ac{};
    if (int rc = archive_args(h, ac, hdr, slot_bytes, hdr_len, out, report, "bftsim_archive_last_trace")) return rc;
    return audit_kept_trace(h, inst_begin, inst_count, key_cap, audit_out, audit_report, &ac);
}
int bftsim_archive_last_ms(bftsim_t* h, float* audit_ms, float* pick_ms, float* emit_ms, float* copy_ms) {
    return h ? last_ms(h->archive_ms, {audit_ms, pick_ms, emit_ms, copy_ms}) : BFTSIM_EINVAL;
}

// ---- the accuser's entry points (SPEC.md §11g): the observer's passes and refusals, then walk, mark, scan and gather
int bftsim_accuse_trace(bftsim_t* h, const uint8_t* stream, uint64_t stream_bytes, const uint64_t* frame_off, uint64_t frames,
                        const uint64_t* inst_frame0, uint64_t inst_count, uint32_t max_heights, uint32_t key_cap,
                        uint32_t view_cap, const bftsim_accuse_out* out, const bftsim_audit_out* audit_out,
                        bftsim_audit_report* audit_report, bftsim_accuse_report* report) {
    if (!h || !report) return BFTSIM_EINVAL;
    AccuseCont xc{};
    if (int rc = accuse_args(h, xc, view_cap, out, report, "bftsim_accuse_trace")) return rc;
    return audit_host_stream(h, stream, stream_bytes, frame_off, frames, inst_frame0, inst_count, max_heights, key_cap,
                             audit_out, audit_report, &xc);
}
int bftsim_accuse_last_trace(bftsim_t* h, uint64_t inst_begin, uint64_t inst_count, uint32_t key_cap, uint32_t view_cap,
                             const bftsim_accuse_out* out, const bftsim_audit_out* audit_out,
                             bftsim_audit_report* audit_report, bftsim_accuse_report* report) {
    if (!h || !report) return BFTSIM_EINVAL;
    AccuseCont xc{};
    if (int rc = accuse_args(h, xc, view_cap, out, report, "bftsim_accuse_last_trace")) return rc;
    return audit_kept_trace(h, inst_begin, inst_count, key_cap, audit_out, audit_report, &xc);
}
int bftsim_accuse_last_ms(bftsim_t* h, float* audit_ms, float* walk_ms, float* compact_ms, float* copy_ms) {
    return h ? last_ms(h->accuse_ms, {audit_ms, walk_ms, compact_ms, copy_ms}) : BFTSIM_EINVAL;
}

// ---- the chronicler's entry points (SPEC.md §11h): the observer's passes and refusals, then walk and rows
int bftsim_timeline_trace(bftsim_t* h, const uint8_t* stream, uint64_t stream_bytes, const uint64_t* frame_off, uint64_t frames,
                          const uint64_t* inst_frame0, uint64_t inst_count, uint32_t max_heights, uint32_t key_cap,
                          uint32_t tl_cap, const bftsim_timeline_out* out, const bftsim_audit_out* audit_out,
                          bftsim_audit_report* audit_report, bftsim_timeline_report* report) {
    if (!h || !report) return BFTSIM_EINVAL;
    TimelineCont tc{};
    if (int rc = timeline_args(h, tc, tl_cap, out, report, "bftsim_timeline_trace")) return rc;
    return audit_host_stream(h, stream, stream_bytes, frame_off, frames, inst_frame0, inst_count, max_heights, key_cap,
                             audit_out, audit_report, &tc);
}
int bftsim_timeline_last_trace(bftsim_t* h, uint64_t inst_begin, uint64_t inst_count, uint32_t key_cap, uint32_t tl_cap,
                               const bftsim_timeline_out* out, const bftsim_audit_out* audit_out,
                               bftsim_audit_report* audit_report, bftsim_timeline_report* report) {
    if (!h || !report) return BFTSIM_EINVAL;
    TimelineCont tc{};
    if (int rc = timeline_args(h, tc, tl_cap, out, report, "bftsim_timeline_last_trace")) return rc;
    return audit_kept_trace(h, inst_begin, inst_count, key_cap, audit_out, audit_report, &tc);
}
int bftsim_timeline_last_ms(bftsim_t* h, float* audit_ms, float* walk_ms, float* rows_ms, float* copy_ms) {
    return h ? last_ms(h->timeline_ms, {audit_ms, walk_ms, rows_ms, copy_ms}) : BFTSIM_EINVAL;
}

// ---- the roll call's entry points (SPEC.md §11i): the observer's passes and refusals, the chronicler's walk and rows,
// then views, walk and gather
int bftsim_rollcall_trace(bftsim_t* h, const uint8_t* stream, uint64_t stream_bytes, const uint64_t* frame_off, uint64_t frames,
                          const uint64_t* inst_frame0, uint64_t inst_count, uint32_t max_heights, uint32_t key_cap,
                          uint32_t tl_cap, const bftsim_rollcall_out* out, bftsim_rollcall_report* report,
                          const bftsim_audit_out* audit_out, bftsim_audit_report* audit_report,
                          const bftsim_timeline_out* timeline_out, bftsim_timeline_report* timeline_report) {
    if (!h || !report) return BFTSIM_EINVAL;
    RollCont rc{};
    if (int e = rollcall_args(h, rc, tl_cap, out, report, timeline_out, timeline_report, "bftsim_rollcall_trace")) return e;
    return audit_host_stream(h, stream, stream_bytes, frame_off, frames, inst_frame0, inst_count, max_heights, key_cap,
                             audit_out, audit_report, &rc);
}
int bftsim_rollcall_last_trace(bftsim_t* h, uint64_t inst_begin, uint64_t inst_count, uint32_t key_cap, uint32_t tl_cap,
                               const bftsim_rollcall_out* out, bftsim_rollcall_report* report,
                               const bftsim_audit_out* audit_out, bftsim_audit_report* audit_report,
                               const bftsim_timeline_out* timeline_out, bftsim_timeline_report* timeline_report) {
    if (!h || !report) return BFTSIM_EINVAL;
    RollCont rc{};
    if (int e = rollcall_args(h, rc, tl_cap, out, report, timeline_out, timeline_report, "bftsim_rollcall_last_trace")) return e;
    return audit_kept_trace(h, inst_begin, inst_count, key_cap, audit_out, audit_report, &rc);
}
int bftsim_rollcall_last_ms(bftsim_t* h, float* audit_ms, float* timeline_ms, float* views_ms, float* walk_ms, float* gather_ms,
                            float* copy_ms) {
    return h ? last_ms(h->rollcall_ms, {audit_ms, timeline_ms, views_ms, walk_ms, gather_ms, copy_ms}) : BFTSIM_EINVAL;
}

// ---- the importer (SPEC.md §11d): every header of a ledger verified from its bytes on the device
// votes per header (average over the slots) from which the tally takes a wave per header instead of a lane. Measured
// at 3 votes a header (the lane mapping 2.8x faster) and at 43 (the wave mapping 8.6x faster); the
// crossover between them was not bisected, 16 is a quarter of a wave
static constexpr uint32_t LEDGER_WAVE_MIN_VOTES = 16;
int bftsim_set_ledger_votes(bftsim_t* h, uint32_t kind) {
    if (!h) return BFTSIM_EINVAL;
    if (kind != BFTSIM_VOTES_SIGNATURES && kind != BFTSIM_VOTES_SEALS)
        return fail(h, BFTSIM_EINVAL, "bftsim_set_ledger_votes: kind is neither BFTSIM_VOTES_SIGNATURES nor BFTSIM_VOTES_SEALS");
    h->ledger_votes = kind;
    return BFTSIM_OK;
}

int bftsim_verify_ledger(bftsim_t* h, const uint8_t* hdr, uint64_t slot_bytes, const uint32_t* hdr_len, uint64_t inst_count,
                         uint32_t max_heights, const bftsim_ledger_out* out, bftsim_ledger_report* report) {
    namespace L = bft::ledger;
    if (!h || !report) return BFTSIM_EINVAL;
    if (!hdr || !hdr_len) return fail(h, BFTSIM_EINVAL, "bftsim_verify_ledger: null hdr or hdr_len");
    if (max_heights == 0 || max_heights > 65535u) return fail(h, BFTSIM_EINVAL, "bftsim_verify_ledger: max_heights outside 1..65535");
    if (slot_bytes == 0) return fail(h, BFTSIM_EINVAL, "bftsim_verify_ledger: slot_bytes is 0");
    if (inst_count >= (1ull << 31)) return fail(h, BFTSIM_EINVAL, "bftsim_verify_ledger: 2^31 instances or more");
    const uint64_t slots = inst_count * max_heights, Sx = slots ? slots : 1, Ix = inst_count ? inst_count : 1;
    // the scan's item count is an int, and a vote's header index a uint32_t
    if (slots >= (1ull << 31) - 1) return fail(h, BFTSIM_ENOMEM, "bftsim_verify_ledger: 2^31 header slots or more");
    if (slot_bytes > (1ull << 40) / Sx) return fail(h, BFTSIM_ENOMEM, "bftsim_verify_ledger: above 1 TiB of header slots");
    HIPCHECK(h, hipSetDevice(h->device));
    if (int rc = audit_sig(h)) return rc;
    SigApi& sa = sig_api();
    hipStream_t s = h->last_stream;
    // the A/B switch of scripts/ledger_bench.py, read only under BFTSIM_TESTING=1: 1 lane per header, 2 wave per header
    uint32_t mapping = 0;
    if (const char* t = getenv("BFTSIM_TESTING"); t && strcmp(t, "1") == 0)
        if (const char* e = getenv("BFTSIM_LEDGER_TALLY")) mapping = (uint32_t)atoi(e);
    Layout sized;
    const uint64_t o_hdr = sized(Sx * slot_bytes), o_len = sized(Sx * 4), o_recs = sized(Sx * sizeof(L::Rec)),
                   o_vbase = sized((Sx + 1) * 8), o_voters = sized(Sx * 32), o_dup = sized(Sx * 4), o_bad = sized(Sx),
                   o_status = sized(Sx), o_bhash = sized(Sx * 32), o_nv = sized(Sx * 2), o_vh = sized(Ix * 8),
                   o_counts = sized(L::CNT_WORDS * 8);
    size_t tb = 0;
    HIPCHECK(h, hipcub::DeviceScan::ExclusiveSum(nullptr, tb, (unsigned long long*)nullptr, (unsigned long long*)nullptr,
                                                 (int)(slots + 1)));
    const uint64_t o_scan = sized(tb ? tb : 1);
    DevMem pool_mem;
    if (pool_mem.alloc(sized.bytes) != hipSuccess)
        return fail(h, BFTSIM_ENOMEM, "bftsim_verify_ledger: " + std::to_string(sized.bytes) + " bytes of device memory");
    uint8_t* pool = pool_mem.as<uint8_t>();
    L::Args a{};
    a.hdr = pool + o_hdr; a.hdr_len = (const uint32_t*)(pool + o_len); a.slot_bytes = slot_bytes; a.slots = slots;
    a.inst = (uint32_t)inst_count; a.H = max_heights; a.addresses = h->d_addr; a.n = h->cfg.n;
    a.quorum = bftsim_two_thirds_majority(h->cfg.n); a.block_period = h->cfg.block_period; a.genesis_hash = h->d_ghash;
    a.genesis_time = h->cfg.genesis_time; a.recs = (L::Rec*)(pool + o_recs); a.vbase = (unsigned long long*)(pool + o_vbase);
    a.voters = (uint64_t*)(pool + o_voters); a.dup = (uint32_t*)(pool + o_dup); a.bad = pool + o_bad;
    a.status = pool + o_status; a.bhash = pool + o_bhash; a.n_votes = (uint16_t*)(pool + o_nv);
    a.vheight = (uint64_t*)(pool + o_vh); a.counts = (unsigned long long*)(pool + o_counts);
    // two timers, 4 and 5 of Events' 6 marks: before the host's wait for the vote total (copy in | presets | decode +
    // scan) and after it (scatter | recoveries | tally + link | copies)
    Phases pre, post;
    HIPCHECK(h, pre.start(4, s));
    if (slots) {
        HIPCHECK(h, hipMemcpyAsync(pool + o_hdr, hdr, slots * slot_bytes, hipMemcpyHostToDevice, s));
        HIPCHECK(h, hipMemcpyAsync(pool + o_len, hdr_len, slots * 4, hipMemcpyHostToDevice, s));
    }
    HIPCHECK(h, pre.mark(s));
    HIPCHECK(h, hipMemsetAsync(a.counts, 0, L::CNT_WORDS * 8, s));
    HIPCHECK(h, hipMemsetAsync(a.vbase, 0, (Sx + 1) * 8, s));
    HIPCHECK(h, hipMemsetAsync(a.vheight, 0, Ix * 8, s));
    // decode, then the dense vote list: a scan of the headers' vote counts, a scatter
    unsigned long long V = 0;
    HIPCHECK(h, pre.mark(s));
    HIPCHECK(h, L::launch_decode(a, s));
    HIPCHECK(h, hipcub::DeviceScan::ExclusiveSum(pool + o_scan, tb, a.vbase, a.vbase, (int)(slots + 1), s));
    HIPCHECK(h, pre.mark(s));                  // the host's wait for the total and its allocation are not decode time
    HIPCHECK(h, hipMemcpyAsync(&V, a.vbase + slots, 8, hipMemcpyDeviceToHost, s));
    HIPCHECK(h, hipStreamSynchronize(s));
    if (V > slots * (uint64_t)L::MAX_VOTES) return fail(h, BFTSIM_EHIP, "bftsim_verify_ledger: the vote scan disagrees with the decode pass");
    const uint64_t Vx = V ? V : 1;
    Layout vsized;
    const uint64_t v_sig = vsized(Vx * 65), v_dig = vsized(Vx * 32), v_addr = vsized(Vx * 20), v_ok = vsized(Vx),
                   v_hdr = vsized(Vx * 4);
    DevMem vote_mem;
    if (vote_mem.alloc(vsized.bytes) != hipSuccess)
        return fail(h, BFTSIM_ENOMEM, "bftsim_verify_ledger: " + std::to_string(vsized.bytes) + " bytes of device memory for the votes");
    uint8_t* vp = vote_mem.as<uint8_t>();
    a.votes = V; a.vsig = vp + v_sig; a.vdig = vp + v_dig; a.vaddr = vp + v_addr; a.vok = vp + v_ok;
    a.vhdr = (uint32_t*)(vp + v_hdr);
    HIPCHECK(h, post.start(5, s));
    HIPCHECK(h, L::launch_scatter(a, s));
    HIPCHECK(h, post.mark(s));
    // recoveries: every vote over its header's seal digest
    if (V && sa.recover(h->sig, a.vdig, a.vsig, V, nullptr, a.vaddr, a.vok, s) != 0)
        return fail(h, BFTSIM_EHIP, std::string("bftsig_recover: ") + sa.last_error(h->sig));
    HIPCHECK(h, post.mark(s));
    // a lane per header below this many votes per header on average, a wave per header from there
    if (mapping != L::TALLY_LANE && mapping != L::TALLY_WAVE)
        mapping = V < slots * (uint64_t)LEDGER_WAVE_MIN_VOTES ? L::TALLY_LANE : L::TALLY_WAVE;
    HIPCHECK(h, L::launch_tally(a, mapping, s));
    HIPCHECK(h, L::launch_link(a, s));
    HIPCHECK(h, post.mark(s));
    unsigned long long c[L::CNT_WORDS] = {0};
    HIPCHECK(h, hipMemcpyAsync(c, a.counts, sizeof c, hipMemcpyDeviceToHost, s));
    HIPCHECK(h, hipStreamSynchronize(s));      // every pass succeeded: only now the caller's buffers
    if (out)
        if (int rc = copy_back(h, pool, {{out->status, o_status, slots}, {out->block_hash, o_bhash, slots * 32},
                                         {out->voters, o_voters, slots * 32}, {out->n_votes, o_nv, slots * 2},
                                         {out->verified_height, o_vh, inst_count * 8}}, s))
            return rc;
    HIPCHECK(h, post.mark(s));
    HIPCHECK(h, hipStreamSynchronize(s));
    float before[3], after[4];
    HIPCHECK(h, pre.read(before, 3));
    HIPCHECK(h, post.read(after, 4));
    // decode kernel + scan, then the scatter: device time on either side of the wait
    h->ledger_ms[0] = before[2] + after[0]; h->ledger_ms[1] = after[1]; h->ledger_ms[2] = after[2];
    h->ledger_ms[3] = after[3] + before[0];
    memset(report, 0, sizeof *report);
    report->headers = c[L::CNT_HEADERS];
    for (uint32_t k = 0; k < L::ST_COUNT; ++k) report->by_status[k] = c[L::CNT_STATUS + k];
    report->votes = V;
    report->recoveries = V;
    report->duplicate_votes = c[L::CNT_DUP];
    report->verified_instances = c[L::CNT_WHOLE];
    return BFTSIM_OK;
}

int bftsim_ledger_last_ms(bftsim_t* h, float* decode_ms, float* recover_ms, float* tally_ms, float* copy_ms) {
    return h ? last_ms(h->ledger_ms, {decode_ms, recover_ms, tally_ms, copy_ms}) : BFTSIM_EINVAL;
}

}  // extern "C"
