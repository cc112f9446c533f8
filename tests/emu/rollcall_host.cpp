// rollcall_host.cpp — TEST-ONLY host build of consensus-rs_amd/csrc/bft_rollcall.h (the candidates, the view slot, the
// proposer, the PrePrepare match, the outcome and the row update the roll call's kernels run, SPEC.md §11i), checked
// against tests/rollcall_ref.py on the CPU. As a shared library (tests/rollcall_lib.py) it runs behind the observer's
// host build (tests/audit_lib.py), over its records, statuses, signers and certificate rows; the chronicler's key table
// it reads is built here by bft_timeline.h's own functions, as tests/emu/timeline_host.cpp builds it. With
// -DROLLCALL_HOST_MAIN it is a stand-alone program for the sanitizers: it reads those arrays and the expected outputs
// from stdin into heap buffers of exactly the counted sizes, runs the same code and compares.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../consensus-rs_amd/csrc/bft_rollcall.h"

using namespace bft;
using namespace bft::rollcall;

// the chronicler's walk of one instance into keys[tl_cap] (tests/emu/timeline_host.cpp, without the rows) -> the
// number of keys; *overflow: a key found the table full
static uint32_t walk_keys(const uint8_t* code, const uint32_t* hx, const uint64_t* round, const uint8_t* digest,
                          const uint8_t* status, const int32_t* signer, uint64_t f0, uint64_t f1, uint32_t n, uint32_t tl_cap,
                          timeline::Key* keys, bool* overflow) {
    const uint32_t quorum = (2u * n) / 3u;
    uint32_t nkeys = 0;
    *overflow = false;
    for (uint64_t k = f0; k < f1; ++k) {
        if (!timeline::counts(status[k], code[k]) || hx[k] == 0) continue;
        if ((uint32_t)signer[k] >= n || (uint32_t)signer[k] > 255u) continue;
        const uint64_t* dig = (const uint64_t*)(digest + 32 * k);
        uint32_t slot = NONE;
        for (uint32_t s = 0; s < nkeys; ++s)
            if (timeline::key_is(keys[s], code[k], hx[k], round[k], dig)) slot = s;
        if (slot == NONE) {
            if (nkeys == tl_cap) { *overflow = true; continue; }
            slot = nkeys++;
            timeline::key_put(keys[slot], code[k], hx[k], round[k], dig);
        }
        timeline::key_vote(keys[slot], (uint32_t)signer[k], quorum, (uint32_t)(k - f0));
    }
    return nkeys;
}

extern "C" {

// rows: inst * n each (frames x4); inst_silent inst * 4; records: rec_cap of them; counts: CNT_WORDS words
void rollcall_host(const uint8_t* code, const uint32_t* hx, const uint64_t* round, const uint8_t* digest,
                   const uint8_t* status, const int32_t* signer, const uint64_t* inst_frame0, uint64_t inst, uint32_t n,
                   uint32_t tl_cap, uint32_t max_heights, uint32_t seed_le, const uint8_t* genesis, const uint16_t* cert_round,
                   const uint8_t* cert_digest, const uint32_t* cert_frame, uint32_t* frames, uint32_t* last_height,
                   uint32_t* last_frame, uint32_t* due, uint32_t* proposed, uint32_t* missed, uint32_t* won,
                   uint32_t* inst_views, uint64_t* inst_silent, uint32_t* inst_flags, Record* records, uint64_t rec_cap,
                   uint64_t* counts) {
    const uint32_t H = max_heights;
    const timeline::Certs certs{cert_round, cert_digest, cert_frame};
    for (uint32_t k = 0; k < CNT_WORDS; ++k) counts[k] = 0;
    if (tl_cap == 0) tl_cap = timeline::default_cap(H);
    timeline::Key* keys = (timeline::Key*)malloc(sizeof(timeline::Key) * (tl_cap ? tl_cap : 1));   // exactly the table
    View* views = (View*)malloc(sizeof(View) * view_cap(H, tl_cap));                                 // exactly the slots
    uint32_t* rows = (uint32_t*)malloc(sizeof(uint32_t) * ROW_WORDS * n);
    uint64_t at = 0;
    for (uint64_t in = 0; in < inst; ++in) {
        const uint64_t f0 = inst_frame0[in], f1 = inst_frame0[in + 1], row0 = in * H;
        bool over = false;
        const uint32_t nkeys = walk_keys(code, hx, round, digest, status, signer, f0, f1, n, tl_cap, keys, &over);
        // views
        const uint32_t cands = H + nkeys;
        uint32_t nviews = 0;
        for (uint32_t j = 0; j < cands; ++j) {
            const Cand c = cand_of(certs, row0, H, keys, j);
            if (!c.due) continue;
            uint32_t rank = 0;
            for (uint32_t q = 0; q < cands; ++q) {
                const Cand o = cand_of(certs, row0, H, keys, q);
                rank += o.due && view_less(o.height, o.round, c.height, c.round) ? 1u : 0u;
            }
            view_put(views[rank], c, certs, row0, genesis, n, seed_le != 0);
            nviews += 1;
        }
        // walk
        memset(rows, 0, sizeof(uint32_t) * ROW_WORDS * n);
        for (uint64_t k = f0; k < f1; ++k) {
            const uint32_t sg = (uint32_t)signer[k];
            if (!rollcall::counts(status[k], code[k]) || sg >= n || sg > 255u) continue;
            if (hx[k] == 0) { counts[CNT_OUT_OF_RANGE] += 1; continue; }
            const uint32_t rel = (uint32_t)(k - f0);
            counts[CNT_FRAMES] += 1;
            row_frame(rows + ROW_WORDS * sg, code[k], hx[k], rel);
            if (code[k] != (uint8_t)MT_PREPREPARE) continue;
            const uint64_t crow = row0 + hx[k] - 1u;
            bool wins = false;
            if (cert_round[crow] != (uint16_t)ROUND_NONE)
                wins = round[f0 + cert_frame[crow]] == round[k] &&
                       audit::same_digest((const uint64_t*)(digest + 32 * k), (const uint64_t*)(cert_digest + 32 * crow));
            for (uint32_t s = 0; s < nviews; ++s) view_pp(views[s], hx[k], round[k], sg, rel, wins);
        }
        // fold
        for (uint32_t s = 0; s < nviews; ++s) {
            View& v = views[s];
            v.outcome = outcome_of(v);
            counts[CNT_OUTCOME + (v.outcome & 0xffu) - 1u] += 1;
            counts[CNT_WON] += v.outcome & OUT_WON ? 1 : 0;
            if (v.proposer < n) {
                uint32_t* r = rows + ROW_WORDS * v.proposer;
                r[ROW_DUE] += 1; r[row_of_outcome(v.outcome)] += 1;
                if (v.outcome & OUT_WON) r[ROW_WON] += 1;
            }
            if (at < rec_cap) records[at] = record_of(v, (uint32_t)in);
            at += 1;
        }
        counts[CNT_VIEWS] += nviews;
        inst_views[in] = nviews;
        inst_flags[in] = over ? (uint32_t)FLAG_PARTIAL : 0u;
        counts[CNT_PARTIAL_INST] += over ? 1 : 0;
        uint32_t silent = 0;
        for (int w = 0; w < 4; ++w) inst_silent[4 * in + w] = 0;
        for (uint32_t v = 0; v < n; ++v) {
            const uint32_t* r = rows + ROW_WORDS * v;
            const uint64_t idx = in * n + v;
            uint32_t all = 0;
            for (int c = 0; c < 4; ++c) { frames[4 * idx + c] = r[ROW_FRAMES + c]; all += r[ROW_FRAMES + c]; }
            last_height[idx] = r[ROW_LAST_HEIGHT]; last_frame[idx] = row_last_frame(r[ROW_LAST_FRAME]);
            due[idx] = r[ROW_DUE]; proposed[idx] = r[ROW_PROPOSED]; missed[idx] = r[ROW_MISSED]; won[idx] = r[ROW_WON];
            if (all == 0) { inst_silent[4 * in + (v >> 6)] |= 1ull << (v & 63u); silent += 1; }
        }
        counts[CNT_SILENT] += silent;
        counts[CNT_SILENT_INST] += silent ? 1 : 0;
    }
    free(rows); free(views); free(keys);
}
}

#ifdef ROLLCALL_HOST_MAIN
// stdin (little-endian): u64 frames, inst, rec_cap; u32 n, tl_cap, max_heights, seed_le; genesis[32]; then the arrays
// code[F] hx[F] round[F] digest[F][32] status[F] signer[F] inst_frame0[inst + 1] cert_round[R] cert_digest[R][32]
// cert_frame[R], R = inst * max_heights; then the expected frames[V][4] last_height[V] last_frame[V] due[V] proposed[V]
// missed[V] won[V], V = inst * n, inst_views[inst] inst_silent[inst][4] inst_flags[inst] records[rec_cap]
// counts[CNT_WORDS]
template <class T> static T* take(uint64_t count) {
    T* p = (T*)malloc(count ? count * sizeof(T) : 1);                 // exactly the counted size
    if (count && fread(p, sizeof(T), count, stdin) != count) exit(2);
    return p;
}
template <class T> static T* room(uint64_t count) { return (T*)malloc(count ? count * sizeof(T) : 1); }
static int rc = 0;
template <class T> static void same(const char* what, const T* got, const T* want, uint64_t count) {
    if (count && memcmp(got, want, count * sizeof(T))) { printf("%s differs\n", what); rc = 1; }
}
int main() {
    uint64_t* hd = take<uint64_t>(3);
    uint32_t* hw = take<uint32_t>(4);
    uint8_t* genesis = take<uint8_t>(32);
    const uint64_t F = hd[0], I = hd[1], C = hd[2];
    const uint32_t n = hw[0], tl_cap = hw[1], H = hw[2], seed_le = hw[3];
    if (F > (1u << 24) || I > (1u << 20) || C > (1u << 24) || n < 1 || n > 256 || H < 1 || H > 65535 || tl_cap > (1u << 20)) return 2;
    const uint64_t R = I * H, V = I * n;
    uint8_t* code = take<uint8_t>(F);
    uint32_t* hx = take<uint32_t>(F);
    uint64_t* round = take<uint64_t>(F);
    uint8_t* digest = take<uint8_t>(F * 32);
    uint8_t* status = take<uint8_t>(F);
    int32_t* signer = take<int32_t>(F);
    uint64_t* if0 = take<uint64_t>(I + 1);
    uint16_t* c_round = take<uint16_t>(R);
    uint8_t* c_digest = take<uint8_t>(R * 32);
    uint32_t* c_frame = take<uint32_t>(R);
    uint32_t* w_fr = take<uint32_t>(V * 4); uint32_t* w_lh = take<uint32_t>(V); uint32_t* w_lf = take<uint32_t>(V);
    uint32_t* w_due = take<uint32_t>(V); uint32_t* w_pr = take<uint32_t>(V); uint32_t* w_mi = take<uint32_t>(V);
    uint32_t* w_won = take<uint32_t>(V); uint32_t* w_iv = take<uint32_t>(I); uint64_t* w_si = take<uint64_t>(I * 4);
    uint32_t* w_if = take<uint32_t>(I); Record* w_rec = take<Record>(C); uint64_t* w_counts = take<uint64_t>(CNT_WORDS);
    uint32_t* fr = room<uint32_t>(V * 4); uint32_t* lh = room<uint32_t>(V); uint32_t* lf = room<uint32_t>(V);
    uint32_t* du = room<uint32_t>(V); uint32_t* pr = room<uint32_t>(V); uint32_t* mi = room<uint32_t>(V);
    uint32_t* wo = room<uint32_t>(V); uint32_t* iv = room<uint32_t>(I); uint64_t* si = room<uint64_t>(I * 4);
    uint32_t* ifl = room<uint32_t>(I); Record* rec = room<Record>(C);
    uint64_t counts[CNT_WORDS];
    rollcall_host(code, hx, round, digest, status, signer, if0, I, n, tl_cap, H, seed_le, genesis, c_round, c_digest, c_frame,
                  fr, lh, lf, du, pr, mi, wo, iv, si, ifl, rec, C, counts);
    const uint64_t kept = counts[CNT_VIEWS] < C ? counts[CNT_VIEWS] : C;
    same("frames", fr, w_fr, V * 4); same("last_height", lh, w_lh, V); same("last_frame", lf, w_lf, V);
    same("due", du, w_due, V); same("proposed", pr, w_pr, V); same("missed", mi, w_mi, V); same("won", wo, w_won, V);
    same("inst_views", iv, w_iv, I); same("inst_silent", si, w_si, I * 4); same("inst_flags", ifl, w_if, I);
    same("records", rec, w_rec, kept); same("counts", counts, w_counts, CNT_WORDS);
    if (rc == 0) printf("ok %llu frames %llu views\n", (unsigned long long)F, (unsigned long long)counts[CNT_VIEWS]);
    void* all[] = {hd, hw, genesis, code, hx, round, digest, status, signer, if0, c_round, c_digest, c_frame, w_fr, w_lh, w_lf,
                   w_due, w_pr, w_mi, w_won, w_iv, w_si, w_if, w_rec, w_counts, fr, lh, lf, du, pr, mi, wo, iv, si, ifl, rec};
    for (void* p : all) free(p);
    return rc;
}
#endif
