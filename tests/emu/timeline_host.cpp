// timeline_host.cpp — TEST-ONLY host build of consensus-rs_amd/csrc/bft_timeline.h (the key table, the vote, the row
// writers and the flags the chronicler's kernels run, SPEC.md §11h), checked against tests/timeline_ref.py on the CPU.
// As a shared library (tests/timeline_lib.py) it runs behind the observer's host build (tests/audit_lib.py), over its
// records, statuses, signers and certificate rows; with -DTIMELINE_HOST_MAIN it is a stand-alone program for the
// sanitizers: it reads those arrays and the expected outputs from stdin into heap buffers of exactly the counted sizes,
// runs the same code and compares.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../consensus-rs_amd/csrc/bft_timeline.h"

using namespace bft;
using namespace bft::timeline;

extern "C" {

// the walk of every instance, then its rows. The rows' arrays hold inst * max_heights rows each; counts: CNT_WORDS words
void timeline_host(const uint8_t* code, const uint32_t* hx, const uint64_t* round, const uint8_t* digest,
                   const uint8_t* status, const int32_t* signer, const uint64_t* inst_frame0, uint64_t inst, uint32_t n,
                   uint32_t tl_cap, uint32_t max_heights, const uint16_t* cert_round, const uint8_t* cert_digest,
                   const uint32_t* cert_frame, uint16_t* prep_round, uint8_t* prep_digest, uint64_t* prep_voters,
                   uint32_t* prep_frame, uint16_t* prep_quorums, uint16_t* rc_quorums, uint16_t* rc_max_round,
                   uint32_t* rc_max_frame, uint16_t* rc_top_round, uint32_t* rc_frames, uint8_t* flags, uint32_t* inst_flags,
                   uint32_t* open_height, uint64_t* counts) {
    const Rows o{prep_round, prep_digest, prep_voters, prep_frame, prep_quorums, rc_quorums, rc_max_round, rc_max_frame,
                 rc_top_round, rc_frames, flags};
    const uint32_t H = max_heights, quorum = (2u * n) / 3u;
    for (uint32_t k = 0; k < CNT_WORDS; ++k) counts[k] = 0;
    for (uint64_t row = 0; row < inst * H; ++row) {
        prep_round[row] = rc_max_round[row] = rc_top_round[row] = (uint16_t)ROUND_NONE;
        prep_frame[row] = rc_max_frame[row] = rc_frames[row] = 0;
        prep_quorums[row] = rc_quorums[row] = 0;
        flags[row] = 0;
        memset(prep_digest + 32 * row, 0, 32);
        memset(prep_voters + 4 * row, 0, 32);
    }
    if (tl_cap == 0) tl_cap = default_cap(H);
    Key* keys = (Key*)malloc(sizeof(Key) * tl_cap);                   // exactly the table: a slot past it is caught
    for (uint64_t in = 0; in < inst; ++in) {
        const uint64_t f0 = inst_frame0[in], row0 = in * H;
        uint32_t nkeys = 0, fl = 0;
        for (uint64_t k = f0; k < inst_frame0[in + 1]; ++k) {
            if (!timeline::counts(status[k], code[k])) continue;
            if (hx[k] == 0) { counts[CNT_OUT_OF_RANGE] += 1; continue; }
            const bool prep = code[k] == (uint8_t)MT_PREPARE;
            counts[prep ? CNT_PREPARE_FRAMES : CNT_RC_FRAMES] += 1;
            if ((uint32_t)signer[k] >= n || (uint32_t)signer[k] > 255u) continue;
            const uint64_t* dig = (const uint64_t*)(digest + 32 * k);
            uint32_t slot = NONE;
            for (uint32_t s = 0; s < nkeys; ++s)
                if (key_is(keys[s], code[k], hx[k], round[k], dig)) slot = s;
            if (slot == NONE) {
                if (nkeys == tl_cap) { fl |= FLAG_KEY_OVERFLOW; continue; }
                slot = nkeys++;
                key_put(keys[slot], code[k], hx[k], round[k], dig);
            }
            Key& key = keys[slot];
            const uint32_t rel = (uint32_t)(k - f0);
            const uint64_t row = row0 + hx[k] - 1u;
            const bool crossed = key_vote(key, (uint32_t)signer[k], quorum, rel);
            if (prep) {
                if (crossed) row_prepare(o, row, round[k], dig, key.voters[0], key.voters[1], key.voters[2], key.voters[3], rel);
            } else {
                if (crossed) { row_rc_quorum(o, row, round[k], rel, round + f0); counts[CNT_RC_QUORUMS] += 1; }
                row_rc_frame(o, row, round[k]);
            }
        }
        inst_flags[in] = fl;
        counts[CNT_KEY_OVERFLOWS] += fl & FLAG_KEY_OVERFLOW ? 1 : 0;
        open_height[in] = H + 1u;
        for (uint32_t x = H; x >= 1; --x) {
            const uint64_t row = row0 + x - 1u;
            const bool has_cert = cert_round[row] != (uint16_t)ROUND_NONE, prepared = prep_quorums[row] != 0;
            const uint32_t cf = cert_frame[row];
            const uint32_t f = row_flags(keys, nkeys, x, prepared, has_cert, (const uint64_t*)(cert_digest + 32 * row),
                                         has_cert ? round[f0 + cf] : 0ull, cf);
            flags[row] = (uint8_t)f;
            if (!has_cert) open_height[in] = x;
            counts[CNT_PREPARED] += prepared ? 1 : 0;
            counts[CNT_RC_HEIGHTS] += rc_quorums[row] ? 1 : 0;
            counts[CNT_PREPARED_FIRST] += f & ROW_PREPARED_FIRST ? 1 : 0;
            counts[CNT_CERT_UNPREPARED] += f & ROW_CERT_UNPREPARED ? 1 : 0;
            counts[CNT_LOCKED_OPEN] += f & ROW_LOCKED_OPEN ? 1 : 0;
        }
    }
    free(keys);
}
}

#ifdef TIMELINE_HOST_MAIN
// stdin (little-endian): u64 frames, inst; u32 n, tl_cap, max_heights, pad; then the arrays code[F] hx[F] round[F]
// digest[F][32] status[F] signer[F] inst_frame0[inst + 1] cert_round[R] cert_digest[R][32] cert_frame[R], then the
// expected prep_round[R] prep_digest[R][32] prep_voters[R][4] prep_frame[R] prep_quorums[R] rc_quorums[R]
// rc_max_round[R] rc_max_frame[R] rc_top_round[R] rc_frames[R] flags[R] inst_flags[inst] open_height[inst]
// counts[CNT_WORDS], R = inst * max_heights
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
    uint64_t* hd = take<uint64_t>(2);
    uint32_t* hw = take<uint32_t>(4);
    const uint64_t F = hd[0], I = hd[1];
    const uint32_t n = hw[0], tl_cap = hw[1], H = hw[2];
    if (F > (1u << 24) || I > (1u << 20) || n < 1 || n > 256 || H < 1 || H > 65535) return 2;
    const uint64_t R = I * H;
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
    uint16_t* w_pr = take<uint16_t>(R); uint8_t* w_pd = take<uint8_t>(R * 32); uint64_t* w_pv = take<uint64_t>(R * 4);
    uint32_t* w_pf = take<uint32_t>(R); uint16_t* w_pq = take<uint16_t>(R); uint16_t* w_rq = take<uint16_t>(R);
    uint16_t* w_rm = take<uint16_t>(R); uint32_t* w_rmf = take<uint32_t>(R); uint16_t* w_rt = take<uint16_t>(R);
    uint32_t* w_rf = take<uint32_t>(R); uint8_t* w_fl = take<uint8_t>(R); uint32_t* w_if = take<uint32_t>(I);
    uint32_t* w_oh = take<uint32_t>(I); uint64_t* w_counts = take<uint64_t>(CNT_WORDS);
    uint16_t* pr = room<uint16_t>(R); uint8_t* pd = room<uint8_t>(R * 32); uint64_t* pv = room<uint64_t>(R * 4);
    uint32_t* pf = room<uint32_t>(R); uint16_t* pq = room<uint16_t>(R); uint16_t* rq = room<uint16_t>(R);
    uint16_t* rm = room<uint16_t>(R); uint32_t* rmf = room<uint32_t>(R); uint16_t* rt = room<uint16_t>(R);
    uint32_t* rf = room<uint32_t>(R); uint8_t* fl = room<uint8_t>(R); uint32_t* ifl = room<uint32_t>(I);
    uint32_t* oh = room<uint32_t>(I);
    uint64_t counts[CNT_WORDS];
    timeline_host(code, hx, round, digest, status, signer, if0, I, n, tl_cap, H, c_round, c_digest, c_frame, pr, pd, pv, pf, pq,
                  rq, rm, rmf, rt, rf, fl, ifl, oh, counts);
    same("prep_round", pr, w_pr, R); same("prep_digest", pd, w_pd, R * 32); same("prep_voters", pv, w_pv, R * 4);
    same("prep_frame", pf, w_pf, R); same("prep_quorums", pq, w_pq, R); same("rc_quorums", rq, w_rq, R);
    same("rc_max_round", rm, w_rm, R); same("rc_max_frame", rmf, w_rmf, R); same("rc_top_round", rt, w_rt, R);
    same("rc_frames", rf, w_rf, R); same("flags", fl, w_fl, R); same("inst_flags", ifl, w_if, I);
    same("open_height", oh, w_oh, I); same("counts", counts, w_counts, CNT_WORDS);
    if (rc == 0) printf("ok %llu frames %llu rows\n", (unsigned long long)F, (unsigned long long)R);
    void* all[] = {hd, hw, code, hx, round, digest, status, signer, if0, c_round, c_digest, c_frame, w_pr, w_pd, w_pv, w_pf,
                   w_pq, w_rq, w_rm, w_rmf, w_rt, w_rf, w_fl, w_if, w_oh, w_counts, pr, pd, pv, pf, pq, rq, rm, rmf, rt, rf, fl,
                   ifl, oh};
    for (void* p : all) free(p);
    return rc;
}
#endif
