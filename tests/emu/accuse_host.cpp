// accuse_host.cpp — TEST-ONLY host build of consensus-rs_amd/csrc/bft_accuse.h (the view table, the group step and the
// record the accuser's kernels run, SPEC.md §11g), checked against tests/accuse_ref.py on the CPU. As a shared library
// (tests/accuse_lib.py) it runs behind the observer's host build (tests/audit_lib.py), over its records, statuses and
// signers; with -DACCUSE_HOST_MAIN it is a stand-alone program for the sanitizers: it reads those arrays and the
// expected outputs from stdin into heap buffers of exactly the counted sizes, runs the same code and compares.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../consensus-rs_amd/csrc/bft_accuse.h"

using namespace bft;
using namespace bft::accuse;

extern "C" {

// the walk of every instance, then the compaction. counts: CNT_WORDS words. Returns the number of records found, of
// which the first min(that, rec_cap) are written.
uint64_t accuse_host(const uint8_t* code, const uint32_t* hx, const uint64_t* round, const uint8_t* digest,
                     const uint8_t* status, const int32_t* signer, const uint64_t* inst_frame0, uint64_t inst,
                     uint64_t frames, uint32_t n, uint32_t view_cap, uint32_t max_heights, uint32_t* frame_pair,
                     uint64_t* inst_accused, uint32_t* inst_flags, Record* records, uint64_t rec_cap, uint64_t* counts) {
    audit::Recs r{};
    r.code = (uint8_t*)code; r.hx = (uint32_t*)hx; r.round = (uint64_t*)round; r.digest = (uint8_t*)digest;
    for (uint32_t k = 0; k < CNT_WORDS; ++k) counts[k] = 0;
    for (uint64_t k = 0; k < frames; ++k) frame_pair[k] = NONE;
    if (view_cap == 0) view_cap = default_view_cap(max_heights);
    View* views = (View*)malloc(sizeof(View) * view_cap);             // exactly the table: a slot past it is caught
    uint32_t* first = (uint32_t*)malloc(sizeof(uint32_t) * 3 * n * view_cap);
    for (uint64_t in = 0; in < inst; ++in) {
        const uint64_t f0 = inst_frame0[in];
        uint32_t nviews = 0, flags = 0;
        uint64_t acc[4] = {0, 0, 0, 0};
        for (uint64_t k = f0; k < inst_frame0[in + 1]; ++k) {
            if (!accuse::counts(status[k], code[k], hx[k]) || (uint32_t)signer[k] >= n) continue;
            uint32_t slot = NONE;
            for (uint32_t s = 0; s < nviews; ++s)
                if (view_is(views[s], hx[k], round[k])) slot = s;
            if (slot == NONE) {
                if (nviews == view_cap) { flags |= FLAG_VIEW_OVERFLOW; continue; }
                slot = nviews++;
                view_put(views[slot], hx[k], round[k]);
                for (uint32_t j = 0; j < 3 * n; ++j) first[(uint64_t)slot * 3 * n + j] = NONE;
            }
            const uint32_t a = group_step(first + cell(slot, code[k], (uint32_t)signer[k], n), (uint32_t)(k - f0), k, digest);
            if (a == NONE) continue;
            frame_pair[k] = (uint32_t)(f0 + a);
            counts[CNT_RECORDS] += 1;
            counts[CNT_CODE + code[k] - 1u] += 1;
            acc[((uint32_t)signer[k] >> 6) & 3u] |= 1ull << (signer[k] & 63);
        }
        uint32_t pc = 0;
        for (int q = 0; q < 4; ++q) {
            inst_accused[4 * in + q] = acc[q];
            pc += (uint32_t)__builtin_popcountll(acc[q]);
        }
        inst_flags[in] = flags;
        counts[CNT_ACCUSED] += pc;
        counts[CNT_INSTANCES] += pc ? 1 : 0;
        counts[CNT_VIEW_OVERFLOWS] += flags & FLAG_VIEW_OVERFLOW ? 1 : 0;
    }
    free(first);
    free(views);
    uint64_t total = 0;
    for (uint64_t k = 0; k < frames; ++k) {
        if (frame_pair[k] == NONE) continue;
        if (total < rec_cap) record_put(records[total], r, signer, inst_of(inst_frame0, inst, k), frame_pair[k], k);
        ++total;
    }
    return total;
}
}

#ifdef ACCUSE_HOST_MAIN
// stdin (little-endian): u64 frames, inst, rec_cap, want_total; u32 n, view_cap, max_heights, pad; then the arrays
// code[F] hx[F] round[F] digest[F][32] status[F] signer[F] inst_frame0[inst + 1], then the expected frame_pair[F]
// inst_accused[inst][4] inst_flags[inst] records[min(want_total, rec_cap)] counts[CNT_WORDS]
template <class T> static T* take(uint64_t count) {
    T* p = (T*)malloc(count ? count * sizeof(T) : 1);                 // exactly the counted size
    if (count && fread(p, sizeof(T), count, stdin) != count) exit(2);
    return p;
}
template <class T> static T* room(uint64_t count) { return (T*)malloc(count ? count * sizeof(T) : 1); }
int main() {
    uint64_t* hd = take<uint64_t>(4);
    uint32_t* hw = take<uint32_t>(4);
    const uint64_t F = hd[0], I = hd[1], cap = hd[2], want_total = hd[3];
    const uint32_t n = hw[0], view_cap = hw[1], H = hw[2];
    if (F > (1u << 24) || I > (1u << 20) || cap > (1u << 24) || n < 1 || n > 256) return 2;
    uint8_t* code = take<uint8_t>(F);
    uint32_t* hx = take<uint32_t>(F);
    uint64_t* round = take<uint64_t>(F);
    uint8_t* digest = take<uint8_t>(F * 32);
    uint8_t* status = take<uint8_t>(F);
    int32_t* signer = take<int32_t>(F);
    uint64_t* if0 = take<uint64_t>(I + 1);
    const uint64_t written = want_total < cap ? want_total : cap;
    uint32_t* want_pair = take<uint32_t>(F);
    uint64_t* want_acc = take<uint64_t>(I * 4);
    uint32_t* want_flags = take<uint32_t>(I);
    Record* want_recs = take<Record>(written);
    uint64_t* want_counts = take<uint64_t>(CNT_WORDS);
    uint32_t* pair = room<uint32_t>(F);
    uint64_t* acc = room<uint64_t>(I * 4);
    uint32_t* flags = room<uint32_t>(I);
    Record* recs = room<Record>(cap);
    uint64_t counts[CNT_WORDS];
    const uint64_t total = accuse_host(code, hx, round, digest, status, signer, if0, I, F, n, view_cap, H, pair, acc, flags,
                                       recs, cap, counts);
    int rc = 0;
    if (total != want_total) { printf("records %llu, expected %llu\n", (unsigned long long)total, (unsigned long long)want_total); rc = 1; }
    if (memcmp(pair, want_pair, F * 4)) { printf("frame_pair differs\n"); rc = 1; }
    if (memcmp(acc, want_acc, I * 32)) { printf("inst_accused differs\n"); rc = 1; }
    if (memcmp(flags, want_flags, I * 4)) { printf("inst_flags differs\n"); rc = 1; }
    if (rc == 0 && memcmp(recs, want_recs, written * sizeof(Record))) { printf("records differ\n"); rc = 1; }
    if (memcmp(counts, want_counts, sizeof counts)) { printf("counts differ\n"); rc = 1; }
    if (rc == 0) printf("ok %llu frames %llu records\n", (unsigned long long)F, (unsigned long long)total);
    void* all[] = {hd, hw, code, hx, round, digest, status, signer, if0, want_pair, want_acc, want_flags, want_recs,
                   want_counts, pair, acc, flags, recs};
    for (void* p : all) free(p);
    return rc;
}
#endif
