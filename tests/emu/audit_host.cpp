// audit_host.cpp — TEST-ONLY host build of consensus-rs_amd/csrc/bft_audit.h (the per-frame parsing, classification
// and tally step the observer's kernels run), checked against tests/audit_ref.py on the CPU. As a shared library
// (tests/audit_lib.py) it runs the observer in two halves with the recoveries, taken from the C oracle, in between;
// with -DAUDIT_HOST_MAIN it is a stand-alone program for the sanitizers: it reads frames from stdin and parses every
// truncation and every single-byte flip of each, from heap buffers of exactly the frame's length; then, if more follows,
// the catalogue of tests/wire_mutations.py with the strict reference's verdicts, each frame parsed the same way.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../consensus-rs_amd/csrc/bft_audit.h"

using namespace bft;
using namespace bft::audit;

// one frame -> its record, in the order the decode kernel tries the decoders
static void decode_one(const uint8_t* p, uint64_t span, const uint8_t* addresses, uint32_t n, bool seed_le,
                       uint32_t max_heights, const Recs& r, uint64_t i, uint32_t* n_seals) {
    uint8_t kbuf[136];
    if (span > MAX_SPAN) { rec_undecodable(r, i); return; }
    wire::Decoded d;
    if (wire::decode_frame(p, (uint32_t)span, d)) {
        if (!subject_record(d, max_heights, kbuf, r, i)) rec_undecodable(r, i);
        else if (d.code == (uint32_t)MT_COMMIT) seal_record(d, kbuf, r, i, (*n_seals)++);
        return;
    }
    bftwire_preprepare* pp = (bftwire_preprepare*)malloc(sizeof(bftwire_preprepare));
    uint8_t* mbuf = (uint8_t*)malloc(PP_BUF);
    uint32_t has_seal = 0;
    if (!(wire::decode_pp_frame(p, (uint32_t)span, *pp, &has_seal) &&
          pp_record(*pp, has_seal, addresses, n, seed_le, max_heights, kbuf, mbuf, r, i)))
        rec_undecodable(r, i);
    free(mbuf);
    free(pp);
}

extern "C" {

// first half: the records of every frame; returns the length of the dense seal list
uint32_t audit_host_decode(const uint8_t* stream, const uint64_t* frame_off, uint64_t frames, const uint8_t* addresses,
                           uint32_t n, uint32_t seed_le, uint32_t max_heights, const Recs* r) {
    uint32_t n_seals = 0;
    for (uint64_t i = 0; i < frames; ++i)
        decode_one(stream + frame_off[i], frame_off[i + 1] - frame_off[i], addresses, n, seed_le != 0, max_heights, *r, i,
                   &n_seals);
    return n_seals;
}

// second half: statuses and signers from the recoveries, then the tally of every instance. counts: CNT_WORDS words
void audit_host_finish(const Recs* rp, uint64_t frames, const uint8_t* addresses, uint32_t n, const uint8_t* rec_addr,
                       const uint8_t* rec_ok, const uint8_t* seal_addr, const uint8_t* seal_ok, const uint64_t* inst_frame0,
                       uint64_t inst, uint32_t max_heights, uint32_t key_cap, uint32_t quorum, uint8_t* status,
                       int32_t* signer, uint32_t* inst_flags, uint16_t* cert_rnd, uint8_t* cert_digest, uint64_t* cert_voters,
                       uint32_t* cert_frame, uint8_t* cert_flg, uint64_t* counts) {
    const Recs& r = *rp;
    for (uint32_t k = 0; k < CNT_WORDS; ++k) counts[k] = 0;
    for (uint64_t i = 0; i < frames; ++i) {
        const uint32_t st = classify(r, i, addresses, n, rec_addr, rec_ok, seal_addr, seal_ok, &signer[i]);
        status[i] = (uint8_t)st;
        counts[CNT_STATUS + st] += 1;
        if (st == ST_OK || st == ST_SEAL_FOREIGN) counts[CNT_CODE + r.code[i] - 1u] += 1;
    }
    if (key_cap == 0) key_cap = 4u * max_heights + 64u;
    std::vector<Key> keys(key_cap);
    for (uint64_t in = 0; in < inst; ++in) {
        uint32_t nkeys = 0, flags = 0;
        for (uint64_t k = inst_frame0[in]; k < inst_frame0[in + 1]; ++k) {
            const uint32_t st = status[k], code = r.code[k];
            if (!((st == ST_OK || st == ST_SEAL_FOREIGN) && (code == (uint32_t)MT_PREPREPARE || code == (uint32_t)MT_COMMIT)))
                continue;
            if (r.hx[k] == 0) { counts[CNT_OUT_OF_RANGE] += 1; continue; }
            Vote v;
            memcpy(v.digest, r.digest + 32 * k, 32);
            v.round = r.round[k]; v.hx = r.hx[k]; v.code = code; v.signer = (uint32_t)signer[k]; v.want = r.pp_want[k];
            uint32_t slot = NONE, rel_any = 0;
            for (uint32_t s = 0; s < nkeys; ++s) {
                const uint32_t rel = key_relation(keys[s], v);
                if (rel & 1u) slot = s;
                rel_any |= rel;
            }
            if (code == (uint32_t)MT_COMMIT && (rel_any & 4u)) continue;
            const bool fresh = slot == NONE;
            if (fresh) {
                if (nkeys == key_cap) { flags |= 1u; continue; }
                slot = nkeys++;
            }
            const uint32_t res = tally_apply(keys[slot], fresh, v, quorum, (rel_any & 2u) != 0);
            if (res & TALLY_CERTIFY) {
                const uint64_t row = in * max_heights + (v.hx - 1u);
                cert_rnd[row] = cert_round(keys[slot]);
                memcpy(cert_digest + 32 * row, keys[slot].digest, 32);
                memcpy(cert_voters + 4 * row, keys[slot].voters, 32);
                cert_frame[row] = (uint32_t)(k - inst_frame0[in]);
                cert_flg[row] = (uint8_t)cert_flags(keys[slot]);
                counts[CNT_CERTIFIED] += 1;
            }
            if (res & TALLY_CONFLICT) { counts[CNT_CONFLICTS] += 1; flags |= 2u; }
        }
        inst_flags[in] = flags;
        if (flags & 1u) counts[CNT_KEY_OVERFLOWS] += 1;
    }
}
}

#ifdef AUDIT_HOST_MAIN
// stdin: u32 n, u8 addresses[n][20], u32 count, then per frame {u32 len, u8 frame[len]} (little-endian); optionally
// u32 cases, then per case {u8 decodable, u32 len, u8 frame[len]}
static bool rd(void* p, size_t n) { return fread(p, 1, n, stdin) == n; }
struct OneRec {
    uint8_t st, code, digest[32], sdig[32], sig[65], seal_dig[32], seal[65];
    uint32_t hx, seal_k, pp_want;
    uint64_t round;
    Recs recs() { return Recs{&st, &code, &hx, &round, digest, sdig, sig, &seal_k, &pp_want, seal_dig, seal}; }
};
// the frame from a heap buffer of exactly `len` bytes: a read past it is caught
static uint32_t parse_exact(const uint8_t* src, uint32_t len, const uint8_t* addr, uint32_t n) {
    uint8_t* f = (uint8_t*)malloc(len ? len : 1);
    memcpy(f, src, len);
    OneRec o;
    uint32_t n_seals = 0;
    decode_one(f, len, addr, n, false, 65535u, o.recs(), 0, &n_seals);
    free(f);
    return o.st;
}
int main() {
    uint32_t n = 0, count = 0;
    if (!rd(&n, 4) || n < 1 || n > 256) return 2;
    std::vector<uint8_t> addr(20 * n);
    if (!rd(addr.data(), addr.size()) || !rd(&count, 4)) return 2;
    uint64_t cases = 0;
    for (uint32_t k = 0; k < count; ++k) {
        uint32_t len = 0;
        if (!rd(&len, 4) || len > (1u << 20)) return 2;
        std::vector<uint8_t> fr(len);
        if (!rd(fr.data(), len)) return 2;
        if (parse_exact(fr.data(), len, addr.data(), n) != ST_OK) { printf("frame %u does not decode\n", k); return 1; }
        for (uint32_t cut = 0; cut < len; ++cut, ++cases)          // every truncation is undecodable
            if (parse_exact(fr.data(), cut, addr.data(), n) != ST_UNDECODABLE) { printf("frame %u cut at %u decodes\n", k, cut); return 1; }
        for (uint32_t j = 0; j < len; ++j)                         // every single-byte flip: any status, no bad access
            for (uint8_t x : {(uint8_t)0x01, (uint8_t)0x80, (uint8_t)0xff}) {
                fr[j] ^= x;
                (void)parse_exact(fr.data(), len, addr.data(), n);
                fr[j] ^= x;
                ++cases;
            }
    }
    printf("ok %u frames %llu cases\n", count, (unsigned long long)cases);
    uint32_t ncat = 0;
    if (!rd(&ncat, 4)) return 0;                                   // no catalogue
    for (uint32_t k = 0; k < ncat; ++k) {
        uint8_t want = 0;
        uint32_t len = 0;
        if (!rd(&want, 1) || !rd(&len, 4) || len > (1u << 20)) return 2;
        std::vector<uint8_t> fr(len);
        if (!rd(fr.data(), len)) return 2;
        const uint32_t st = parse_exact(fr.data(), len, addr.data(), n);
        if (st != (want ? (uint32_t)ST_OK : (uint32_t)ST_UNDECODABLE)) { printf("case %u: status %u, decodable %u\n", k, st, want); return 1; }
    }
    printf("catalogue ok %u cases\n", ncat);
    return 0;
}
#endif
