// ledger_host.cpp — TEST-ONLY host build of consensus-rs_amd/csrc/bft_ledger.h (the decode, scatter, tally and link
// steps the importer's kernels run), checked against tests/ledger_ref.py on the CPU. As a shared library
// (tests/ledger_lib.py) it runs the importer in two halves with the recoveries, taken from the C oracle, in between;
// with -DLEDGER_HOST_MAIN it is a stand-alone program for the sanitizers: it reads headers from stdin and decodes
// every truncation and every single-byte flip of each, from heap buffers of exactly the header's length.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../consensus-rs_amd/csrc/bft_ledger.h"

using namespace bft;
using namespace bft::ledger;

extern "C" {

uint64_t ledger_host_rec_size(void) { return sizeof(Rec); }

// first half: the record of every slot and the first dense vote slot of each (vbase: slots + 1 words); returns the
// length of the dense vote list
uint64_t ledger_host_decode(const uint8_t* hdr, uint64_t slot_bytes, const uint32_t* hdr_len, uint64_t slots, Rec* recs,
                            uint64_t* vbase) {
    uint8_t kbuf[136];
    uint64_t V = 0;
    for (uint64_t i = 0; i < slots; ++i) {
        vbase[i] = V;
        V += decode_header(hdr + i * slot_bytes, hdr_len[i], slot_bytes, kbuf, recs[i]);
    }
    vbase[slots] = V;
    return V;
}
void ledger_host_scatter(const uint8_t* hdr, uint64_t slot_bytes, const uint32_t* hdr_len, uint64_t slots, const Rec* recs,
                         const uint64_t* vbase, uint8_t* vsig, uint32_t* vhdr, uint8_t* vdig) {
    for (uint64_t i = 0; i < slots; ++i)
        if (recs[i].st == ST_OK && recs[i].n_votes != NONE)
            scatter_votes(hdr + i * slot_bytes, hdr_len[i], recs[i], (uint32_t)i, vbase[i], vsig, vhdr, vdig);
}
// second half: the tally of every header from the recoveries, the statuses, verified_height. counts: CNT_WORDS words
void ledger_host_finish(const Rec* recs, const uint64_t* vbase, uint64_t inst, uint32_t H, const uint8_t* addresses, uint32_t n,
                        uint32_t quorum, uint32_t block_period, const uint8_t* genesis_hash, uint64_t genesis_time,
                        const uint8_t* vaddr, const uint8_t* vok, uint8_t* status, uint8_t* bhash, uint64_t* voters,
                        uint16_t* n_votes, uint64_t* vheight, uint64_t* counts) {
    for (uint32_t k = 0; k < CNT_WORDS; ++k) counts[k] = 0;
    for (uint64_t i = 0; i < inst * H; ++i) {
        const Rec& r = recs[i];
        Tally t{{0, 0, 0, 0}, 0, 0};
        const bool has = r.st == ST_OK && r.n_votes != NONE;
        if (has)
            for (uint32_t v = 0; v < r.n_votes; ++v) tally_vote(t, vote_validator(addresses, n, vaddr, vok, vbase[i] + v));
        memcpy(voters + 4 * i, t.voters, 32);
        const uint32_t st = link_status(recs + (i / H) * H, (uint32_t)(i % H) + 1u, genesis_hash, genesis_time, block_period,
                                        t.voters, t.bad, quorum, addresses, n);
        status[i] = (uint8_t)st;
        n_votes[i] = (uint16_t)(has ? r.n_votes : 0u);
        memcpy(bhash + 32 * i, r.bhash, 32);
        counts[CNT_STATUS + st] += 1;
        if (st != ST_ABSENT) counts[CNT_HEADERS] += 1;
        counts[CNT_DUP] += t.dup;
    }
    for (uint64_t in = 0; in < inst; ++in) {
        bool whole = false;
        vheight[in] = verified_height(status + in * H, H, &whole);
        if (whole) counts[CNT_WHOLE] += 1;
    }
}
}

#ifdef LEDGER_HOST_MAIN
// stdin: u32 count, then per header {u32 len, u8 header[len]} (little-endian)
static bool rd(void* p, size_t n) { return fread(p, 1, n, stdin) == n; }
// the header from a heap buffer of exactly `len` bytes (a read past it is caught); its votes scattered when it decodes
static uint32_t decode_exact(const uint8_t* src, uint32_t len) {
    uint8_t* f = (uint8_t*)malloc(len ? len : 1);
    memcpy(f, src, len);
    uint8_t kbuf[136];
    Rec r;
    const uint32_t nv = decode_header(f, len, len, kbuf, r);
    if (r.st == ST_OK && r.n_votes != NONE) {
        std::vector<uint8_t> vsig(65 * (nv ? nv : 1)), vdig(32 * (nv ? nv : 1));
        std::vector<uint32_t> vhdr(nv ? nv : 1);
        scatter_votes(f, len, r, 0, 0, vsig.data(), vhdr.data(), vdig.data());
    }
    free(f);
    return r.st;
}
int main() {
    uint32_t count = 0;
    if (!rd(&count, 4)) return 2;
    uint64_t cases = 0;
    for (uint32_t k = 0; k < count; ++k) {
        uint32_t len = 0;
        if (!rd(&len, 4) || len == 0 || len > (1u << 20)) return 2;
        std::vector<uint8_t> h(len);
        if (!rd(h.data(), len)) return 2;
        if (decode_exact(h.data(), len) != ST_OK) { printf("header %u does not decode\n", k); return 1; }
        if (decode_exact(h.data(), 0) != ST_ABSENT) { printf("header %u of length 0 is not absent\n", k); return 1; }
        for (uint32_t cut = 1; cut < len; ++cut, ++cases)           // every truncation is undecodable
            if (decode_exact(h.data(), cut) != ST_UNDECODABLE) { printf("header %u cut at %u decodes\n", k, cut); return 1; }
        for (uint32_t j = 0; j < len; ++j)                          // every single-byte flip: any status, no bad access
            for (uint8_t x : {(uint8_t)0x01, (uint8_t)0x80, (uint8_t)0xff}) {
                h[j] ^= x;
                (void)decode_exact(h.data(), len);
                h[j] ^= x;
                ++cases;
            }
    }
    printf("ok %u headers %llu cases\n", count, (unsigned long long)cases);
    return 0;
}
#endif
