// trace_host.cpp — TEST-ONLY host build of consensus-rs_amd/csrc/bft_trace.h (the frame emitter the trace
// kernels run), checked against tests/trace_ref.py on the CPU. As a shared library (tests/trace_lib.py) it
// emits one frame; with -DTRACE_HOST_MAIN it is a stand-alone program for the sanitizers: it reads messages
// and their expected frames from stdin, emits each frame into a heap buffer of exactly the counted length
// and compares.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../consensus-rs_amd/csrc/bft_trace.h"

using namespace bft::trace;

extern "C" {
// the frame of one message into out[0, cap); returns the emitted length, *counted = the size pass's length.
// header: a Preprepare's header bytes (else null); seal: a Commit's (else null)
uint32_t trace_host_frame(uint32_t code, uint64_t ctime, uint64_t round, uint64_t height, const uint8_t* digest,
                          const uint8_t* header, uint32_t hlen, const uint8_t* sig, const uint8_t* seal, uint8_t* out,
                          uint32_t cap, uint32_t* counted) {
    const Msg m{code, ctime, round, height, digest, header, hlen, sig, seal};
    *counted = frame_len(m);
    return write_frame(out, cap, m);
}
uint64_t trace_host_create_time(uint32_t code, uint64_t genesis_time, uint32_t block_period, uint32_t tick) {
    return create_time(code, genesis_time, block_period, tick);
}
}

#ifdef TRACE_HOST_MAIN
// stdin: u32 count, then per message {u32 code, u64 ctime, u64 round, u64 height, u8 digest[32], u32 hlen,
// u8 header[hlen], u8 sig[65], u8 has_seal, u8 seal[65] if has_seal, u32 flen, u8 frame[flen]} (little-endian)
static bool rd(void* p, size_t n) { return fread(p, 1, n, stdin) == n; }
int main() {
    uint32_t count = 0;
    if (!rd(&count, 4)) return 2;
    uint64_t bytes = 0;
    for (uint32_t k = 0; k < count; ++k) {
        uint32_t code, hlen, flen;
        uint64_t ctime, round, height;
        uint8_t digest[32], sig[65], seal[65], has_seal;
        if (!rd(&code, 4) || !rd(&ctime, 8) || !rd(&round, 8) || !rd(&height, 8) || !rd(digest, 32) || !rd(&hlen, 4)) return 2;
        uint8_t* header = hlen ? (uint8_t*)malloc(hlen) : nullptr;
        if (hlen && !rd(header, hlen)) return 2;
        if (!rd(sig, 65) || !rd(&has_seal, 1) || (has_seal && !rd(seal, 65)) || !rd(&flen, 4)) return 2;
        uint8_t* want = (uint8_t*)malloc(flen ? flen : 1);
        if (!rd(want, flen)) return 2;
        const Msg m{code, ctime, round, height, digest, header, hlen, sig, has_seal ? seal : nullptr};
        const uint32_t len = frame_len(m);
        uint8_t* got = (uint8_t*)malloc(len ? len : 1);      // exactly the counted length: a store past it is caught
        const uint32_t n = write_frame(got, len, m);
        if (n != len || len != flen || memcmp(got, want, len) != 0) {
            printf("frame %u: counted %u emitted %u expected %u%s\n", k, len, n, flen, len == flen ? ", bytes differ" : "");
            return 1;
        }
        // a short buffer: nothing is stored past it, and the emitted length still reports the full frame
        const uint32_t cut = len / 2;
        uint8_t* part = (uint8_t*)malloc(cut ? cut : 1);
        if (write_frame(part, cut, m) != len || memcmp(part, want, cut) != 0) {
            printf("frame %u: bounded write differs\n", k);
            return 1;
        }
        bytes += len;
        free(part); free(got); free(want); free(header);
    }
    printf("ok %u frames %llu bytes\n", count, (unsigned long long)bytes);
    return 0;
}
#endif
