// bft_trace.h — the signed wire frame of one logged consensus broadcast (SPEC.md §11b), composed from the
// emitters the tree already has and shared by the host and the GPU:
//   frame   = emit_frame {Header{Consensus, ttl 10, create_time 0, peer_id None}, payload}   (bft_wire_block.h)
//   payload = GossipMessage {code, create_time, msg, signature: Some, commit_seal}            (protocol/mod.rs:44-53)
//   msg     = crypto::emit_msg: Subject {view, digest}, or PrePrepare {view, Block{header, []}} over the
//             header bytes of header_raw                                                       (bft_crypto.h)
// The same code runs with a counting functor (the size pass) and with a bounded writer (the emit pass), so the
// two passes agree by construction; the writer never stores past the counted length.
#pragma once
#include "bft_common.h"
#include "bft_crypto.h"
#include "bft_wire_block.h"

namespace bft {

// what the trace kernels read of a launch (bftsim.hip): the message log, and what bftsim_crypto_verify kept
struct TraceArgs {
    const uint32_t* mlog;
    uint32_t cap;
    // dense, per message: kept by bftsim_crypto_verify (bftsim_set_trace_keep)
    const uint64_t* moff;             // [n_inst + 1]
    const uint64_t* mref;
    const uint8_t* raw;
    const uint32_t* msg_k;
    const uint8_t* sigs;
    const uint8_t* seals;
};
// twins (bftsim_set_trace_twins, SPEC.md §11f): the merged frame index and, per twin slot, what TraceArgs' dense arrays
// hold per message. An argument of the twin kernels alone (TwinOpt)
struct TwinArgs {
    const uint64_t* fmap;             // [frames] message, | twins::F_TWIN for a twin
    const uint32_t* tslot;            // [messages + 1] twins before message m: a twin's slot
    const uint8_t* traw;
    const uint32_t* tmsg_k;
    const uint8_t* tsigs;
    const uint8_t* tseals;
};

namespace trace {

// what bftsim_crypto_verify derived for one message
struct Msg {
    uint32_t code;                    // MessageType 1..4
    uint64_t ctime, round, height;
    const uint8_t* digest;            // 32 bytes (Prepare / Commit / RoundChange)
    const uint8_t* header;            // Preprepare: the block's header bytes, else null
    uint32_t hlen;
    const uint8_t* sig;               // 65 bytes
    const uint8_t* seal;              // Commit: 65 bytes, else null
};

// create_time: RoundChange carries the wall clock in ms (round_change.rs:61), the others 0
BFT_FN uint64_t create_time(uint32_t code, uint64_t genesis_time, uint32_t block_period, uint32_t tick) {
    return code == (uint32_t)MT_ROUND_CHANGE ? 1000ull * (genesis_time + (uint64_t)block_period * (uint64_t)tick) : 0ull;
}

template <class E>
BFT_FN void emit_gossip(const E& e, const Msg& m) {
    using crypto::mp_arr;
    using crypto::mp_uint;
    uint32_t ml = 0;
    crypto::emit_msg(wire::CountE{&ml}, m.round, m.height, m.digest, m.header, m.hlen);
    mp_arr(e, 5);
    mp_arr(e, 2); mp_uint(e, m.code - 1u); mp_arr(e, 0);    // MessageType unit variant
    mp_uint(e, m.ctime);
    mp_arr(e, ml);
    crypto::emit_msg(wire::UintE<E>{&e}, m.round, m.height, m.digest, m.header, m.hlen);
    wire::emit_bytes(e, m.sig, 65);
    if (m.seal) wire::emit_bytes(e, m.seal, 65); else e(0xc0);
}
// what TcpServer::broadcast puts on the wire (p2p/server.rs:187, p2p/codec.rs:15-53)
template <class E>
BFT_FN void emit(const E& e, const Msg& m) {
    wire::emit_frame(e, wire::P2P_CONSENSUS, wire::DEFAULT_TTL, 0ull, [&](const auto& f) { emit_gossip(f, m); });
}
BFT_FN uint32_t frame_len(const Msg& m) {
    uint32_t n = 0;
    emit(wire::CountE{&n}, m);
    return n;
}
// the frame into out[0, len): `len` is frame_len's count; returns the emitted length (!= len: the passes
// disagree, and nothing was stored past len)
BFT_FN uint32_t write_frame(uint8_t* out, uint32_t len, const Msg& m) {
    uint32_t n = 0;
    emit(wire::BufE{out, &n, len}, m);
    return n;
}

}  // namespace trace
}  // namespace bft
