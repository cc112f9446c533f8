// bftsim_impl.h — what libbftsim's host translation units share (bftsim.hip, bftsim_observe.hip): the handle, the error
// path, the owners of the cold paths' temporaries, libbftsig's entry points and the kept trace's passes. Internal: all
// but the handle has hidden visibility, so the library exports none of it.
#pragma once
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>                 // types only: librccl is opened at bftsim_comm_init (dlopen)

#include <initializer_list>
#include <string>
#include <vector>

#include "bft_hip.h"
#include "bft_trace.h"

struct bftsim {
    bftsim_config cfg;
    std::vector<uint8_t> addresses;
    int device = 0;
    std::string err;
    uint8_t genesis_hash[32];
    uint32_t genesis_seed = 0;
    uint32_t seg = 64;
    uint32_t hcap = 0;
    // device buffers
    uint64_t cap_inst = 0;
    uint8_t* d_addr = nullptr;
    uint8_t* d_ghash = nullptr;
    unsigned long long* d_stats = nullptr;
    uint64_t* d_red = nullptr;        // bftsim_stats image reduced by bftsim_stats_allreduce
    uint4* d_evict = nullptr;         // attribution pass only (bft_l2_evict_kernel): 64 MiB of zeros
    bool pmc_evict = false;
    ncclComm_t comm = nullptr;        // bftsim_comm_init: one rank of a multi-GPU run (RCCL over xGMI)
    // real-crypto mode (bftsim_set_crypto, SPEC.md §11)
    bool crypto = false;
    uint64_t forged[4] = {0, 0, 0, 0};
    uint32_t mlog_cap = 0;
    uint32_t* d_mlog = nullptr;       // [cap_inst][mlog_cap][MLOG_WORDS]
    uint32_t* d_mlog_n = nullptr;     // [cap_inst]
    uint8_t* d_keys = nullptr;        // [2N][32]: the validators' secrets, then their forged keys
    uint32_t* d_vsnap = nullptr;      // [cap_inst][seg][8] commit set at each lane's last commit
    uint32_t* d_votes = nullptr;      // [cap_inst][rows][8] canonical committer's commit set per height
    uint8_t* d_vsig = nullptr;        // [last_n][H][N][65] the votes' signatures, or their seals (bftsim_crypto_verify)
    uint8_t* d_vhas = nullptr;        // [last_n][H][N]
    uint64_t vsig_n = 0;              // instances d_vsig holds (0: no verify since the last launch)
    uint32_t ledger_votes = BFTSIM_VOTES_SIGNATURES;   // what the next verify gathers (bftsim_set_ledger_votes)
    void* sig = nullptr;              // libbftsig handle (bftsig_t*)
    // the trace (bftsim_set_trace_keep, SPEC.md §11b): what bftsim_crypto_verify kept of the last launch
    bool trace_keep = false;
    uint8_t* d_tkeep = nullptr;       // one allocation: moff, mref, raw, msg_k, sigs, seals (trace_args points into it)
    bft::TraceArgs trace_args{};
    bft::TwinArgs twin_args{};
    uint64_t trace_n = 0, trace_M = 0;    // instances (0: nothing kept) and messages it holds
    uint64_t* d_tfoff = nullptr;      // [M + 1] frame offsets, then [n + 1] instance offsets, then the error counter
    std::vector<uint64_t> trace_moff, trace_ioff;   // host, [n + 1]: first frame / first stream byte of each instance
    float trace_ms[3] = {0, 0, 0};    // size pass + scan, emit kernel, device-to-host copies of the last calls
    // twins (bftsim_set_trace_twins, SPEC.md §11f): the kept trace's frames are its messages and their twins
    bool trace_twins = false;         // what the next keeping verify does
    bool trace_has_twins = false;     // the kept trace was built with twins on
    uint8_t* d_twkeep = nullptr;      // one allocation: tslot, if0, fmap, traw, tmsg_k, tsigs, tseals (trace_args points into it)
    const uint64_t* d_tif0 = nullptr; // [n + 1] first frame of each instance (twins off: trace_args.moff)
    uint64_t trace_F = 0;             // frames: trace_M + the twins
    uint64_t twin_counts[2] = {0, 0}; // PrePrepare twins, vote twins of the kept trace
    float twin_ms[3] = {0, 0, 0};     // mark + scan + merge, digests, signing of the last verify with twins on
    float audit_ms[4] = {0, 0, 0, 0}; // decode, recoveries, classify + tally, copies of the last audit (SPEC.md §11c)
    float ledger_ms[4] = {0, 0, 0, 0};// decode, recoveries, tally + link, copies of the last bftsim_verify_ledger (§11d)
    uint8_t* d_tips = nullptr;        // [cap_inst * 32]
    uint64_t backlog_bytes = 0;
    int fast = 1;                     // FAST kernel + resume for N = 64 (bftsim_set_fast(h, 0): full kernel)
    uint32_t window = 0;              // 0: full per-height rows; else ring of `window` rows
    uint32_t rcs_k = bft::RCS_DEFAULT_K;   // RoundChangeSet rounds per validator (bftsim_set_rcs_capacity)
    uint64_t* d_trace = nullptr;
    uint64_t* h_trace = nullptr;
    uint32_t trace_ticks = 0;
    uint64_t n_req = 0;               // instances of the next launch (bftsim_prepare); <= cap_inst
    uint64_t last_n = 0, last_first = 0;
    uint32_t last_set = 0;            // the row-table set of the last launch
    hipStream_t last_stream = nullptr;
    // Every device buffer of a launch belongs to a row-table set (RowSet): bftsim_prepare allocates sets[0 .. n_sets),
    // n_sets = max(1, pipeline), and free_bufs releases them; the handle holds no pointer into a set. An unpipelined
    // launch runs on set 0; whatever reads a launch's results reads sets[last_set].
    // Pipelined launches (bftsim_set_pipeline(h, D), the batch-throughput mode): a ring of D row-table sets,
    // each with the scratch of one launch, so that up to D launches are in flight at once.
    //   * the consensus kernel (+ resume + suffix rows) of each launch runs on one of `n_cs` launch streams
    //     (round-robin), after the caller's earlier work on its stream and after its set's last chain;
    //   * the prev_hash chains of `hash_batch` consecutive launches run as ONE chain kernel on one of `n_hs`
    //     hash streams (round-robin). A chain is sequential in height and a launch's chains take ~1.5 ms
    //     whatever their number, so batching B launches per kernel gives B times the chain throughput
    //     (profiles/r04). Results are complete once bftsim_sync (or any fetch) returns; those flush a
    //     partial batch first.
    static constexpr uint32_t MAX_SETS = 32, MAX_CS = 8, MAX_HS = 8, MAX_BATCH = bft::CHAIN_MAX_SETS;
    struct RowSet {
        uint32_t* ch = nullptr; uint32_t* flags = nullptr; uint32_t* ticks = nullptr; uint64_t* views = nullptr;
        uint32_t* rec = nullptr; uint8_t* hash = nullptr;
        uint32_t* sfx = nullptr;      // header suffix rows of the hash pass (sfx_rows per instance)
        uint32_t* spec = nullptr;     // little-endian seeds, N = 64: predicted blocks [H + 1][n] (seed chain)
        // big-endian seeds, N = 64: predicted chains: Byzantine masks [n], first height whose
        // recorded block differs from its prediction [n]
        uint64_t* byz = nullptr; uint32_t* bad = nullptr;
        uint32_t* pred = nullptr;     // [n][H] the predicted block of each height (bft_spec_suffix_kernel)
        // a launch's own scratch
        uint64_t* hist = nullptr;     // [HIST_BINS]
        uint32_t* rcs = nullptr;      // RoundChangeSet tables, rcs_words(seg) per wave / workgroup
        uint32_t* backlog = nullptr;  // replay mode: backlog slots, backlog_words(seg) per wave / workgroup
        // FAST launches (N = 64): [n] hand-over flags, [2 + n] the resume kernel's queue, [SAVE_WORDS][n * 64] saved
        // lane state
        uint32_t* resume = nullptr; uint32_t* resume_q = nullptr; uint32_t* save = nullptr;
        // host-mapped: the hand-over count of the set's last launch (resume grid). Like the events it lives until
        // bftsim_destroy: a grid estimate that outlasts the buffers
        uint32_t* hint = nullptr;
        hipEvent_t done = nullptr;    // hash pass of the last launch that used the set
        hipEvent_t batch_done = nullptr;   // or: the event of the chain batch that hashed it (flush_batch)
        hipEvent_t entry = nullptr;   // the caller's stream at the launch call
        bool busy = false;
    } sets[MAX_SETS];
    // block-hash chains: one wave per instance (bft_hash_chain_wave_kernel) up to this many instances per
    // launch, lane pairs above. 0: lane pairs at every size -- the wave chain measured slower at every
    // shard size (ds_bpermute latency and LDS issue at low occupancy), kept as an A/B arm
    // (BFTSIM_TESTING + BFTSIM_CHAIN_WAVE_MAX)
    uint64_t chain_wave_max = 0;
    // one lane per instance from this many instances per launch (kern_fast.hip bft_hash_chain_lane_kernel: fewer
    // instructions per header, longer chains; BFTSIM_TESTING + BFTSIM_CHAIN_LANE_MIN overrides)
    // predicted lanes against predicted lane pairs (r06/ab_mid, ab_lane_min): 8,192 1.69e9-1.70e9 vs 1.47e9-1.49e9;
    // 6,144 1.52e9-1.59e9 vs 1.45e9-1.46e9; 5,120 1.36e9 vs 1.41e9; 4,096 1.31e9 vs 1.41e9
    uint64_t chain_lane_min = 6144;
    // persistent lane-chain waves per dispatch, 0: a wave per 64 instances (BFTSIM_TESTING + BFTSIM_CHAIN_GRID; an A/B
    // arm: capping the chain waves so that the consensus kernels keep SIMD slots measured the same or slower)
    uint32_t chain_grid = 0;
    // lane chains encode each height's suffix themselves from the recorded rows: no suffix-row kernel on the launch
    // streams (0.3-0.45 ms per cfg3 launch beside the FAST kernels), no 400 MB of rows written and read back
    // (BFTSIM_TESTING + BFTSIM_CHAIN_INLINE=0: the suffix rows)
    uint32_t chain_inline = 1;
    // s_setprio of the chain waves (Params::chain_prio), against the FAST kernels' 2. Recorded chains: 0. Predicted
    // lane pairs (small shards, their latency the step's tail) above the FAST kernels, with their suffix rows, at the
    // sync's flush and at earlier ones alike: 2,048 per GPU 1.08e9 at 0, 1.13e9-1.22e9 at 3 (profiles/r06/ab_prio).
    // Predicted lanes (large shards: throughput, not latency) below them: cfg3 2.06e9-2.10e9 at 0 or 1 against
    // 1.80e9-1.93e9 at 3 (profiles/r06/ab_spec_lane).
    static constexpr uint32_t PRIO_RECORDED = 0, PRIO_SPEC_PAIR = 3, PRIO_SPEC_LANE = 0;
    bool seed_spec = true;            // little-endian seeds, N = 64: predicted blocks (BFTSIM_TESTING + BFTSIM_SEED_SPEC=0: off)
    int pipeline = 0;                 // number of row-table sets (0: no pipelining)
    uint32_t sfx_rows = 0;            // heights per hash-pass chunk (0: no hash pass)
    uint32_t n_sets = 0, cur_set = 0; // allocated sets; the ring cursor of the pipelined launches
    bool last_pipe = false;           // the last launch ran on the launch streams
    hipStream_t cs[MAX_CS] = {}, hstr[MAX_HS] = {};
    uint32_t n_cs = 2, n_hs = 2, cur_cs = 0, cur_hs = 0;
    // launch streams with little-endian seeds: a launch's seed chain and FAST kernel are serial on its stream
    // and there is no hash pass, so more launches run side by side (profiles/r04/ab_le_streams)
    static constexpr uint32_t N_CS_SEEDED = 4;
    uint32_t hash_batch = 4;          // launches per chain kernel (BFTSIM_TESTING + BFTSIM_HASH_BATCH overrides)
    // big-endian seeds, N = 64, pipelined: the chains of a batch run on predicted blocks from launch time on
    // (BFTSIM_TESTING + BFTSIM_HASH_SPEC=0: off), over up to N_HS_SPEC hash streams so that the
    // batches of a burst of launches run side by side
    // on at every size: a small shard's chains (lane pairs) are bound by their latency, which they start ahead
    // of; a large shard's (lanes, each predicting and encoding its blocks itself) fill the issue slots the consensus
    // kernels leave from the first launch on (cfg3: 2.06e9-2.10e9 against 1.94e9-1.98e9 recorded;
    // profiles/r06/ab_spec_lane). BFTSIM_TESTING + BFTSIM_HASH_SPEC=0: recorded chains at every size; =2: predicted
    // for lossy schedules too
    uint64_t hash_spec_max = ~0ull;
    bool spec_lossy = false;          // predicted chains with drops or crashes too (BFTSIM_HASH_SPEC=2)
    static constexpr uint32_t N_HS_SPEC = 3;
    struct Pending { uint32_t set, ev, first, cs; } pend[MAX_BATCH];   // cs: the launch stream it ran on
    // one event per chain batch (flush_batch) instead of one per set: a ring, re-recorded after BATCH_EVS batches. Safe
    // because BATCH_EVS > MAX_SETS: a batch marks at least one set, so more than MAX_SETS batches cannot all still be
    // some set's batch_done; by the time an event is re-recorded no set points at it
    static constexpr uint32_t BATCH_EVS = 64;
    static_assert(BATCH_EVS > MAX_SETS, "a re-recorded batch event must not be any set's batch_done");
    hipEvent_t batch_ev[BATCH_EVS] = {};
    uint32_t batch_ev_head = 0;
    uint32_t n_pend = 0;
    bft::Params batch_p{};            // the launch parameters of the pending batch (sizes, genesis, prio)
    bool batch_spec = false;          // the pending batch runs predicted chains
    uint32_t batch_hs = 0;            // the pending batch's hash stream (chosen at its first launch)
    // per-launch kernel timing: a ring of event quadruples, read by bftsim_kernel_ms_sum
    static constexpr uint32_t RING = 64;
    struct LaunchEv { hipEvent_t c0, c1, h0, h1, sx; bool has_hash, pending; } ring[RING] = {};
    uint32_t ring_head = 0;
    double acc_c = 0, acc_h = 0;
    uint32_t acc_n = 0;
    float archive_ms[4] = {0, 0, 0, 0};// the observer's passes, pick, emit + heights, copies of the last archive (SPEC.md §11e)
    float accuse_ms[4] = {0, 0, 0, 0}; // the observer's passes, walk, mark + scan + gather, copies of the last accuse (SPEC.md §11g)
    float timeline_ms[4] = {0, 0, 0, 0};// the observer's passes, walk, rows, copies of the last timeline (SPEC.md §11h)
    float rollcall_ms[6] = {0, 0, 0, 0, 0, 0};   // the observer's, the chronicler's, views, walk, scan + gather, copies (§11i)
};

#pragma GCC visibility push(hidden)

inline int fail(bftsim* h, int code, const std::string& msg) {
    if (h) h->err = msg;
    return code;
}
#define HIPCHECK(h, x)                                                                          \
    do {                                                                                        \
        hipError_t e_ = (x);                                                                    \
        if (e_ != hipSuccess) return fail(h, BFTSIM_EHIP, std::string(#x) + ": " + hipGetErrorString(e_)); \
    } while (0)

// a *_last_ms getter: the stored phase times into the caller's pointers, each of which may be null
inline int last_ms(const float* ms, std::initializer_list<float*> dst) {
    for (float* d : dst) {
        if (d) *d = *ms;
        ++ms;
    }
    return BFTSIM_OK;
}

// Owners of the cold paths' temporaries (verify, export, audit): released on every return, so that each HIP call
// there is a HIPCHECK with an early return. Not for the launch path, which owns nothing temporary.
struct DevMem {                       // a device allocation
    void* p = nullptr;
    DevMem() = default;
    DevMem(DevMem&& o) noexcept : p(o.release<void>()) {}
    DevMem(const DevMem&) = delete;
    DevMem& operator=(const DevMem&) = delete;
    ~DevMem() { (void)hipFree(p); }
    hipError_t alloc(size_t bytes) { return hipMalloc(&p, bytes); }
    template <class T> T* as() const { return (T*)p; }
    template <class T> T* release() { T* r = (T*)p; p = nullptr; return r; }   // the handle takes the allocation over
};
struct Events {                       // up to MAX timing events
    static constexpr int MAX = 6;
    hipEvent_t ev[MAX] = {};
    Events() = default;
    Events(const Events&) = delete;
    Events& operator=(const Events&) = delete;
    ~Events() { for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e); }
    hipError_t create(int n) {
        for (int k = 0; k < n && k < MAX; ++k)
            if (hipError_t e = hipEventCreate(&ev[k]); e != hipSuccess) return e;
        return hipSuccess;
    }
    hipEvent_t operator[](int k) const { return ev[k]; }
};

// libbftsig (include/bftsig.h), next to this library: the batched secp256k1 of real-crypto mode
struct SigApi {
    int (*create)(int, void**) = nullptr;
    void (*destroy)(void*) = nullptr;
    const char* (*last_error)(const void*) = nullptr;
    int (*secret_to_address)(void*, const uint8_t*, uint64_t, uint8_t*, uint8_t*, uint8_t*, void*) = nullptr;
    int (*sign)(void*, const uint8_t*, const uint32_t*, const uint8_t*, uint64_t, uint8_t*, uint8_t*, void*) = nullptr;
    int (*recover)(void*, const uint8_t*, const uint8_t*, uint64_t, uint8_t*, uint8_t*, uint8_t*, void*) = nullptr;
    bool ok = false;
    std::string why;
};
SigApi& sig_api();

// the kept trace's passes (bftsim.hip), which the observer's *_last_trace entry points run too
int trace_ready(bftsim* h, const char* what);
int trace_size_pass(bftsim* h);
int trace_emit(bftsim* h, const char* what, uint64_t m0, uint64_t m1, uint8_t* d_out, hipEvent_t t0, hipEvent_t t1);

#pragma GCC visibility pop
