/*
 * bftsim.h — C ABI of libbftsim, the MI355X-native batched PBFT simulator.
 *
 * This is the drop-in boundary for the reference's single-instance consensus path: one call runs
 * many independent, seeded consensus-rs clusters on a gfx950 GPU. The reference interfaces it
 * replaces (all paths in 2892931976/consensus-rs):
 *   - `trait Backend` (src/consensus/backend.rs:45-68) + `ImplBackend::{gossip,commit,verify}`
 *     (backend.rs:140-242): the N Cores of one cluster, their gossip and their chain commits
 *     become one instance simulated on the GPU;
 *   - `trait Engine` (src/consensus/consensus.rs:28-38) + `Minner` (src/minner/mod.rs:28-144):
 *     the height driver becomes the per-instance tick loop;
 *   - `trait ValidatorSet` / `ImplValidatorSet` (src/consensus/validator.rs:10-159): exported below
 *     as plain functions (quorum, proposer seed, sorted set);
 *   - the network entry `HandleMsgFn` (src/p2p/server.rs:45) / `handle_msg_middle`
 *     (src/consensus/pbft/core/core.rs:50-116): replaced by the seeded delivery schedule
 *     (SPEC.md §3).
 * Conventions (mirroring the reference's `Result`): every entry returns 0 on success and a
 * negative code on failure; `bftsim_last_error` explains the last failure. No exceptions or
 * panics cross the ABI. A handle is not thread-safe: use one handle per host thread / GPU.
 * Result buffers are caller-owned.
 */
#ifndef BFTSIM_H
#define BFTSIM_H
#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BFTSIM_OK 0
#define BFTSIM_EINVAL -1      /* bad configuration / arguments */
#define BFTSIM_EHIP -2        /* HIP runtime error */
#define BFTSIM_ENOMEM -3
#define BFTSIM_EUNSUPPORTED -4

/* result flags (per instance) */
#define BFTSIM_FLAG_SAFETY 1u        /* two different blocks committed at one height (frozen) */
#define BFTSIM_FLAG_PHASE_CAP 2u     /* messages dropped at the per-tick phase cap */
#define BFTSIM_FLAG_CORE_PANIC 4u    /* a Core panicked (core.rs:540 unwrap on no request) */
#define BFTSIM_FLAG_OUTBOX 8u        /* a second message of one kind in one phase was dropped */
#define BFTSIM_FLAG_TIMEOUT 16u      /* max_ticks reached before `heights` */
#define BFTSIM_FLAG_RCS_OVERFLOW 32u /* more round-change rounds than the set's capacity (bftsim_set_rcs_capacity) */
#define BFTSIM_FLAG_WINDOW 64u       /* windowed run: a lookup older than the row ring (result unpinned) */

/* Conventions the reference leaves to unvendored crates (SPEC.md §1, §7): they are
 * parity-unpinned, so they are explicit switches here rather than silent assumptions.
 *   seed_byte_order: how `U128::from(seed_buf)` reads the 16-byte buffer hash[0..8] ++ 0^8 in
 *     randon_seed (src/consensus/validator.rs:39-48; `bigint = "4.4.1"`, Cargo.toml:16).
 *     BE: seed = (BE64(hash[0..8]) * 2^64) mod N  (seed == 0 for every power-of-two N);
 *     LE: seed = LE64(hash[0..8]) mod N           (every N needs the block hash in-kernel).
 *   header_encoding: the StorageValue serialization of `Header` behind `hash()` (block.rs:76-80);
 *     only the compact rmp-serde form of SPEC.md §7 exists today.
 *   backlog_mode: what BackLogActor does with FutureMessage / FutureRoundMessage
 *     (src/consensus/pbft/core/back_log.rs:38-91). DROP is the reference (stored, never re-delivered);
 *     REPLAY is the opt-in liveness variant of SPEC.md §10 (not a parity target of the reference). */
#define BFTSIM_SEED_BE 0u
#define BFTSIM_SEED_LE 1u
#define BFTSIM_ENC_RMP_COMPACT 0u
#define BFTSIM_BACKLOG_DROP 0u
#define BFTSIM_BACKLOG_REPLAY 1u

typedef struct bftsim_config {
    uint32_t n;                  /* validators per instance: 1..256 */
    uint32_t heights;            /* stop once the canonical chain reaches this height */
    uint32_t max_ticks;          /* cap on ticks (a tick = block_period = RC timeout) */
    uint32_t block_period;       /* seconds (examples/c1.toml:6) */
    uint64_t genesis_time;       /* examples/c1.toml:15 */
    uint64_t seed;               /* Philox key (SPEC.md §5) */
    uint32_t drop_ppm;           /* per-link per-phase drop probability */
    uint32_t byz_count;          /* equivocating validators per instance (SPEC.md §6) */
    uint32_t proposer_crash_ppm; /* per-view probability that the proposer stays silent */
    uint32_t phase_cap;          /* max message phases per tick */
    uint64_t silent_mask[4];     /* validators that never run */
    const uint8_t *addresses;    /* n*20 bytes, ascending = validator index order */
    uint8_t genesis_proposer[20];
    uint64_t genesis_gas_used;
    uint32_t seed_byte_order;    /* BFTSIM_SEED_BE (default) | BFTSIM_SEED_LE */
    uint32_t header_encoding;    /* BFTSIM_ENC_RMP_COMPACT */
    uint32_t backlog_mode;       /* BFTSIM_BACKLOG_DROP (reference) | BFTSIM_BACKLOG_REPLAY */
    uint32_t reserved;           /* must be 0 */
} bftsim_config;

typedef struct bftsim_result {   /* host buffers, caller-owned; H = config.heights */
    uint64_t *committed_height;  /* [n_inst] canonical chain length (<= H) */
    uint32_t *flags;             /* [n_inst] */
    uint32_t *ticks;             /* [n_inst] ticks used */
    uint64_t *views;             /* [n_inst] instance-rounds: sum of (commit round + 1) */
    uint16_t *round;             /* [n_inst*H] round of the first commit of each height */
    uint16_t *proposer;          /* [n_inst*H] proposer index of the committed block */
    uint8_t *variant;            /* [n_inst*H] 1 = the equivocated second block */
    uint32_t *time_tick;         /* [n_inst*H] header.time = genesis + period*(tick+1) */
    uint8_t *block_hash;         /* [n_inst*H*32] Keccak-256 of the header (block.rs:76-80) */
    uint64_t capacity;           /* instances the buffers above hold: at least the instances the call
                                    writes (bftsim_run's n, bftsim_launched_count's n), else the call
                                    fails with BFTSIM_EINVAL and writes nothing */
} bftsim_result;

typedef struct bftsim_stats {    /* summed over the instances of the last launch */
    uint64_t instances;
    uint64_t committed_heights;
    uint64_t views;              /* instance-rounds */
    uint64_t ticks;
    uint64_t flagged[7];         /* instances with each flag bit set */
    uint64_t round_hist[65];     /* rounds-to-commit: heights committed in round 0..63, [64] = 64+ */
    uint64_t latency_hist[65];   /* commit latency: ticks between the records of heights x-1 and x
                                    (genesis = tick 0), [64] = 64+ */
} bftsim_stats;

typedef struct bftsim bftsim_t;

/* lifecycle */
int bftsim_create(const bftsim_config *cfg, int hip_device, bftsim_t **out);
void bftsim_destroy(bftsim_t *h);
const char *bftsim_last_error(bftsim_t *h);

/* synchronous: run instances [first, first+n) and copy results to host buffers */
int bftsim_run(bftsim_t *h, uint64_t first_instance, uint64_t n_instances, bftsim_result *out);

/* device-resident API (benchmarks): allocate once, launch many times, fetch on demand */
int bftsim_prepare(bftsim_t *h, uint64_t n_instances);
int bftsim_launch(bftsim_t *h, uint64_t first_instance, void *hip_stream);   /* async */
int bftsim_sync(bftsim_t *h);
int bftsim_fetch(bftsim_t *h, bftsim_result *out);
/* the instance range of the last launch [first, first + n): the count bftsim_fetch, _fetch_summary,
 * _export_headers, _export_ledger, _crypto_verify and _trace_sizes write per-instance rows for (n = 0: nothing
 * launched). Every one of those takes the capacity of the caller's buffers (in instances) and refuses a short one
 * with BFTSIM_EINVAL before writing anything (the reference's Result-returning boundary,
 * src/consensus/backend.rs:45-68) */
int bftsim_launched_count(bftsim_t *h, uint64_t *first_instance, uint64_t *n_instances);
int bftsim_stats_get(bftsim_t *h, bftsim_stats *out);   /* device reduction + copy */
/* multi-GPU (one process per GPU): the instances shard over the ranks with no data-path
 * collective; the statistics of every rank are summed by one RCCL all-reduce over xGMI. Rank 0 makes
 * the 128-byte id (ncclGetUniqueId) and the host hands it to every rank (any channel); each rank
 * then joins with its handle. Replaces the per-node Engine of create_bft_engine
 * (src/consensus/consensus.rs:42-60) with one engine per device and a node-wide statistic.
 * BFTSIM_EUNSUPPORTED when librccl.so.1 cannot be opened. */
/* 0 when librccl.so.1 opens with every entry point this library uses, else BFTSIM_EUNSUPPORTED. Every rank
 * calls it and the ranks agree on the answer (any channel) BEFORE any of them calls bftsim_comm_init:
 * ncclCommInitRank blocks until every rank has joined, so a rank that could not even open the library
 * would leave the others waiting there (bftsim/distributed.py capi_comm_init). */
int bftsim_comm_available(void);
int bftsim_comm_unique_id(uint8_t unique_id[128]);
int bftsim_comm_init(bftsim_t *h, int world_size, int rank, const uint8_t unique_id[128]);
/* bftsim_stats of the last launch summed over every rank (collective: every rank calls it) */
int bftsim_stats_allreduce(bftsim_t *h, bftsim_stats *out);
/* per-kernel device time of the last launch, from HIP events on the launch stream (ms) */
int bftsim_last_kernel_ms(bftsim_t *h, float *consensus_ms, float *hash_ms);
/* summed per-kernel device times (ms) of every launch since the previous call, without blocking
 * between launches (waits only for the launches being summed) */
int bftsim_kernel_ms_sum(bftsim_t *h, double *consensus_ms, double *hash_ms, uint32_t *launches);
/* pipelined launches (power-of-two N; with little-endian seeds at N = 64 too, whose launches carry their own
 * seed chain and no hash pass; the batch throughput mode of the benchmark): a ring of `on` row-table sets
 * (on = 1 means 2; 0 disables; at most 32), each with the scratch of one launch, so that up to `on` launches
 * are in flight. A launch's consensus kernel runs on one of two internal launch streams (four with
 * little-endian seeds) after the caller's earlier work on `hip_stream` and after its set's last hash
 * pass; the prev_hash chains of bftsim_set_hash_batch consecutive launches run as one kernel on one of two
 * internal hash streams (a chain is sequential in height: a launch's chains take ~1.5 ms however many
 * there are, so batching multiplies their throughput). Results of a launch are complete once bftsim_sync
 * returns (it also enqueues a partial hash batch); bftsim_fetch/_stats_get/_fetch_summary read the last
 * launch (and sync as they need). The HIP runtime needs a hardware queue per stream in use: with the defaults that
 * is six (the caller's, two launch and three hash streams; four launch streams with little-endian seeds), so
 * GPU_MAX_HW_QUEUES >= 6 in the environment before HIP initialises (HIP's default is 4; bench.py sets 8). Takes
 * effect at the next bftsim_prepare (buffers are re-allocated). */
int bftsim_set_pipeline(bftsim_t *h, int on);
/* pipelined launches: the number of consecutive launches whose block-hash chains run as one kernel (1..32,
 * default 4). A launch waiting for its batch is hashed when the batch fills, at bftsim_sync, or when the ring
 * needs its row-table set again. With big-endian seeds at N = 64 and a lossless schedule (no drops, no proposer
 * crashes) the chains of a batch run on the predicted canonical blocks as soon as the batch is flushed, and are
 * checked against the recorded blocks (and re-run from the first one that differs) once the batch's consensus
 * kernels are done. */
int bftsim_set_hash_batch(bftsim_t *h, uint32_t launches);
/* verification switch: 0 runs N = 64 through the full kernel alone instead of the FAST kernel +
 * resume (results are identical; the default 1 is the fast path) */
int bftsim_set_fast(bftsim_t *h, int on);
/* optional per-tick state digests of the next launch (debug; NULL disables) */
int bftsim_set_trace(bftsim_t *h, uint64_t *host_out, uint32_t trace_ticks);
/* windowed runs for long horizons (10,000 heights x 1M instances): keep only a ring
 * of `window` canonical rows per instance (power of two >= 64; 0 = every height, the default).
 * Block hashes are then computed in-kernel; per-height outputs are not kept (bftsim_fetch fails):
 * read bftsim_fetch_summary and the histograms of bftsim_stats_get. A lookup older than the ring
 * (a validator lagging > window heights) sets BFTSIM_FLAG_WINDOW. */
int bftsim_set_window(bftsim_t *h, uint32_t window);
/* RoundChangeSet capacity: distinct round-change rounds each validator keeps between two resets of its
 * set (the reference's HashMap<u64, MessageManage>, round_change_set.rs:11-35, is unbounded).
 * 1..4096, default 16. A validator needing more sets BFTSIM_FLAG_RCS_OVERFLOW on its instance;
 * bftsim_run then re-runs the batch at twice the capacity until no instance overflows (instances are
 * independent and deterministic, so the others are unchanged), as long as the doubled tables fit in 90 %
 * of the free device memory; otherwise it returns BFTSIM_OK with the flagged results. The grown capacity
 * stays in effect for later prepare / launch / run calls, with tables proportional to it (set it back
 * with this call). Takes effect at the next bftsim_prepare. */
int bftsim_set_rcs_capacity(bftsim_t *h, uint32_t rounds);
/* per-instance outputs of the last launch (any pointer may be NULL; capacity = instances each
 * buffer holds); tip_hash[i*32..] = hash of
 * the block at committed_height[i] (the genesis hash at 0), which commits to the whole chain */
int bftsim_fetch_summary(bftsim_t *h, uint64_t capacity, uint64_t *committed_height, uint32_t *flags, uint32_t *ticks,
                         uint64_t *views, uint8_t *tip_hash);

/* real-crypto mode (SPEC.md §11). Every consensus message the simulation
 * broadcasts is logged; bftsim_crypto_verify then does, batched on the GPU (libbftsig):
 *   - sign it with its sender's key (finalize_message, core.rs:425-429), the Commit seal first
 *     (encrypt_commit_bytes, types/votes.rs:94-101);
 *   - recover its signer and check membership (GossipMessage::address, protocol/mod.rs:103-116;
 *     handle_message, core.rs:314-322), and recover every seal (verify_commit, commit.rs:94-100).
 * A `forged` validator signs with a key that is not its own (keccak of its secret): every receiver
 * drops its consensus messages, which the simulation applies when they are sent. The verify pass
 * proves that assumption message by message (`mismatches` must be 0). Each message is recovered once,
 * as every receiver gets the same bytes (the reference recovers it at each receiver).
 * secrets32: host, n x 32 bytes in the sorted validator order; each must derive the address of its
 * index (else BFTSIM_EINVAL). forged: host, n bytes (NULL = none). log_cap: messages per instance
 * (0 = heights * (4n + 8) + 64n). NULL secrets turn the mode off. Takes effect at the next
 * bftsim_prepare. Needs libbftsig.so next to libbftsim.so; window 0; N = 64 runs the full kernel. */
typedef struct bftsim_crypto_report {
    uint64_t messages;             /* consensus messages broadcast (each signed once) */
    uint64_t seals;                /* Commit seals (signed, then recovered) */
    uint64_t forged;               /* messages of forged senders */
    uint64_t recovered_as_sender;  /* messages whose signature recovers their sender */
    uint64_t mismatches;           /* recovered validity != the simulated delivery: 0 */
    uint64_t seal_errors;          /* seals that do not recover */
    uint64_t signatures;           /* ECDSA signs performed: messages + seals */
    uint64_t recoveries;           /* ECDSA recoveries performed: messages + seals */
    uint64_t log_overflows;        /* instances whose log exceeded log_cap (then the call fails) */
} bftsim_crypto_report;
int bftsim_set_crypto(bftsim_t *h, const uint8_t *secrets32, const uint8_t *forged, uint32_t log_cap);
/* after a launch: the sign / recover pass of its messages; capacity = instances inst_checksum and
 * inst_messages hold (checked when either is non-NULL); inst_checksum (host, n x 32, nullable) =
 * per instance the XOR over its messages of keccak256(signature || seal or 65 zero bytes);
 * inst_messages (host, n, nullable) = messages per instance */
int bftsim_crypto_verify(bftsim_t *h, bftsim_crypto_report *out, uint64_t capacity, uint8_t *inst_checksum,
                         uint32_t *inst_messages);

/* the ledger with votes (real-crypto mode, after bftsim_crypto_verify): for every instance and height
 * x <= committed_height, in slot [i*H + x-1] of `slot_bytes` bytes, the Header that Backend::commit
 * inserts (backend.rs:163-174): the block's header (SPEC.md §7) with votes = the signatures of the
 * Commit messages in the committing Core's commit set at its commit (core.rs:402-413), ascending
 * validator order (or, after bftsim_set_ledger_votes(h, BFTSIM_VOTES_SEALS), those Commits' seals: the votes that
 * bftsim_verify_ledger can check). hdr_len = 0 beyond the committed height. The hash of a header is the run's
 * block_hash of that height (block_hash() ignores votes, types/block.rs:76-80). Together with
 * block_hash per height this is the ledger's headers + block_hashes_by_height (store/schema.rs). */
uint64_t bftsim_ledger_slot_bytes(uint32_t n_validators);
int bftsim_export_ledger(bftsim_t *h, uint64_t capacity, uint8_t *hdr, uint64_t slot_bytes, uint32_t *hdr_len);

/* the trace (real-crypto mode, SPEC.md §11b): the last launch's consensus traffic as the signed wire frames a
 * reference node would have read from its socket. A frame is what TcpServer::broadcast writes for one logged
 * broadcast: a 4-byte big-endian size, then RawMessage{Header{Consensus, ttl 10, create_time 0, peer_id None},
 * payload}, the payload being the GossipMessage{code, create_time, msg, signature: Some, commit_seal} bytes; msg is
 * Subject{view, digest} (Prepare, Commit, RoundChange) or PrePrepare{view, Block{header, transactions: []}}. Every
 * value is the one bftsim_crypto_verify derived and the signature the one it computed (nothing is signed twice); a
 * forged sender's frames are signed with keccak(secret). Every logged message has a frame, those dropped at the
 * phase cap or sent by forged validators included; Blocks and Sync messages are not logged.
 * bftsim_set_trace_keep (default 0): bftsim_crypto_verify keeps on the device what the export needs (each message's
 * signature, each Commit's seal, the digests and the dense message index) until the next launch, prepare or
 * destroy; its results are the same either way. */
int bftsim_set_trace_keep(bftsim_t *h, int on);
/* exact sizes of the last launch's trace (after bftsim_crypto_verify with keep on): frames and stream bytes per
 * instance (either may be NULL); capacity = instances the buffers hold */
int bftsim_trace_sizes(bftsim_t *h, uint64_t capacity, uint32_t *inst_frames, uint64_t *inst_bytes);
/* the frames of instances [inst_begin, inst_begin + inst_count) of the last launch (indices into the launch), so
 * that a large trace can be pulled in pieces; the device stream is allocated per call for that range. Host buffers:
 *   stream      [stream_cap bytes] the frames back to back, instance by instance, in broadcast-log order
 *   frame_off   [frame_cap + 1] byte offset of each frame in `stream`, then the total (what bftwire_split_frames
 *               returns for the stream)
 *   frame_meta  nullable, [frame_cap][4]: log word 0 (tick), log word 1 (phase | code << 8 | sender << 16),
 *               log word 6 (flags: 1 forged, 2 wildcard digest, 4 equivocation, 8 old-block commit), instance
 *               index relative to inst_begin
 *   inst_frame0 nullable, [inst_count + 1] first frame index of each instance, then the frame count
 * BFTSIM_EINVAL, with nothing written, when keep is off, no bftsim_crypto_verify ran since the launch, the range is
 * outside the launch, or stream_cap / frame_cap is below the range's bytes / frames. BFTSIM_EHIP, with nothing
 * written, if the emit pass disagrees with the size pass on any frame's length. */
int bftsim_export_trace(bftsim_t *h, uint64_t inst_begin, uint64_t inst_count, uint8_t *stream, uint64_t stream_cap,
                        uint64_t *frame_off, uint64_t frame_cap, uint32_t *frame_meta, uint64_t *inst_frame0);
/* diagnostics, not part of the export's contract: device times (ms, HIP events) of the trace's last size pass + scan,
 * emit kernel and device-to-host copies, as scripts/trace_bench.py records them */
int bftsim_trace_last_ms(bftsim_t *h, float *size_ms, float *emit_ms, float *copy_ms);

/* Twins (SPEC.md §11f): an equivocator's second frames. A Byzantine validator sends variant 0 of its block to some
 * receivers and variant 1 to the others, and its votes count for both variants; the log, and so the trace, holds
 * one entry for each. bftsim_set_trace_twins (default 0; any value but 0 or 1 is BFTSIM_EINVAL) is read by the next
 * bftsim_crypto_verify that runs with bftsim_set_trace_keep on (with keep off it has no effect): the kept trace then
 * carries, immediately behind every equivocating PrePrepare (flag 4) and behind every wildcard Prepare / Commit
 * (flag 2) of a valid block above height 0 whose proposer is one of the instance's Byzantine validators, one more
 * frame, the twin: the same message (code, view, create_time, sender, signing key) for the block's other variant,
 * with that variant's digest (header, for a PrePrepare), its own commit seal and its own signature. frame_meta word 2
 * of a twin is its original's flags with bit 16 set; words 0, 1 and 3 are the original's. bftsim_trace_sizes,
 * bftsim_export_trace, bftsim_audit_last_trace and bftsim_archive_last_trace see the twins in place. Twins are not
 * log entries: the report and checksums of bftsim_crypto_verify, bftsim_export_ledger, bftsim_fetch and the statistics
 * are the same with twins on and off. */
int bftsim_set_trace_twins(bftsim_t *h, int on);
/* the twins of the last kept trace: those of PrePrepares and those of votes (either may be NULL); 0 and 0 for a trace
 * kept with twins off. BFTSIM_EINVAL, with nothing written, whenever bftsim_export_trace would refuse for lack of a
 * kept trace. */
int bftsim_trace_twin_counts(bftsim_t *h, uint64_t *pp_twins, uint64_t *vote_twins);
/* diagnostics: device times (ms, HIP events) of the last verify's twin passes: mark + scan + merge (with the host's
 * round trip for the count), the digest kernels, the signing; as scripts/trace_bench.py --twins records them */
int bftsim_trace_twins_last_ms(bftsim_t *h, float *index_ms, float *digest_ms, float *sign_ms);

/* the observer (SPEC.md §11c): a frame stream in the export's format, audited from its bytes on the device. Per frame:
 * decode (every read bounded by the frame's span in frame_off; the bytes are untrusted), the sign payload rebuilt from
 * the decoded fields with signature None, its signer recovered and looked up in the handle's validator set, and for a
 * Commit the seal (keccak(0x03 || digest), types/votes.rs:94-101) recovered and compared with the signer. Per
 * instance, in frame order, over the accepted frames (status OK or SEAL_FOREIGN): a tally of the Commit votes per
 * (height, round, digest), a commit certificate per height (the first key whose voters exceed
 * bftsim_two_thirds_majority(N)) and a safety verdict (a second digest with a quorum at a certified height).
 * The validator set, N and seed_byte_order are the handle's config; no secrets are needed and bftsim_set_crypto need
 * not have been called (libbftsig.so must be next to libbftsim.so). The handle's run state is untouched.
 * frame status (one byte per frame, the first matching row wins): */
#define BFTSIM_AUDIT_OK 0u             /* decodes; the signature recovers to validator `signer`; a Commit's seal too */
#define BFTSIM_AUDIT_UNDECODABLE 1u    /* span under 4 bytes or size prefix != span - 4; not a Consensus RawMessage; the
                                          GossipMessage or its msg does not parse or has trailing bytes; code outside
                                          1..4; signature None; a Commit without a seal, another message with one */
#define BFTSIM_AUDIT_UNRECOVERABLE 2u  /* the signature does not recover */
#define BFTSIM_AUDIT_NOT_VALIDATOR 3u  /* it recovers to an address outside the set (every forged sender's frame) */
#define BFTSIM_AUDIT_SEAL_BAD 4u       /* Commit whose seal does not recover (dropped by the reference, commit.rs:94-100) */
#define BFTSIM_AUDIT_SEAL_FOREIGN 5u   /* Commit whose seal recovers to another address: accepted, counted apart */
/* instance flags */
#define BFTSIM_AUDIT_KEY_OVERFLOW 1u   /* a frame's key was absent from a full key table: the frame was ignored */
#define BFTSIM_AUDIT_CONFLICT 2u       /* two digests with a quorum of Commits at one height (wire-level BFTSIM_FLAG_SAFETY) */
struct bftsim_audit_report {
    uint64_t frames, ok, undecodable, unrecoverable, not_validator, seal_bad, seal_foreign;
    uint64_t by_code[4];        /* accepted frames per MessageType */
    uint64_t out_of_range;      /* accepted PrePrepare/Commit frames with height 0 or > max_heights */
    uint64_t certified;         /* (instance, height) pairs with a certificate */
    uint64_t conflicts, key_overflows;
    uint64_t recoveries;        /* ECDSA recoveries performed */
};
typedef struct bftsim_audit_report bftsim_audit_report;
struct bftsim_audit_out {       /* host, caller-owned, any pointer may be NULL */
    uint8_t *frame_status; int32_t *frame_signer;                 /* [frames]; signer: validator index for status 0, 4, 5, else -1 */
    uint32_t *inst_flags;                                          /* [inst_count] BFTSIM_AUDIT_KEY_OVERFLOW | _CONFLICT */
    uint16_t *cert_round; uint8_t *cert_digest; uint64_t *cert_voters;
    uint32_t *cert_frame; uint8_t *cert_flags;                     /* [inst_count * max_heights] (x32, x4), row
                                                                      inst * max_heights + height - 1: round (0xffff:
                                                                      no certificate; rounds above 0xfffe read 0xfffe),
                                                                      digest, voter bitmap, the completing frame's index
                                                                      within the instance, flags (1 proposed before
                                                                      completion, 2 by the rightful proposer) */
};
typedef struct bftsim_audit_out bftsim_audit_out;
/* stream [stream_bytes]: frames back to back; frame_off [frames + 1]: byte offset of each frame, then the total;
 * inst_frame0 [inst_count + 1]: first frame of each instance, then the frame count (what bftsim_export_trace writes).
 * key_cap: keys per instance's table (0 = 4 * max_heights + 64); nothing is evicted. Arguments are checked before
 * any device work and a refused call writes nothing: BFTSIM_EINVAL for a null handle, report, frame_off or
 * inst_frame0, a frame_off that decreases or does not end at stream_bytes, an inst_frame0 that decreases or does not
 * run from 0 to frames, max_heights of 0 or above 65,535, 2^32 frames or more, 2^31 instances or more. Hostile frame
 * contents are never an error of the call: they become statuses. */
int bftsim_audit_trace(bftsim_t *h, const uint8_t *stream, uint64_t stream_bytes, const uint64_t *frame_off, uint64_t frames,
                       const uint64_t *inst_frame0, uint64_t inst_count, uint32_t max_heights, uint32_t key_cap,
                       const bftsim_audit_out *out, bftsim_audit_report *report);
/* the kept trace of the last launch (bftsim_set_trace_keep on, after bftsim_crypto_verify), instances
 * [inst_begin, inst_begin + inst_count): emitted and audited on the device, no stream copy to the host;
 * frame counts as bftsim_trace_sizes gives them; max_heights = config.heights. Refuses what bftsim_export_trace
 * refuses. */
int bftsim_audit_last_trace(bftsim_t *h, uint64_t inst_begin, uint64_t inst_count, uint32_t key_cap,
                            const bftsim_audit_out *out, bftsim_audit_report *report);
/* diagnostics: device times (ms, HIP events) of the last audit's decode kernel, recoveries, classification + tally, and
 * copies (the stream to the device, the outputs back), as scripts/audit_bench.py records them */
int bftsim_audit_last_ms(bftsim_t *h, float *decode_ms, float *recover_ms, float *tally_ms, float *copy_ms);

/* the archiver (SPEC.md §11e): what a node that only listened can write down of the chain it saw. The observer's passes,
 * then for every certified height the ledger Header assembled on the device from the bytes alone: the 12 leading fields of
 * the block in the first accepted PrePrepare frame of that height whose digest is the certificate's, re-encoded
 * canonically, and as votes the commit seals of the Commit frames that set the certificate's voter bits, ascending by
 * validator, each as it was received. The output has the slot layout of bftsim_export_ledger, so bftsim_verify_ledger
 * takes it as is. */
#define BFTSIM_ARCHIVE_OK 0u          /* the slot holds the header */
#define BFTSIM_ARCHIVE_NONE 1u        /* the height has no certificate: hdr_len 0 */
#define BFTSIM_ARCHIVE_NO_PROPOSAL 2u /* certified, but the instance has no accepted PrePrepare frame with the
                                         certificate's (height, digest): hdr_len 0 */
struct bftsim_archive_report {
    uint64_t headers;               /* slots written */
    uint64_t by_status[3];
    uint64_t votes;                 /* seals written */
    uint64_t foreign_seals;         /* of those, taken from BFTSIM_AUDIT_SEAL_FOREIGN frames */
    uint64_t archived_instances;    /* instances whose OK slots form a prefix and the rest are NONE */
};
typedef struct bftsim_archive_report bftsim_archive_report;
struct bftsim_archive_out {         /* host, caller-owned, any pointer may be NULL; rows inst * max_heights + x - 1 */
    uint8_t *status;                /* BFTSIM_ARCHIVE_* */
    uint32_t *pp_frame;             /* the PrePrepare frame used (index within the instance), 0xffffffff if none */
    uint16_t *n_votes;              /* seals in the slot (0 unless OK) */
    uint64_t *archived_height;      /* [inst_count] the largest x with slots 1..x all OK */
};
typedef struct bftsim_archive_out bftsim_archive_out;
/* stream .. key_cap, audit_out and audit_report (both nullable): as bftsim_audit_trace, whose refusals are this call's
 * and whose outputs those two receive unchanged. hdr [inst_count * max_heights * slot_bytes] / hdr_len
 * [inst_count * max_heights]: host buffers, slot i * max_heights + x - 1; of a slot only its first
 * bftsim_ledger_slot_bytes(config.n) bytes are written (the header, then zeros). BFTSIM_EINVAL too for a null hdr,
 * hdr_len or report and for slot_bytes below bftsim_ledger_slot_bytes(config.n); BFTSIM_ENOMEM for 2^31 slots or more. A
 * refused call writes nothing; hostile frame contents are never an error; the handle's run state is untouched; no
 * secrets are needed. A header that would not fit its slot fails the call with BFTSIM_EHIP before any copy to the host. */
int bftsim_archive_trace(bftsim_t *h, const uint8_t *stream, uint64_t stream_bytes, const uint64_t *frame_off, uint64_t frames,
                         const uint64_t *inst_frame0, uint64_t inst_count, uint32_t max_heights, uint32_t key_cap,
                         uint8_t *hdr, uint64_t slot_bytes, uint32_t *hdr_len, const bftsim_archive_out *out,
                         const bftsim_audit_out *audit_out, bftsim_audit_report *audit_report,
                         bftsim_archive_report *report);
/* the same over the kept trace of the last launch, as bftsim_audit_last_trace: the stream never leaves the device */
int bftsim_archive_last_trace(bftsim_t *h, uint64_t inst_begin, uint64_t inst_count, uint32_t key_cap, uint8_t *hdr,
                              uint64_t slot_bytes, uint32_t *hdr_len, const bftsim_archive_out *out,
                              const bftsim_audit_out *audit_out, bftsim_audit_report *audit_report,
                              bftsim_archive_report *report);
/* diagnostics: device times (ms, HIP events) of the last archive call: the observer's passes (decode, recoveries,
 * classification + tally), the pick kernel, the emit and heights kernels, and the copies, as scripts/archive_bench.py
 * records them */
int bftsim_archive_last_ms(bftsim_t *h, float *audit_ms, float *pick_ms, float *emit_ms, float *copy_ms);

/* the accuser (SPEC.md §11g): who misbehaved, and what proves it. The observer's passes, then per instance over the
 * frames it accepts (status OK or SEAL_FOREIGN) that are a PrePrepare, Prepare or Commit at a height in 1..max_heights:
 * a group is (signer, code, height, round), the round as the full u64; a group whose frames carry two digests yields one
 * evidence record, frame_a the group's first frame in stream order and frame_b its first frame with another digest.
 * The two frames prove the fault to anyone who has the validator set: both decode, both recover to the same validator,
 * and they differ in the digest alone among (code, height, round, digest). Further digests and repeats add nothing.
 * Records are ordered by frame_b ascending. */
#define BFTSIM_ACCUSE_VIEW_OVERFLOW 1u /* instance flag: a frame's (height, round) was absent from a full view table:
                                          the frame was ignored */
struct bftsim_accuse_record {       /* 32 bytes; frame_a < frame_b, both indices among the call's frames */
    uint64_t round;
    uint32_t inst, height, signer, code, frame_a, frame_b;
};
typedef struct bftsim_accuse_record bftsim_accuse_record;
struct bftsim_accuse_report {
    uint64_t records;               /* evidence records found (of which min(records, rec_cap) were written) */
    uint64_t by_code[3];            /* of PrePrepares, Prepares, Commits */
    uint64_t accused;               /* (instance, validator) pairs accused: the popcounts of inst_accused */
    uint64_t accused_instances;     /* instances with a record */
    uint64_t view_overflows;        /* instances with BFTSIM_ACCUSE_VIEW_OVERFLOW */
};
typedef struct bftsim_accuse_report bftsim_accuse_report;
struct bftsim_accuse_out {          /* host, caller-owned, any pointer may be NULL */
    uint32_t *frame_pair;           /* [frames] frame_a of the record whose frame_b this frame is, else 0xffffffff */
    uint64_t *inst_accused;         /* [inst_count * 4] bitmap of the validators that sign a record of the instance */
    uint32_t *inst_flags;           /* [inst_count] BFTSIM_ACCUSE_VIEW_OVERFLOW */
    bftsim_accuse_record *records;  /* [rec_cap] the first min(report.records, rec_cap) records */
    uint64_t rec_cap;               /* 0 with records NULL */
};
typedef struct bftsim_accuse_out bftsim_accuse_out;
/* stream .. key_cap, audit_out and audit_report (both nullable): as bftsim_audit_trace, whose refusals are this call's
 * and whose outputs those two receive unchanged. view_cap: (height, round) pairs per instance's table (0 =
 * 2 * max_heights + 64); nothing is evicted. BFTSIM_EINVAL too for a null out or report and for a rec_cap above 0 with
 * records NULL; BFTSIM_ENOMEM, before anything is launched, for tables the device cannot hold. A refused call writes
 * nothing; hostile frame contents are never an error; the handle's run state is untouched; no secrets are needed. */
int bftsim_accuse_trace(bftsim_t *h, const uint8_t *stream, uint64_t stream_bytes, const uint64_t *frame_off, uint64_t frames,
                        const uint64_t *inst_frame0, uint64_t inst_count, uint32_t max_heights, uint32_t key_cap,
                        uint32_t view_cap, const bftsim_accuse_out *out, const bftsim_audit_out *audit_out,
                        bftsim_audit_report *audit_report, bftsim_accuse_report *report);
/* the same over the kept trace of the last launch, as bftsim_audit_last_trace: the stream never leaves the device */
int bftsim_accuse_last_trace(bftsim_t *h, uint64_t inst_begin, uint64_t inst_count, uint32_t key_cap, uint32_t view_cap,
                             const bftsim_accuse_out *out, const bftsim_audit_out *audit_out,
                             bftsim_audit_report *audit_report, bftsim_accuse_report *report);
/* diagnostics: device times (ms, HIP events) of the last accuse call: the observer's passes (decode, recoveries,
 * classification + tally), the walk kernel, mark + scan + gather, and the copies, as scripts/accuse_bench.py records
 * them */
int bftsim_accuse_last_ms(bftsim_t *h, float *audit_ms, float *walk_ms, float *compact_ms, float *copy_ms);

/* the chronicler (SPEC.md §11h): how a height got to its certificate, or where an instance stopped. The observer's
 * passes, then per instance over the frames it accepts (status OK or SEAL_FOREIGN) that are a Prepare or a RoundChange
 * at a height in 1..max_heights: a Prepare votes in the key (height, round, digest), a RoundChange in the key
 * (height, round) whatever digest it carries (round_change.rs:78-92 never reads it), the round as the full u64, a
 * signer once per key. A key has a quorum when its distinct voters exceed bftsim_two_thirds_majority(n). Per
 * (instance, height) the first Prepare key to reach one is described as it stood at the completing frame, the others
 * are counted, and three flags join the row to the observer's certificate row of the same call. Rounds in the rows
 * are clipped as cert_round is (above 0xfffe: 0xfffe; 0xffff: none); frame indices are within the instance. */
#define BFTSIM_TIMELINE_KEY_OVERFLOW 1u   /* instance flag: a frame's key was absent from a full table: the frame was
                                             ignored */
#define BFTSIM_TIMELINE_PREPARED_FIRST 1u /* row flag: the height has a commit certificate, and a Prepare key with its
                                             digest and the full round of the frame cert_frame reached its quorum at a
                                             frame below cert_frame */
#define BFTSIM_TIMELINE_CERT_UNPREPARED 2u /* row flag: the height has a commit certificate, and no Prepare key with its
                                              digest, at any round, reaches a quorum in the instance (prepare.rs:59) */
#define BFTSIM_TIMELINE_LOCKED_OPEN 4u    /* row flag: a prepare quorum and no commit certificate */
struct bftsim_timeline_report {
    uint64_t prepare_frames;        /* accepted Prepares with a height in range, those ignored for a full table too */
    uint64_t rc_frames;             /* accepted RoundChanges with a height in range, those ignored for a full table
                                       too: it exceeds the sum of bftsim_timeline_out.rc_frames, which counts only
                                       the tallied ones, by the RoundChanges that BFTSIM_TIMELINE_KEY_OVERFLOW ignored */
    uint64_t out_of_range;          /* accepted Prepares and RoundChanges at height 0 or above max_heights */
    uint64_t prepared;              /* rows with a prepare quorum */
    uint64_t rc_quorums;            /* RoundChange keys that reached a quorum */
    uint64_t rc_heights;            /* rows with at least one of them */
    uint64_t prepared_first;        /* rows with BFTSIM_TIMELINE_PREPARED_FIRST */
    uint64_t cert_unprepared;       /* rows with BFTSIM_TIMELINE_CERT_UNPREPARED */
    uint64_t locked_open;           /* rows with BFTSIM_TIMELINE_LOCKED_OPEN */
    uint64_t key_overflows;         /* instances with BFTSIM_TIMELINE_KEY_OVERFLOW */
};
typedef struct bftsim_timeline_report bftsim_timeline_report;
struct bftsim_timeline_out {        /* host, caller-owned, any pointer may be NULL; rows = inst_count * max_heights,
                                       row inst * max_heights + height - 1 */
    uint16_t *prep_round;           /* [rows] the round of the first Prepare key to reach a quorum, 0xffff: none */
    uint8_t *prep_digest;           /* [rows * 32] its digest */
    uint64_t *prep_voters;          /* [rows * 4] its voters at the completing frame */
    uint32_t *prep_frame;           /* [rows] the completing frame (0 without a quorum) */
    uint16_t *prep_quorums;         /* [rows] Prepare keys of the height that reached a quorum, saturating */
    uint16_t *rc_quorums;           /* [rows] RoundChange keys of the height that reached a quorum, saturating */
    uint16_t *rc_max_round;         /* [rows] the greatest round among them, 0xffff: none */
    uint32_t *rc_max_frame;         /* [rows] the frame that completed that key's quorum (0 without one) */
    uint16_t *rc_top_round;         /* [rows] the greatest round a tallied RoundChange of the height names, 0xffff: none */
    uint32_t *rc_frames;            /* [rows] the tallied RoundChanges of the height */
    uint8_t *flags;                 /* [rows] BFTSIM_TIMELINE_PREPARED_FIRST | _CERT_UNPREPARED | _LOCKED_OPEN */
    uint32_t *inst_flags;           /* [inst_count] BFTSIM_TIMELINE_KEY_OVERFLOW */
    uint32_t *open_height;          /* [inst_count] the smallest height without a commit certificate, max_heights + 1
                                       if every height has one */
};
typedef struct bftsim_timeline_out bftsim_timeline_out;
/* stream .. key_cap, audit_out and audit_report (both nullable): as bftsim_audit_trace, whose refusals are this call's
 * and whose outputs those two receive unchanged. tl_cap: keys per instance's table (0 = 4 * max_heights + 64); nothing
 * is evicted. Every counted frame is matched against all keys its instance holds so far, as the observer's are under
 * key_cap: a stream with many distinct (height, round) pairs costs frames x min(keys, tl_cap) comparisons per instance,
 * so tl_cap is also the bound on what a hostile stream can make the walk cost; raise it only for streams whose rounds
 * are known to run that far. BFTSIM_EINVAL too for a null out or report; BFTSIM_ENOMEM, before anything is launched, for tables the
 * device cannot hold. A refused call writes nothing; hostile frame contents are never an error; the handle's run state
 * is untouched; no secrets are needed. */
int bftsim_timeline_trace(bftsim_t *h, const uint8_t *stream, uint64_t stream_bytes, const uint64_t *frame_off, uint64_t frames,
                          const uint64_t *inst_frame0, uint64_t inst_count, uint32_t max_heights, uint32_t key_cap,
                          uint32_t tl_cap, const bftsim_timeline_out *out, const bftsim_audit_out *audit_out,
                          bftsim_audit_report *audit_report, bftsim_timeline_report *report);
/* the same over the kept trace of the last launch, as bftsim_audit_last_trace: the stream never leaves the device */
int bftsim_timeline_last_trace(bftsim_t *h, uint64_t inst_begin, uint64_t inst_count, uint32_t key_cap, uint32_t tl_cap,
                               const bftsim_timeline_out *out, const bftsim_audit_out *audit_out,
                               bftsim_audit_report *audit_report, bftsim_timeline_report *report);
/* diagnostics: device times (ms, HIP events) of the last timeline call: the observer's passes (decode, recoveries,
 * classification + tally), the walk kernel, the rows kernel, and the copies, as scripts/timeline_bench.py records
 * them */
int bftsim_timeline_last_ms(bftsim_t *h, float *audit_ms, float *walk_ms, float *rows_ms, float *copy_ms);

/* the roll call (SPEC.md §11i): which validator failed to do its job. The observer's passes and the chronicler's walk,
 * then per instance over the frames the observer accepts (status OK or SEAL_FOREIGN, code 1..4) at a height in
 * 1..max_heights: per validator what it signed, and per view the wire proves started — (x, 0) at x = 1 or above a
 * commit certificate of x - 1, (x, r > 0) at a quorate RoundChange key of the chronicler — the proposer
 * (seed(parent) + r mod n) mod n under the handle's seed_byte_order, with the genesis hash or the certificate digest of
 * x - 1 as the parent, and whether a counting PrePrepare of that proposer at (x, r) is in the instance. Rounds are the
 * full u64; frame indices are within the instance. */
#define BFTSIM_ROLLCALL_PROPOSED 1u       /* outcome: the proposer's PrePrepare at the view is in the instance */
#define BFTSIM_ROLLCALL_MISSED 2u         /* outcome: it is not */
#define BFTSIM_ROLLCALL_UNATTRIBUTED 3u   /* outcome: height - 1 has no certificate, so the proposer is unknown */
#define BFTSIM_ROLLCALL_WON 0x100u        /* added to PROPOSED: the height's certificate was completed at this round, and
                                             one of those PrePrepares carries its digest */
#define BFTSIM_ROLLCALL_PARTIAL 1u        /* instance flag: the chronicler's key table overflowed (tl_cap): RoundChange
                                             quorums, and their views, may be missing; what was found stands */
struct bftsim_rollcall_record {     /* one due view */
    uint64_t round;
    uint32_t inst, height;
    uint32_t proposer;              /* 0xffffffff: unattributed */
    uint32_t outcome;               /* BFTSIM_ROLLCALL_PROPOSED (| _WON), _MISSED or _UNATTRIBUTED */
    uint32_t start_frame;           /* the frame that proves the start: the certificate frame of height - 1 (round 0),
                                       the RoundChange key's completing frame (round > 0); 0xffffffff for (1, 0) */
    uint32_t pp_frame;              /* the first counting PrePrepare of the proposer at the view, 0xffffffff: none */
};
typedef struct bftsim_rollcall_record bftsim_rollcall_record;
struct bftsim_rollcall_report {
    uint64_t frames;                /* counting frames */
    uint64_t out_of_range;          /* accepted frames at height 0 or above max_heights */
    uint64_t views;                 /* due views, whatever rec_cap */
    uint64_t by_outcome[3];         /* PROPOSED (with or without WON), MISSED, UNATTRIBUTED */
    uint64_t won;                   /* views with BFTSIM_ROLLCALL_WON */
    uint64_t silent;                /* (instance, validator) pairs without a counting frame */
    uint64_t silent_instances;      /* instances with at least one */
    uint64_t partial_instances;     /* instances with BFTSIM_ROLLCALL_PARTIAL */
};
typedef struct bftsim_rollcall_report bftsim_rollcall_report;
struct bftsim_rollcall_out {        /* host, caller-owned, any pointer may be NULL; rows = inst_count * n, row inst * n + v */
    uint32_t *frames;               /* [rows * 4] the counting frames v signed, by code 1..4 */
    uint32_t *last_height;          /* [rows] the greatest height among them, 0: none */
    uint32_t *last_frame;           /* [rows] v's last counting frame, 0xffffffff: none */
    uint32_t *due;                  /* [rows] the instance's attributed views whose proposer is v */
    uint32_t *proposed;             /* [rows] those with outcome PROPOSED */
    uint32_t *missed;               /* [rows] those with outcome MISSED */
    uint32_t *won;                  /* [rows] those with WON */
    uint32_t *inst_views;           /* [inst_count] due views of the instance */
    uint64_t *inst_silent;          /* [inst_count * 4] bitmap of the validators without a counting frame */
    uint32_t *inst_flags;           /* [inst_count] BFTSIM_ROLLCALL_PARTIAL */
    bftsim_rollcall_record *records;/* [rec_cap] the first min(report.views, rec_cap) views, instance-major, within an
                                       instance by (height, round) ascending */
    uint64_t rec_cap;
};
typedef struct bftsim_rollcall_out bftsim_rollcall_out;
/* stream .. key_cap, audit_out and audit_report (both nullable): as bftsim_audit_trace, whose refusals are this call's
 * and whose outputs those two receive unchanged; tl_cap, timeline_out and timeline_report (both nullable): as
 * bftsim_timeline_trace, likewise. An instance has at most max_heights + tl_cap views, and its table has that many
 * slots. BFTSIM_EINVAL too for a null out or report, for rec_cap above 0 without records, and for a handle of more than
 * 256 validators; BFTSIM_ENOMEM, before anything is launched, for tables the device cannot hold. A refused call writes
 * nothing; hostile frame contents are never an error (a RoundChange quorum at round 2^60 is one view); the handle's run
 * state is untouched; no secrets are needed. */
int bftsim_rollcall_trace(bftsim_t *h, const uint8_t *stream, uint64_t stream_bytes, const uint64_t *frame_off, uint64_t frames,
                          const uint64_t *inst_frame0, uint64_t inst_count, uint32_t max_heights, uint32_t key_cap,
                          uint32_t tl_cap, const bftsim_rollcall_out *out, bftsim_rollcall_report *report,
                          const bftsim_audit_out *audit_out, bftsim_audit_report *audit_report,
                          const bftsim_timeline_out *timeline_out, bftsim_timeline_report *timeline_report);
/* the same over the kept trace of the last launch, as bftsim_audit_last_trace: the stream never leaves the device */
int bftsim_rollcall_last_trace(bftsim_t *h, uint64_t inst_begin, uint64_t inst_count, uint32_t key_cap, uint32_t tl_cap,
                               const bftsim_rollcall_out *out, bftsim_rollcall_report *report,
                               const bftsim_audit_out *audit_out, bftsim_audit_report *audit_report,
                               const bftsim_timeline_out *timeline_out, bftsim_timeline_report *timeline_report);
/* diagnostics: device times (ms, HIP events) of the last roll call: the observer's passes, the chronicler's walk + rows,
 * then the views kernel, the walk kernel (with its fold), scan + gather, and the copies, as scripts/rollcall_bench.py
 * records them */
int bftsim_rollcall_last_ms(bftsim_t *h, float *audit_ms, float *timeline_ms, float *views_ms, float *walk_ms,
                            float *gather_ms, float *copy_ms);

/* the importer (SPEC.md §11d): what a syncing node runs on every Header it is handed, Engine::verify_header with
 * seal = true and verify_seal (src/consensus/backend.rs:319-367), batched: every header of every instance's ledger,
 * verified from untrusted bytes on the device.
 * A vote that can be verified from its header is a commit seal, sign(keccak(0x03 || block hash)) (types/votes.rs:68-101):
 * it depends on the block alone. The reference's Core::commit hands Backend::commit the Commit messages' signatures
 * instead (core.rs:402-413), whose payload holds a round and a seal that the header does not carry. So the votes the
 * ledger keeps are a switch, read by the next bftsim_crypto_verify (which gathers them; still one 65-byte table): */
#define BFTSIM_VOTES_SIGNATURES 0u     /* the Commit messages' signatures, as the reference stores them (default) */
#define BFTSIM_VOTES_SEALS 1u          /* the Commits' seals, a.k.a. what verify_seal recovers */
/* any other kind is BFTSIM_EINVAL; slot layout, order and bftsim_ledger_slot_bytes of bftsim_export_ledger are the same */
int bftsim_set_ledger_votes(bftsim_t *h, uint32_t kind);
/* header status (one byte per slot). The checks run in the reference's order and the first that fails wins; verify_seal
 * checks its votes' signatures before it counts them, so BAD_VOTE is decided before the LACK_VOTES of too few voters: */
#define BFTSIM_LEDGER_OK 0u            /* every check below passes */
#define BFTSIM_LEDGER_ABSENT 1u        /* hdr_len = 0 */
#define BFTSIM_LEDGER_UNDECODABLE 2u   /* hdr_len > slot_bytes (nothing is read); not a SPEC.md §7 Header of 11..13 fields
                                          (extra above 32 bytes included) or trailing bytes; a vote that is not 65 bytes;
                                          more than 256 votes */
#define BFTSIM_LEDGER_BAD_HEIGHT 3u    /* header.height is 0 (InvalidHeight) or is not the slot's x */
#define BFTSIM_LEDGER_NO_PARENT 4u     /* x > 1 and slot x - 1 is ABSENT or UNDECODABLE (UnknownAncestor) */
#define BFTSIM_LEDGER_BAD_PARENT 5u    /* prev_hash != the parent's block hash */
#define BFTSIM_LEDGER_BAD_TIME 6u      /* time < parent.time + block_period (InvalidTimestamp) */
#define BFTSIM_LEDGER_LACK_VOTES 7u    /* votes None or fewer than 13 fields; or, after BAD_VOTE, distinct voters <=
                                          bftsim_two_thirds_majority(N) (LackVotes) */
#define BFTSIM_LEDGER_BAD_VOTE 8u      /* a vote does not recover, or recovers outside the set (InvalidSignature) */
#define BFTSIM_LEDGER_BAD_PROPOSER 9u  /* header.proposer is not in the set */
struct bftsim_ledger_report {
    uint64_t headers;               /* slots with hdr_len != 0 */
    uint64_t by_status[10];         /* slots per status, ABSENT included */
    uint64_t votes;                 /* votes of the decodable headers */
    uint64_t recoveries;            /* ECDSA recoveries performed (one per vote) */
    uint64_t duplicate_votes;       /* votes of a validator whose vote the header already held (not counted as voters) */
    uint64_t verified_instances;    /* instances where every non-absent slot is OK and the absent ones form a suffix */
};
typedef struct bftsim_ledger_report bftsim_ledger_report;
struct bftsim_ledger_out {          /* host, caller-owned, any pointer may be NULL; rows inst * max_heights + x - 1 */
    uint8_t *status;                /* [inst_count * max_heights] BFTSIM_LEDGER_* */
    uint8_t *block_hash;            /* x32: Keccak-256 of the header re-encoded from its decoded fields with votes nil
                                       (deserialize, then block_hash()); zeros where absent or undecodable */
    uint64_t *voters;               /* x4: bitmap of the validators whose seal recovered */
    uint16_t *n_votes;              /* votes the header carries (0 where None, absent or undecodable) */
    uint64_t *verified_height;      /* [inst_count] the largest x with slots 1..x all OK */
};
typedef struct bftsim_ledger_out bftsim_ledger_out;
/* hdr / hdr_len: host buffers in the layout bftsim_export_ledger writes (slot i * max_heights + x - 1 of slot_bytes
 * bytes, hdr_len 0 for an absent height). The parent of x = 1 is the genesis (bftsim_genesis_hash, genesis_time); the
 * parent of x > 1 is slot x - 1 as decoded, whether or not it verified itself. A vote is recovered over
 * keccak(0x03 || block hash). The reference counts votes.len(); distinct validators are counted here (a validator's
 * seal is the same bytes every time, RFC 6979), the surplus reported in duplicate_votes. The validator set, N,
 * block_period, genesis_time and the genesis hash are the handle's; no secrets are needed and bftsim_set_crypto need
 * not have been called (libbftsig.so must be next to libbftsim.so). The handle's run state is untouched; the work runs
 * on the stream of the last launch (the default stream when there is none). Arguments are checked before any device
 * work and a refused call writes nothing: BFTSIM_EINVAL for a null h, hdr, hdr_len or report, max_heights of 0 or above
 * 65,535, slot_bytes of 0, 2^31 instances or more; BFTSIM_ENOMEM for 2^31 slots or more. Hostile contents are never an
 * error of the call: they become statuses. */
int bftsim_verify_ledger(bftsim_t *h, const uint8_t *hdr, uint64_t slot_bytes, const uint32_t *hdr_len,
                         uint64_t inst_count, uint32_t max_heights, const bftsim_ledger_out *out,
                         bftsim_ledger_report *report);
/* diagnostics: device times (ms, HIP events) of the last bftsim_verify_ledger's decode (the decode kernel and the vote
 * scan, then the scatter; not the host's wait for the scan's total between them), recoveries, tally + link, and copies, as scripts/ledger_bench.py records them */
int bftsim_ledger_last_ms(bftsim_t *h, float *decode_ms, float *recover_ms, float *tally_ms, float *copy_ms);

/* ValidatorSet / block helpers on the host (validator.rs, types/block.rs) */
uint32_t bftsim_two_thirds_majority(uint32_t n);                    /* validator.rs:149-154 */
uint32_t bftsim_seed_from_hash(const uint8_t hash[32], uint32_t n); /* validator.rs:39-48 (BE) */
uint32_t bftsim_seed_from_hash_order(const uint8_t hash[32], uint32_t n, uint32_t seed_byte_order);
uint32_t bftsim_calc_proposer(const uint8_t prev_hash[32], uint32_t n, uint64_t round); /* :33-37,74-77 (BE) */
void bftsim_keccak256(const uint8_t *data, size_t len, uint8_t out[32]);
void bftsim_genesis_hash(const bftsim_config *cfg, uint8_t out[32]); /* core/genesis.rs:44-55 */
int bftsim_view_cmp(uint64_t h1, uint64_t r1, uint64_t h2, uint64_t r2); /* consensus/types.rs:81-98 */
/* Core::check_message (src/consensus/pbft/core/core.rs:366-399) as the kernels run it: code =
 * MessageType (protocol/mod.rs:36-41: 1 Preprepare, 2 Prepare, 3 Commit, 4 RoundChange), state =
 * State (protocol/mod.rs:25-30: 1 AcceptRequest .. 4 Committed). Returns BFTSIM_CHECK_* (>= 0), or
 * BFTSIM_EINVAL for codes / states outside those enums. */
#define BFTSIM_CHECK_OK 0
#define BFTSIM_CHECK_UNKNOWN 1        /* ConsensusError::UnknownMessageType (height 0) */
#define BFTSIM_CHECK_FUTURE_BLOCK 2   /* FutureBlockMessage(h) */
#define BFTSIM_CHECK_OLD 3            /* OldMessage */
#define BFTSIM_CHECK_FUTURE_MSG 4     /* FutureMessage (backlog) */
int bftsim_check_message(uint32_t code, uint64_t msg_height, uint64_t core_height, uint32_t state);

/* Ledger export (core/ledger.rs:193-245 `add_block`: the `headers` map Hash -> Header of
 * store/schema.rs:66-68; the `block_hashes_by_height` list is bftsim_result.block_hash): after a
 * launch or run, the MessagePack Header bytes (SPEC.md §7, votes None: commit seals are not
 * modelled) of every committed height of the last launch, host buffers:
 * hdr[(i*H + x-1) * BFTSIM_HEADER_SLOT ...] with hdr_len[i*H + x-1] bytes (0 beyond the committed
 * height); Keccak-256 of those bytes is that height's block hash. capacity = instances the buffers
 * hold (hdr: capacity*H slots, hdr_len: capacity*H words). */
#define BFTSIM_HEADER_SLOT 288
int bftsim_export_headers(bftsim_t *h, uint64_t capacity, uint8_t *hdr, uint32_t *hdr_len);

#ifdef __cplusplus
}
#endif
#endif
