"""The genesis times and block periods at which a header's `time` field (SPEC.md §7:
genesis_time + block_period * (time_tick + 1)) takes each of MessagePack's five unsigned widths, and changes width
in the middle of a chain. Plain data and two helpers, shared by the CPU and the GPU tests of the time widths
(test_oracle_kat, test_emu_time_widths, test_time_widths_cpu, test_gpu_time_widths)."""
from __future__ import annotations

import dataclasses
import functools

import numpy as np

# id -> (genesis_time, or None: the largest that cannot wrap for the config; block_period;
#        the encoded sizes of `time` the case is there for; whether a chain changes size between two heights)
CASES = {
    "t-1-2": (120, 1, {1, 2}, True),                      # 0x7f -> 0xcc 0x80 within 8 ticks
    "t-2-3": (250, 1, {2, 3}, True),                      # 0xcc 0xff -> 0xcd 0x01 0x00 within 6 ticks
    "t-0": (0, 1, {1, 2, 3}, True),                       # with the height field: needs >= 260 heights
    "t-3-5": (65500, 3, {3, 5}, True),                    # 0xcd -> 0xce near tick 11
    "t-5-9": (2 ** 32 - 40, 3, {5, 9}, True),             # 0xce -> 0xcf near tick 13
    "t-bigstep": (0, 2 ** 32 - 1, {5, 9}, True),          # 2^32 - 1 at tick 0, 9 bytes afterwards
    "t-top": (None, 3, {9}, False),                       # high bytes all 0xff, the last tick still below 2^64
}
IDS = list(CASES)
SHORT_IDS = [k for k in IDS if k != "t-0"]               # the rows that show their sizes within 20 heights


def le(cfg):
    return dataclasses.replace(cfg, seed_byte_order=1, name=(cfg.name or "n%d" % cfg.n) + "-le")


# the MessagePack width boundaries of an unsigned integer, for the encoder grids of the CPU tier (test_oracle_kat,
# test_time_widths_cpu): every height x every time x parents and tx hashes of all-high and all-low bytes
WIDTH_EDGES = [0, 127, 128, 255, 256, 65535, 65536, 2 ** 32 - 1]
GRID_HEIGHTS = WIDTH_EDGES
GRID_TIMES = WIDTH_EDGES + [2 ** 32, 2 ** 64 - 1]
GRID_HASHES = [bytes(range(200, 232)), bytes(range(0, 32))]        # all-high (two bytes each) and all-low

# ---- pipelined chain kernels (N = 64): 5 launches over distinct ranges, the last one compared. Only the depth-3 modes
# (wave, pair: lossless cfg3) come back to a set; at depth 6 five launches reuse none, so the lossy modes here show
# the widths, not a repair over another instance's rows (tests/test_gpu_set_reuse.py has those).
# name -> (config of _shapes' chain_cfg, instances, depth, hash batch or 0, environment under BFTSIM_TESTING=1).
# The library does not report which chain kernel a launch ran: these settings select the modes only as long as
# bftsim.hip's knobs and thresholds (chain_wave_max, chain_lane_min, chain_inline, chain_grid, hash_spec, seed_spec)
# keep their meaning, as for the pipeline tests these settings are taken from.
LAUNCHES = 5


def _lane(inline, spec, grid):
    return dict(BFTSIM_CHAIN_LANE_MIN="1", BFTSIM_CHAIN_INLINE=inline, BFTSIM_HASH_SPEC=spec, BFTSIM_CHAIN_GRID=grid)


CHAIN_MODES = {
    "wave": ("cfg3-30", 64, 3, 4, dict(BFTSIM_CHAIN_WAVE_MAX="1000000")),
    "pair": ("cfg3-30", 64, 3, 4, dict(BFTSIM_CHAIN_WAVE_MAX="0")),
    "pair-predicted": ("cfg3-30", 96, 6, 2, dict(BFTSIM_HASH_SPEC="2")),
    "pair-recorded": ("cfg3-30", 96, 6, 2, dict(BFTSIM_HASH_SPEC="0")),
    "pair-predicted-drop": ("n64-drop", 96, 6, 2, dict(BFTSIM_HASH_SPEC="2")),      # the repair from inside a chain
    "pair-recorded-drop": ("n64-drop", 96, 6, 2, dict(BFTSIM_HASH_SPEC="0")),
    "le-predicted": ("cfg3-30-le", 96, 6, 0, dict(BFTSIM_SEED_SPEC="1")),
    "le-wave-hash": ("cfg3-30-le", 96, 6, 0, dict(BFTSIM_SEED_SPEC="0")),
}
CHAIN_MODES.update({f"lane-inline{i}-spec{s}-grid{g}": ("cfg3-30", 160, 6, 3, _lane(i, s, g))
                    for i in "01" for s in "20" for g in "03"})
CHAIN_MODES["lane-inline1-spec2-drop"] = ("n64-drop", 160, 6, 3, _lane("1", "2", "0"))
CHAIN_MODE_IDS = list(CHAIN_MODES)
TIGHTEST = "lane-inline1-spec2-grid0"                   # the 56-dword LDS column, each lane's own encoder call
CHAIN_MODES[TIGHTEST + "-260"] = ("cfg3-260",) + CHAIN_MODES[TIGHTEST][1:]         # t-0 shows its sizes from 256 heights on


def _shapes():
    """name -> (config, first instance, instances), per group of tests/test_gpu_time_widths.py"""
    from bftsim.configs import BftConfig, cfg2, cfg3, cfg5
    drop64 = dict(n=64, byz_count=21, drop_ppm=50_000)
    # plain Simulator.run: the smallest shape that selects each kernel and still commits past tick 13 (where t-5-9
    # changes size)
    plain = {
        "n4-drop10": (lambda: cfg2(heights=40), 0, 64),
        "n7-drop5": (lambda: cfg5(heights=60), 0, 64),                      # several instances per wave, segment hash
        "n64-byz21": (lambda: cfg3(heights=70), 0, 3),                      # FAST + canonical_run, two passes
        "n64-byz21-le": (lambda: le(cfg3(heights=70)), 0, 3),               # in-kernel wave hash, seed chain kernel
        "n64-drop5": (lambda: BftConfig(heights=20, seed=15, name="n64-drop5", **drop64), 0, 4),     # resume kernel
        # where the next proposer depends on the block hash (little-endian seeds, N no power of two) the time case
        # changes the schedule, and most lossy chains with f Byzantine validators fork within 10 heights: 64 or 128
        # instances, so that some commit past tick 13 at every case
        "n64-drop5-le": (lambda: le(BftConfig(heights=20, seed=9, name="n64-drop5", **drop64)), 0, 64),
        "n65-drop10": (lambda: BftConfig(n=65, heights=20, seed=9, byz_count=21, drop_ppm=100_000, name="n65"), 0, 128),
        "n100-drop10": (lambda: BftConfig(n=100, heights=20, seed=6, byz_count=33, drop_ppm=100_000, name="n100"), 0, 128),
        "n256-byz85": (lambda: BftConfig(n=256, heights=16, seed=5, byz_count=85, name="n256"), 0, 2),
    }
    long = {
        "n64-byz21-260": (lambda: cfg3(heights=260), 0, 3),
        "n7-drop5-300": (lambda: cfg5(heights=300), 0, 16),
    }
    chain_cfg = {
        "cfg3-30": lambda: cfg3(heights=30),
        "n64-drop": lambda: BftConfig(heights=30, seed=17, name="n64-drop", **drop64),
        "cfg3-30-le": lambda: le(cfg3(heights=30)),
        "cfg3-260": lambda: cfg3(heights=260),
    }
    chain = {mode: (chain_cfg[c], (LAUNCHES - 1) * n, n) for mode, (c, n, *_) in CHAIN_MODES.items()}
    # ledger export: 16 heights, so that a lossless chain passes tick 13
    ledger = {
        "n64-byz21": (lambda: cfg3(heights=16), 0, 6),
        "n7-drop5": (lambda: cfg5(heights=16), 0, 16),
    }
    no_fast = {"n64-byz21": (lambda: cfg3(heights=20), 0, 3)}              # with Simulator.set_fast(False)
    stream = (lambda: cfg5(heights=300), 0, 16, 64)                         # windowed: first, instances, window
    return dict(PLAIN=plain, LONG=long, CHAIN=chain, LEDGER=ledger, NO_FAST=no_fast), stream


TABLES, STREAM = _shapes()
PLAIN, LONG, CHAIN, LEDGER, NO_FAST = (TABLES[k] for k in ("PLAIN", "LONG", "CHAIN", "LEDGER", "NO_FAST"))
STREAM_IDS = ["t-0", "t-5-9"]
LEDGER_IDS = ["t-2-3", "t-5-9", "t-top"]
CHAIN_IDS = ["t-1-2", "t-5-9", "t-top"]                 # sizes 1/2 and 5/9 with a change inside a chain; the longest suffix
CHAIN_REST = [k for k in IDS if k not in CHAIN_IDS]    # on the tightest chain mode only (inline, predicted lanes)


@functools.lru_cache(maxsize=None)
def reference(table: str, shape: str, case: str):
    """-> (config, first, n, the oracle's run) of a shape of TABLES at a time case: computed once per session, left
    unchanged, and asserted to show the case's sizes"""
    import oracle_lib as O
    mk, first, n = TABLES[table][shape]
    cfg = with_time(mk(), case)
    ref = O.run(cfg, first, n, threads=8)
    assert_case(case, cfg, ref)
    return cfg, first, n, ref


# ---- real-crypto mode (SPEC.md §11): the header's `time` inside PrePrepare frames, archives and sealed ledgers, and
# create_time = 1000 * (genesis_time + block_period * tick) of the RoundChange frames. 1000 * time stays below 2^64.
# id -> (genesis_time, block_period, sizes of the header's time, sizes of create_time over all frames)
CRYPTO = {
    "c-1-2": (120, 1, {1, 2}, {1, 5}),                    # create_time 121,000 ...: the 5-byte form
    "c-5-9": (2 ** 32 - 40, 3, {5, 9}, {1, 9}),
    "c-2^54": (2 ** 54, 3, {9}, {1, 9}),                  # 1000 * 2^54 = 0xfa00...: the top byte of create_time in use
    "c-2-3": (250, 1, {2, 3}, {1, 5}),                    # a header time of exactly 256 (0xcd 0x01 0x00) in a PrePrepare frame
    "c-0": (0, 1, {1}, {1, 3}),                           # create_time 1000 * tick: 3 bytes to tick 65, 5 from tick 66
}
CRYPTO_IDS = list(CRYPTO)
CRYPTO_SHAPES = ("cfg1", "n4-lossy")                    # at every case; and once, at c-5-9:
CRYPTO_ONCE = ("c-5-9", "n65-lossy")


def _crypto_shape(case: str, shape: str):
    """-> (config, secrets, first, instances). cfg1 (N = 5, the keys of examples/*.toml, c5 silent) at 12 heights, 14
    where the time has to pass tick 13, 6 where every size shows at once; N = 4 with drops, one instance, <= 12 heights
    (c-0: 30 % drops, so that round changes go on past tick 66); N = 65 with drops, one instance, 6 heights"""
    import ledger_ref as LR
    import trace_ref as TR
    from bftsim.configs import BftConfig, cfg1
    g, period = CRYPTO[case][:2]
    if shape == "cfg1":
        keys = TR._reference_keys()
        # N = 5: the proposers follow the block hashes, so the genesis time decides where the silent c5 proposes and a
        # round changes; at genesis time 0, seed 4 has round changes within 6 heights (seed 1 has none within 12)
        cfg = cfg1(True, heights={"c-1-2": 12, "c-5-9": 14}.get(case, 6), seed=4 if case == "c-0" else 1)
        cfg = dataclasses.replace(cfg, genesis_time=g, block_period=period, name=f"cfg1-{case}")
        return cfg, [keys[a] for a in cfg.addresses], 0, 1
    if shape == "n65-lossy":
        # several lane rounds per wave, 44 seals. N = 65 shrugs off 10 % drops without a round change; at 17 % instance
        # 9 commits its 6 heights at ticks 0, 1, 3, 6, 13, 14 in 18 views: RoundChange frames, and 9-byte times at the
        # last two heights
        n, heights, drop, first = 65, 6, 170_000, 9
    else:
        n = 4
        heights, drop, first = {"c-1-2": (12, 100_000, 4), "c-5-9": (12, 100_000, 4), "c-0": (8, 300_000, 3)}.get(
            case, (6, 100_000, 4))
    cfg, sec = LR.keyed(BftConfig(n=n, heights=heights, seed=21, drop_ppm=drop, genesis_time=g, block_period=period,
                                  name=f"{shape}-{case}"), 7)
    return cfg, sec, first, 1


@functools.lru_cache(maxsize=None)
def crypto_reference(case: str, shape: str):
    """the Python reference of a real-crypto run at a time case, computed once per session and shared by the CPU and
    the GPU tests: trace_ref.reference's dict (cfg, secrets, first, n, forged, res, inst) plus `want`: the Python
    observer's, archiver's and importer's verdicts on the trace (twins_ref.verdicts), and the sizes it shows"""
    import oracle_lib as O
    import trace_ref as TR
    import twins_ref as TW
    cfg, secrets, first, n = _crypto_shape(case, shape)
    res = O.run_crypto(cfg, first, n, cap=4096)
    assert int(res["mlog_n"].max()) < 4096
    inst = [TR.instance_trace(cfg, first, res, i, secrets, (), rel=i) for i in range(n)]
    ref = dict(cfg=cfg, secrets=secrets, first=first, n=n, forged=(), res=res, inst=inst)
    stream, off, _, f0 = TR.joined(ref)
    ref["want"] = TW.verdicts(cfg, res, stream, off, f0)
    ref["time_sizes"] = time_sizes(cfg, res)[0]
    ref["ctime_sizes"] = {uint_size(m["ctime"]) for t in inst for m in t[3]}
    return ref


@functools.lru_cache(maxsize=None)
def twins_reference():
    """twins_ref.reference('n7') (N = 7, byz_count 2, seed 5, lossless, instances 2..3) at c-5-9 over 15 heights, so that
    an equivocator's second frames carry headers with 5- and 9-byte times"""
    import ledger_ref as LR
    import oracle_lib as O
    import twins_ref as TW
    from bftsim.configs import BftConfig
    g, period = CRYPTO["c-5-9"][:2]
    cfg, secrets = LR.keyed(BftConfig(n=7, heights=15, seed=5, byz_count=2, genesis_time=g, block_period=period,
                                      name="n7-byz2-c-5-9"), 7)
    first, n = 2, 2
    res = O.run_crypto(cfg, first, n, cap=4096)
    inst = [TW.instance_trace(cfg, first, res, i, secrets, (), rel=i) for i in range(n)]
    ref = dict(cfg=cfg, secrets=secrets, first=first, n=n, forged=(), res=res, inst=inst,
               plain=[TW.plain_of(t) for t in inst], counts=tuple(sum(t[4][k] for t in inst) for k in (0, 1)))
    stream, off, _, f0 = TW.joined(ref)
    ref["want"] = TW.verdicts(cfg, res, stream, off, f0)
    ref["time_sizes"] = time_sizes(cfg, res)[0]
    return ref


def assert_crypto_case(case: str, shape: str, ref):
    _, _, hdr, ctime = CRYPTO[case]
    if (case, shape) == ("c-0", "n4-lossy"):
        ctime = ctime | {5}
    assert hdr <= ref["time_sizes"], (case, shape, "header time sizes", sorted(ref["time_sizes"]))
    assert ctime <= ref["ctime_sizes"], (case, shape, "create_time sizes", sorted(ref["ctime_sizes"]))
    assert max(m["ctime"] for t in ref["inst"] for m in t[3]) < 2 ** 64


def boundary_ledgers():
    """the importer's rule time >= parent.time + block_period across the 32-bit boundary, in the tuples of
    ledger_ref.tamper_cases: cfg1's sealed ledger with height 2 at time 2^32 - 1 and height 3 (chained to it) at exactly
    parent + block_period (a 9-byte time above a 5-byte one: OK) and at one less (BAD_TIME)"""
    import ledger_ref as LR
    c1 = LR.reference("cfg1")
    L, sec, period = c1["ledger"][0], c1["secrets"], c1["cfg"].block_period
    rs = lambda h, **f: LR.reseal(LR.replace_field(h, **f), sec, [0, 1, 2, 3])
    parent = rs(L[1], time=2 ** 32 - 1)
    link = LR.block_hash(LR.decode(parent))
    out = []
    for name, t, st in (("exact", 2 ** 32 - 1 + period, LR.OK), ("one less", 2 ** 32 - 2 + period, LR.BAD_TIME)):
        assert uint_size(t) == 9 and uint_size(2 ** 32 - 1) == 5
        out.append((f"time {name} at 2^32", c1, [[L[0], parent, rs(L[2], prev_hash=link, time=t)]], 6,
                    {(0, 1): LR.OK, (0, 2): LR.OK, (0, 3): st}))
    return out


def with_time(cfg, case: str):
    """cfg at the case's genesis_time and block_period (t-top: from cfg's own max_ticks)"""
    g, period, _, _ = CASES[case]
    if g is None:
        g = 2 ** 64 - 1 - period * (cfg.max_ticks + 2)
    return dataclasses.replace(cfg, genesis_time=g, block_period=period, name=f"{cfg.name or 'n%d' % cfg.n}-{case}")


def uint_size(v: int) -> int:
    """bytes MessagePack spends on an unsigned integer"""
    assert 0 <= v < 2 ** 64, v
    return 1 if v < 128 else 2 if v < 256 else 3 if v < 65536 else 5 if v < 2 ** 32 else 9


def time_sizes(cfg, res):
    """-> (the set of encoded sizes of `time` over the committed rows of an oracle result, whether the size changes
    between two consecutive heights of one instance). Python integers: a time at or above 2^64 asserts."""
    sizes, change = set(), False
    for i, ch in enumerate(np.asarray(res["committed_height"])):
        row = [uint_size(cfg.genesis_time + cfg.block_period * (int(t) + 1)) for t in res["time_tick"][i, :int(ch)]]
        sizes.update(row)
        change = change or any(a != b for a, b in zip(row, row[1:]))
    return sizes, change


def assert_case(case: str, cfg, res, what=""):
    """the run really has the sizes the case is there for (and a change inside a chain where the table says so)"""
    _, _, want, mid = CASES[case]
    sizes, change = time_sizes(cfg, res)
    assert want <= sizes, (what or cfg.name, case, "sizes", sorted(sizes), "wanted", sorted(want))
    assert change or not mid, (what or cfg.name, case, "no size change inside a chain")
    if case == "t-top":
        last = cfg.genesis_time + cfg.block_period * (int(np.asarray(res["time_tick"]).max()) + 1)
        assert last < 2 ** 64 and cfg.genesis_time >> 16 == 2 ** 48 - 1, (what or cfg.name, hex(cfg.genesis_time))
