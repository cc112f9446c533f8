"""GPU: row-table sets reused by other instances, every launch compared (tests/reuse_cases.py).

The pipelined launch mode keeps a ring of row-table sets. FAST launches (N = 64) do not clear the record rows, predicted
chains hash from launch time on, and only bft_spec_verify_kernel and the CHAIN_REPAIR re-run put right what a
prediction got wrong. That rests on every reader stopping at the committed height and on the repair starting at exactly
the first recorded block that differs from its prediction. Launches that repeat one instance range cannot show either
fail: the set they reuse already holds the right rows. Here every launch has a range of its own, so a reused set holds
the rows, hashes, predictions and suffix rows of other instances -- lower and higher committed heights, other blocks
(reuse_cases.assert_reuse_preconditions, asserted first by every test) -- and each launch that is compared is compared
whole: a skipped or late repair, a wrong first-differing height or a row read past the committed height surfaces as a
wrong hash or a stale row. The proposer-crash configurations are the repair cases (every instance misses a prediction,
from height 1 or from inside its chain); drop, fork and byz22 stay on the canonical tick and can miss only on the
variant.

Every chain kernel and mode (the settings of test_gpu_pipeline.py, which the library reads only under BFTSIM_TESTING=1
and does not report back: they select the modes as long as bftsim.hip's knobs keep their meaning), two ring shapes,
two drivers; alternating launch sizes; an unpipelined handle; both drivers in turn on one handle; the tip hashes and
the exported headers; the general kernel, which clears its rows, as control."""
import pytest

import reuse_cases as R
from parity_util import assert_same

pytestmark = pytest.mark.gpu


def _lane(inline, spec, grid=None):
    env = dict(BFTSIM_CHAIN_LANE_MIN="1", BFTSIM_CHAIN_INLINE=inline, BFTSIM_HASH_SPEC=spec)
    if grid:
        env["BFTSIM_CHAIN_GRID"] = grid
    return env


# mode -> environment; None: no knobs at all, not even BFTSIM_TESTING (the product's own choices)
MODES = {
    "default": None,
    "pair-pred": dict(BFTSIM_HASH_SPEC="2"),              # 2: predicted chains for lossy schedules too
    "pair-rec": dict(BFTSIM_HASH_SPEC="0"),
    "wave": dict(BFTSIM_CHAIN_WAVE_MAX="1000000", BFTSIM_HASH_SPEC="0"),
    "lane-inline0-pred": _lane("0", "2"),
    "lane-inline0-rec": _lane("0", "0"),
    "lane-inline1-pred": _lane("1", "2"),
    "lane-inline1-rec": _lane("1", "0"),
    "lane-inline1-pred-grid3": _lane("1", "2", "3"),      # 3 persistent waves for the whole batch
}
LE_MODES = {
    "le-spec": dict(BFTSIM_SEED_SPEC="1"),                # the seed chain's predictions, per set
    "le-wave": dict(BFTSIM_SEED_SPEC="0"),                # hashes in-kernel
}
MODES_ALL = {**MODES, **LE_MODES}
# (depth, hash batch): at 2 x 3 the ring comes back to a set still waiting in the batch, which is flushed first
RINGS = [(3, 2), (2, 3)]
RING_IDS = ["d3b2", "d2b3"]
STEP_LAUNCHES = 7
BURSTS = (1, 2, 3, 4)                                     # launches per burst: ranges 0 | 1 2 | 3 4 5 | 6 7 8 9

MATRIX = [(c, m) for c in R.BIG_ENDIAN for m in MODES] + [("le-drop", m) for m in LE_MODES]
MATRIX_IDS = [f"{c}-{m}" for c, m in MATRIX]


def _sim(cfg):
    from bftsim.runtime import Simulator
    return Simulator(cfg)


def _set_mode(mode, monkeypatch):
    env = MODES_ALL[mode]
    if env is None:
        monkeypatch.delenv("BFTSIM_TESTING", raising=False)
        return
    monkeypatch.setenv("BFTSIM_TESTING", "1")
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _compare(sim, ref, what):
    """sync, fetch and stats of the last launch against the oracle's result of its range"""
    sim.sync()
    got = sim.fetch()
    st = sim.stats()
    assert_same(ref, got, what)
    assert st["views"] == int(ref["views"].sum()), (what, "views")
    assert st["committed_heights"] == int(ref["committed_height"].sum()), (what, "committed_heights")


def _stepwise(cfg_id, depth, batch, what, launches=STEP_LAUNCHES, sizes=None):
    """`launches` launches over the ranges 0, 1, ...; every one compared, so every reuse of every set is pinned.
    sizes: the launch sizes in turn (prepare between the launches), the heads of the ranges compared"""
    n = R.instances(cfg_id)
    sim = _sim(R.config(cfg_id))
    try:
        sim.set_pipeline(True, depth)
        if batch:
            sim.set_hash_batch(batch)
        sim.prepare(n)
        for k in range(launches):
            m = sizes[k % len(sizes)] if sizes else n
            if sizes:
                sim.prepare(m)
            sim.launch(k * n)
            _compare(sim, R.head(R.ref(cfg_id, k), m), f"{what} launch {k} of {m}")
    finally:
        sim.close()


def _bursts(cfg_id, depth, batch, what):
    """the ranges 0 .. 9 in bursts of 1, 2, 3 and 4 launches, the last launch of each burst compared: several launches
    in flight in a batch (sync flushes every batch at size 1 in the stepwise driver), the ring wrapping across bursts"""
    n = R.instances(cfg_id)
    sim = _sim(R.config(cfg_id))
    try:
        sim.set_pipeline(True, depth)
        sim.set_hash_batch(batch)
        sim.prepare(n)
        k = 0
        for burst in BURSTS:
            for _ in range(burst):
                sim.launch(k * n)
                k += 1
            _compare(sim, R.ref(cfg_id, k - 1), f"{what} burst of {burst}, launch {k - 1}")
    finally:
        sim.close()
    assert k == R.MAX_LAUNCHES


@pytest.mark.parametrize("depth,batch", RINGS, ids=RING_IDS)
@pytest.mark.parametrize("cfg_id,mode", MATRIX, ids=MATRIX_IDS)
def test_stepwise(cfg_id, mode, depth, batch, monkeypatch):
    R.assert_reuse_preconditions(cfg_id, depth, STEP_LAUNCHES)
    _set_mode(mode, monkeypatch)
    _stepwise(cfg_id, depth, batch, f"{cfg_id} {mode} depth {depth} batch {batch}")


@pytest.mark.parametrize("depth,batch", RINGS, ids=RING_IDS)
@pytest.mark.parametrize("cfg_id,mode", MATRIX, ids=MATRIX_IDS)
def test_bursts(cfg_id, mode, depth, batch, monkeypatch):
    R.assert_reuse_preconditions(cfg_id, depth, sum(BURSTS))
    _set_mode(mode, monkeypatch)
    _bursts(cfg_id, depth, batch, f"{cfg_id} {mode} depth {depth} batch {batch}")


@pytest.mark.parametrize("depth,batch", RINGS, ids=RING_IDS)
@pytest.mark.parametrize("mode", ["pair-pred", "lane-inline1-pred"])
@pytest.mark.parametrize("cfg_id", ["crash", "drop"])
def test_alternating_sizes(cfg_id, mode, depth, batch, monkeypatch):
    """prepare(96) / prepare(40) between the launches: a launch of 40 leaves rows 40 .. 95 of the set's previous user
    untouched, and the next launch of 96 finds them there"""
    R.assert_reuse_preconditions(cfg_id, depth, STEP_LAUNCHES)
    _set_mode(mode, monkeypatch)
    _stepwise(cfg_id, depth, batch, f"{cfg_id} {mode} depth {depth} batch {batch} sizes 96/40", sizes=(R.N_INST, 40))


@pytest.mark.parametrize("mode", ["default", "pair-pred"])
@pytest.mark.parametrize("cfg_id", ["drop", "crash-byz"])
def test_tips_and_exported_headers(cfg_id, mode, monkeypatch):
    """the two other readers of a set after a launch: the tip hashes (the hash at the committed height, the genesis
    hash at height 0) and the ledger export (a header per committed height, nothing above it), after every launch of
    the stepwise sequence -- instances that stop below the previous user's height have its rows and hashes above"""
    import numpy as np
    import oracle_lib as O
    import trace_ref as TR
    R.assert_reuse_preconditions(cfg_id, 3, STEP_LAUNCHES)
    _set_mode(mode, monkeypatch)
    cfg, n = R.config(cfg_id), R.instances(cfg_id)
    genesis = np.frombuffer(TR.genesis_hash(cfg), np.uint8)
    sim = _sim(cfg)
    try:
        sim.set_pipeline(True, 3)
        sim.set_hash_batch(2)
        sim.prepare(n)
        for k in range(STEP_LAUNCHES):
            sim.launch(k * n)
            sim.sync()
            summ = sim.fetch_summary(n)
            hdrs = sim.export_headers(n)
            ref = R.ref(cfg_id, k)
            ch = ref["committed_height"]
            assert np.array_equal(summ["committed_height"], ch), (cfg_id, mode, k)
            want = np.where((ch > 0)[:, None], ref["block_hash"][np.arange(n), np.maximum(ch, 1) - 1], genesis[None, :])
            assert np.array_equal(summ["tip_hash"], want), (cfg_id, mode, k, "tips")
            for i in range(n):
                for x in range(1, cfg.heights + 1):
                    h = hdrs[i][x - 1]
                    if x > ch[i]:
                        assert h == b"", (cfg_id, mode, k, i, x, "a header above the committed height")
                    else:
                        assert O.keccak256(h) == bytes(ref["block_hash"][i, x - 1]), (cfg_id, mode, k, i, x)
    finally:
        sim.close()


@pytest.mark.parametrize("cfg_id", ["drop", "crash", "byz22"])
def test_unpipelined_handle_reuse(cfg_id):
    """one handle, run() over four ranges without a pipeline: set 0 of a FAST launch is not cleared either"""
    n = R.instances(cfg_id)
    sim = _sim(R.config(cfg_id))
    try:
        for k in range(4):
            got = sim.run(k * n, n)
            st = sim.stats()
            ref = R.ref(cfg_id, k)
            assert_same(ref, got, f"{cfg_id} unpipelined run {k}")
            assert st["views"] == int(ref["views"].sum()) and st["committed_heights"] == int(ref["committed_height"].sum())
    finally:
        sim.close()


@pytest.mark.parametrize("mode", ["default", "pair-pred"])
@pytest.mark.parametrize("cfg_id", ["drop", "crash"])
def test_mixed_drivers_on_one_handle(cfg_id, mode, monkeypatch):
    """pipelined launches, an unpipelined run() between them, pipelined launches again, on one handle of depth 3 and
    hash batch 2. The run() carries a tick trace, which keeps it off the launch streams: it waits for the pipelined
    launches before it, runs wholly on set 0 and leaves the ring's cursor alone. So the sets go 1, 2 | 0 | 0, 1, 2:
    range 3 reuses the set of range 2 (the run's), ranges 4 and 5 those of ranges 0 and 1 -- every reused set holds
    another range's rows, asserted first on the oracle alone. Every launch is compared whole, the run() both by what
    it returns and by a fetch of its own."""
    launches, trace_ticks = 6, 4
    R.assert_reuse_preconditions(cfg_id, 3, launches)
    for prev, new in ((2, 3), (0, 4), (1, 5)):
        lower, differing = R.stale_counts(R.ref(cfg_id, prev), R.ref(cfg_id, new))
        if cfg_id == "crash":
            assert differing == R.N_INST, (cfg_id, prev, new, differing)
        else:
            assert lower >= R.MIN_LOWER and differing >= R.MIN_DIFFERING, (cfg_id, prev, new, lower, differing)
    _set_mode(mode, monkeypatch)
    n = R.instances(cfg_id)
    cfg = R.config(cfg_id)
    sim = _sim(cfg)
    try:
        sim.set_pipeline(True, 3)
        sim.set_hash_batch(2)
        sim.prepare(n)
        for k in range(launches):
            what = f"{cfg_id} {mode} mixed drivers, range {k}"
            if k == 2:
                got = sim.run(k * n, n, trace_ticks=trace_ticks)
                assert got["trace"].shape == (n, trace_ticks, cfg.n)
                assert_same(R.ref(cfg_id, k), got, what + " (run)")
            else:
                sim.launch(k * n)
            _compare(sim, R.ref(cfg_id, k), what)
    finally:
        sim.close()


@pytest.mark.parametrize("cfg_id", list(R.CONTROLS))
def test_general_kernel_control(cfg_id):
    """the general kernel clears its rows, hashes each launch on a hash stream and marks each set done by itself:
    depth 2, 5 launches over distinct ranges, every one compared"""
    _stepwise(cfg_id, 2, 0, f"{cfg_id} general kernel depth 2", launches=5)
