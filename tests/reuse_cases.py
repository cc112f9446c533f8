"""Row-table sets reused by other instances (N = 64 FAST launches leave the record rows uncleared, predicted chains
hash from launch time on, and only bft_spec_verify_kernel and the CHAIN_REPAIR re-run put right what a prediction got
wrong): the configurations, the oracle's run of every instance range, computed once and shared, and the conditions
under which a reused set really holds stale rows that differ from the fresh ones. Plain data and helpers, shared by
test_reuse_cases_cpu (the conditions, on the oracle alone) and test_gpu_set_reuse (the launches)."""
from __future__ import annotations

import functools

import numpy as np

N_INST = 96            # per launch, range k at k * 96: 1.5 waves of the lane kernel, an odd tail of lane pairs
MAX_LAUNCHES = 10      # ranges k = 0 .. 9

# id -> BftConfig fields (N = 64). drop, fork and byz22 commit every block with proposer 0 at tick = height - 1 (checked
# over k < 10), so a prediction can miss there only on the variant (a library without the repair still passes drop in
# the predicted modes and fails fork and byz22, DESIGN §4h: drop's predictions do not miss at all over these ranges);
# crash misses in every instance, from height 1 (the whole chain repaired) or from inside the chain, and every
# instance commits all 30 heights.
# crash-byz (seed 35): 8 .. 17 of a range's 96 instances time out before they commit anything and a few more within 3
# heights, at this seed and at every seed from 35 to 119, so "every instance has a row that differs from the previous
# user's" cannot hold for it at any seed. It keeps crash's per-range miss conditions and takes, for the stale rows,
# the lossy configurations' two conditions with the differing-row bound at two thirds of the instances (below).
CONFIGS = {
    "drop": dict(heights=30, seed=17, byz_count=21, drop_ppm=50_000),
    "crash": dict(heights=30, seed=18, proposer_crash_ppm=300_000),
    "crash-byz": dict(heights=40, seed=35, byz_count=10, proposer_crash_ppm=200_000),
    "fork": dict(heights=30, seed=20, byz_count=30, drop_ppm=20_000),
    "byz22": dict(heights=70, seed=51, byz_count=22),
    "le-drop": dict(heights=20, seed=15, byz_count=21, drop_ppm=50_000, seed_byte_order=1),
}
BIG_ENDIAN = [c for c in CONFIGS if c != "le-drop"]
CRASH = ("crash", "crash-byz")

# the general kernel as control (it clears its rows): id -> (fields, instances per launch)
CONTROLS = {
    "n16-drop": (dict(n=16, heights=20, seed=21, drop_ppm=100_000), 96),
    "n100-drop": (dict(n=100, heights=20, seed=16, byz_count=33, drop_ppm=100_000), 8),
}

# the conditions' bounds (instances of 96); the minima the oracle gives over k < 10 and depths 2 and 3 are far above
MIN_LOWER = 8          # drop, fork, byz22, le-drop: committed height below the previous user's       [16]
MIN_DIFFERING = 16     # drop, fork, byz22, le-drop: a committed row that differs from the previous user's  [26]
MIN_DIFFERING_CRASH_BYZ = 64   # two thirds of 96: the instances that neither time out early nor stop within 3 heights [76]
MIN_MISS_INSIDE = 32   # crash, crash-byz: first block off the canonical tick above height 1           [63, 52]
MIN_MISS_AT_1 = 8      # crash, crash-byz: first such block at height 1                               [25, 12]


def config(cfg_id: str):
    from bftsim.configs import BftConfig
    if cfg_id in CONTROLS:
        return BftConfig(name=cfg_id, **CONTROLS[cfg_id][0])
    return BftConfig(n=64, name="reuse-" + cfg_id, **CONFIGS[cfg_id])


def instances(cfg_id: str) -> int:
    return CONTROLS[cfg_id][1] if cfg_id in CONTROLS else N_INST


@functools.lru_cache(maxsize=None)
def ref(cfg_id: str, k: int):
    """the oracle's run of range k (instances k * n .. k * n + n - 1): computed once per session, shared by every mode,
    left unchanged"""
    import oracle_lib as O
    n = instances(cfg_id)
    return O.run(config(cfg_id), k * n, n, threads=8)


def head(res, n: int):
    """the first n instances of a result"""
    from parity_util import FIELDS
    return {f: res[f][:n] for f in FIELDS}


def _committed_mask(res):
    H = res["proposer"].shape[1]
    return np.arange(H)[None, :] < res["committed_height"][:, None]        # column x - 1 is height x


def stale_counts(prev, new):
    """-> (instances of `new` that commit fewer heights than the same slot of `prev`: stale, valid-looking rows above
    the new height; instances with a row at a height <= the new committed height whose (proposer, variant, time_tick)
    differs from the previous user's. Above its own committed height the previous user reads as zeros, as the oracle
    returns it: the set holds there what still earlier users left, or nothing)"""
    lower = int((new["committed_height"] < prev["committed_height"]).sum())
    mask = _committed_mask(new)
    diff = np.zeros_like(mask)
    for f in ("proposer", "variant", "time_tick"):
        diff |= new[f] != prev[f]
    return lower, int((diff & mask).any(axis=1).sum())


def miss_counts(res):
    """-> (instances whose first committed block with proposer != 0 or time_tick != height - 1 lies above height 1,
    instances where it is height 1). Such a block cannot be what the predicted chains hashed (proposer 0 at tick
    height - 1), whatever the variant: a lower bound on the prediction misses."""
    H = res["proposer"].shape[1]
    off = ((res["proposer"] != 0) | (res["time_tick"] != np.arange(H)[None, :])) & _committed_mask(res)
    any_off, first = off.any(axis=1), off.argmax(axis=1)
    return int((any_off & (first >= 1)).sum()), int((any_off & (first == 0)).sum())


@functools.lru_cache(maxsize=None)
def assert_reuse_preconditions(cfg_id: str, depth: int, launches: int):
    """What a test with a ring of `depth` sets and `launches` launches over the ranges 0 .. launches - 1 relies on,
    asserted on the oracle's results alone: every launch k >= depth reuses the set of launch k - depth, and that set
    then holds rows that are stale for the new instances; with proposer crashes, every range misses predictions both
    at height 1 and inside a chain."""
    assert 2 <= depth < launches <= MAX_LAUNCHES
    n = instances(cfg_id)
    for k in range(depth, launches):
        lower, differing = stale_counts(ref(cfg_id, k - depth), ref(cfg_id, k))
        what = (cfg_id, "depth", depth, "launch", k)
        if cfg_id == "crash":
            assert differing == n, (what, "instances with a differing row", differing)
        else:
            need = MIN_DIFFERING_CRASH_BYZ if cfg_id == "crash-byz" else MIN_DIFFERING
            assert lower >= MIN_LOWER, (what, "instances with a lower committed height", lower)
            assert differing >= need, (what, "instances with a differing row", differing)
    if cfg_id in CRASH:
        for k in range(launches):
            inside, at1 = miss_counts(ref(cfg_id, k))
            assert inside >= MIN_MISS_INSIDE, (cfg_id, "range", k, "first miss above height 1", inside)
            assert at1 >= MIN_MISS_AT_1, (cfg_id, "range", k, "first miss at height 1", at1)
