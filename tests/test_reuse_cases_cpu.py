"""CPU: the premises of tests/test_gpu_set_reuse.py, on the oracle alone (tests/reuse_cases.py): launches over distinct
instance ranges leave rows in a row-table set that are stale for the set's next user -- lower committed heights, rows
that differ -- and the proposer-crash configurations miss predictions in every range, from height 1 and from inside a
chain. Without these a reused set would hold what the new launch writes anyway, and a skipped repair would pass."""
import numpy as np
import pytest

import reuse_cases as R


@pytest.mark.parametrize("depth", [2, 3])
@pytest.mark.parametrize("cfg_id", list(R.CONFIGS))
def test_reuse_preconditions(cfg_id, depth):
    R.assert_reuse_preconditions(cfg_id, depth, R.MAX_LAUNCHES)


@pytest.mark.parametrize("cfg_id", ["drop", "fork", "byz22"])
def test_lossy_big_endian_configs_stay_on_the_canonical_tick(cfg_id):
    """every committed block of these has proposer 0 at tick = height - 1: a prediction can miss only on the variant.
    (Why the crash configurations are the repair cases; if this ever fails the table's comment is out of date, not the
    product.)"""
    for k in range(R.MAX_LAUNCHES):
        assert R.miss_counts(R.ref(cfg_id, k)) == (0, 0), (cfg_id, k)


def test_counts_on_constructed_results():
    """stale_counts and miss_counts on hand-made results: rows above the new committed height do not count"""
    def res(ch, prop, tick, var=None):
        prop = np.array(prop, np.uint16)
        return dict(committed_height=np.array(ch, np.uint32), proposer=prop, time_tick=np.array(tick, np.uint32),
                    variant=np.zeros_like(prop, np.uint8) if var is None else np.array(var, np.uint8))
    prev = res([3, 1, 3, 2], [[0, 0, 0], [0, 9, 9], [0, 0, 0], [0, 0, 0]], [[0, 1, 2]] * 4)
    new = res([2, 3, 3, 3], [[0, 0, 7], [0, 0, 0], [0, 5, 0], [0, 0, 0]], [[0, 1, 2]] * 4,
              [[0, 0, 0], [0, 0, 0], [0, 0, 0], [0, 0, 1]])
    # instance 0: lower; its differing row is above its height. 1: differs from prev's rows 2 and 3 (as the oracle
    # returned them). 2: differs at height 2. 3: the variant differs at height 3
    assert R.stale_counts(prev, new) == (1, 3)
    r = res([3, 3, 2, 0], [[0, 0, 4], [3, 0, 0], [0, 0, 4], [5, 5, 5]], [[0, 1, 2], [0, 1, 2], [0, 1, 2], [9, 9, 9]])
    assert R.miss_counts(r) == (1, 1)
    r = res([3, 3], [[0, 0, 0], [0, 0, 0]], [[0, 1, 3], [1, 2, 3]])
    assert R.miss_counts(r) == (1, 1)
