"""The roll call on the CPU (SPEC.md §11i): the Python reference on the hand-made rules and against the runs, the host
build of consensus-rs_amd/csrc/bft_rollcall.h against the reference on every case, the same code as a stand-alone
program under AddressSanitizer + UBSan, the ABI and the documents."""
import ctypes
import json
import os
import re
import subprocess

import numpy as np
import pytest

import rollcall_cases as RC
import rollcall_lib as RL
import rollcall_ref as RR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
CASES = RC.stream_cases()


def pinned(w) -> dict:
    """a case's full expected output as plain data (tests/golden/rollcall_*.json)"""
    out = {k: np.asarray(w[k]).tolist() for k in RR.ARRAYS}
    out["records"] = [[int(x) for x in r] for r in w["records"]]
    out["report"] = w["report"]
    return out


def test_reference_on_the_handmade_rules():
    RC.check_handmade(RC.handmade())


def test_hundred_validators_reach_word_one():
    c = RC.hundred()
    w = c["want"]
    assert RR.silent_of(w, 0) == [70, 80] and int(w["inst_silent"][0, 0]) == 0
    assert RR.missed_of(w, 0)[-1] == (1, c["round"], 80) and int(w["missed"][0, 80]) == 1
    assert int(w["frames"][0, 99, 1]) == 1 and int(w["frames"][0, 66, 3]) == 1


@pytest.mark.parametrize("name", list(CASES))
def test_host_build_equals_reference(name):
    c = CASES[name]()
    got = RL.rollcall(c["stream"], c["off"], c["f0"], c["cfg"], c["genesis"], c["heights"])
    RR.assert_same(got, c["want"])


def test_host_build_tl_cap_two_and_record_prefix():
    c = RC.handmade()
    got = RL.rollcall(c["stream"], c["off"], c["f0"], c["cfg"], c["genesis"], c["heights"], tl_cap=2)
    RR.assert_same(got, c["want_cap2"])
    got = RL.rollcall(c["stream"], c["off"], c["f0"], c["cfg"], c["genesis"], c["heights"], rec_cap=7, obs=got["obs"])
    RR.assert_same(got, c["want"], rec_cap=7)


@pytest.mark.parametrize("name", ["handmade", "n4"])
def test_sanitizer_program(name):
    """the host build as a stand-alone program under ASan + UBSan, a child process fed on stdin"""
    exe = RL.build_san()
    c = CASES[name]()
    import audit_lib as AL
    obs = AL.observe(c["stream"], c["off"], c["f0"], c["cfg"], c["heights"])
    for tl_cap, want in ((0, c["want"]), (2, c.get("want_cap2"))):
        if want is None:
            continue
        data = RL.san_input(obs, c["f0"], c["cfg"], c["genesis"], tl_cap, c["heights"], want)
        r = subprocess.run([exe], input=data, capture_output=True, timeout=120)
        assert r.returncode == 0 and r.stdout.startswith(b"ok "), (r.returncode, r.stdout[-400:], r.stderr[-2000:])


def test_crash_case_premises_and_closure():
    c = RC.crash()
    w, cfg = c["want"], c["cfg"]
    assert cfg.byz_count == 0 and cfg.drop_ppm == 0 and not cfg.silent
    RC.check_against_run(w, cfg, c["ref"]["res"], c["ref"]["first"])
    missed = [RR.missed_of(w, i) for i in range(4)]
    assert any(r == 0 for m in missed for _, r, _ in m), missed      # a MISSED view at round 0,
    assert any(r > 0 for m in missed for _, r, _ in m), missed       # one at a round above 0,
    assert any(not m for m in missed), missed                        # and an instance with none
    assert w["report"]["silent"] == 0 and w["report"]["by_outcome"][2] == 0
    assert pinned(w) == json.load(open(os.path.join(GOLDEN, "rollcall_crash.json")))


def test_n4_pinned():
    assert pinned(RC.twins("n4")["want"]) == json.load(open(os.path.join(GOLDEN, "rollcall_n4.json")))


def test_cfg1_silent_validator():
    c = RC.cfg1()
    w, cfg = c["want"], c["cfg"]
    assert list(cfg.silent) == [4] and RR.silent_of(w, 0) == [4]
    RC.check_against_run(w, cfg, c["ref"]["res"], 0)
    views = RR.views_of(w, 0)
    assert any(p == 4 for _, _, p, _, _, _ in views)
    assert all(oc == RR.MISSED for _, _, p, oc, _, _ in views if p == 4)


def test_entry_points_bound_and_refusals():
    from bftsim import _abi, runtime
    L = runtime.lib()
    for name in ("bftsim_rollcall_trace", "bftsim_rollcall_last_trace", "bftsim_rollcall_last_ms"):
        assert getattr(L, name).argtypes is not None
    assert ctypes.sizeof(_abi.CRollCallReport) == 80 and _abi.ROLLCALL_RECORD.itemsize == 32
    assert ctypes.sizeof(_abi.CRollCallOut) == 12 * 8
    rep = _abi.CRollCallReport()
    assert L.bftsim_rollcall_trace(None, None, 0, None, 0, None, 0, 1, 0, 0, None, ctypes.byref(rep), None, None, None, None) != 0
    assert L.bftsim_rollcall_last_trace(None, 0, 0, 0, 0, None, None, None, None, None, None) != 0
    assert L.bftsim_rollcall_last_ms(None, None, None, None, None, None, None) != 0


def test_new_structs_bound_in_integration_md():
    hdr = open(os.path.join(ROOT, "include", "bftsim.h")).read()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in re.findall(r"struct (bftsim_rollcall_\w+) \{", hdr) + re.findall(r"int (bftsim_rollcall_\w+)\(", hdr):
        assert name in doc, name
