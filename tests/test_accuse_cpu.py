"""CPU: the accuser (SPEC.md §11g). The Python reference alone (tests/accuse_ref.py) first shows what it is for: on the
twinned trace of the pinned N = 7 case it accuses equivocators and nobody else, each record naming the two frames that
prove it; on the plain trace it finds nothing; a forged sender is never accused. Then the host build of the walk and the
compaction (consensus-rs_amd/csrc/bft_accuse.h, tests/emu/accuse_host.cpp) against that reference array for array, on
those traces and on a hand-made stream with one instance per rule; the same code as a stand-alone program under
ASan + UBSan; the C ABI's bindings and argument checks."""
import ctypes
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import accuse_cases as XC       # first: it puts oracle/ on the path
import accuse_lib as XL
import accuse_ref as XR
import audit_ref as AR
import twins_ref as TW

HERE = os.path.dirname(__file__)
PIN = json.load(open(os.path.join(HERE, "golden", "accuse_n7.json")))


def _host(c, want_key="want", **kw):
    """the host build over a case, asserted equal to the reference under the same caps"""
    got = XL.accuse(c["stream"], c["off"], c["f0"], c["cfg"], c["heights"], **kw)
    XR.assert_same({k: got[k] for k in XR.ARRAYS + ("report",)}, c[want_key])
    AR.assert_same({k: got["obs"][k] for k in AR.ARRAYS + ("report",)}, c["want"]["audit"])
    return got


def _honest_never_accused(c):
    ref, want = c["ref"], c["want"]
    for i in range(ref["n"]):
        byz = TW.byzantine_senders(TW.log_of(ref["res"], i))
        assert set(XR.accused(want, i)) <= byz <= XC.seeded_byz(c["cfg"], ref["first"] + i), i
        assert not set(XR.accused(want, i)) & set(ref["forged"])


def test_reference_on_the_twinned_n7_trace():
    """285 frames, 15 twins: 15 records, one per twin (no group had an earlier frame), each pairing a twin with the
    original before it; the accused are Byzantine validators of their instance, and every twin's signer is accused.
    Instance 3 has Byzantine validators but none of them ever proposes, so nobody equivocates there and nobody is
    accused: accused is a subset of the Byzantine set, not the set"""
    c = XC.twins("n7")
    want, meta = c["want"], c["meta"]
    tw = (meta[:, 2] & TW.TWIN) != 0
    assert len(meta) == PIN["frames"] == 285 and int(tw.sum()) == PIN["twins"] == 15
    assert want["records"].tolist() == [tuple(r) for r in PIN["records"]]
    assert [XR.accused(want, i) for i in range(3)] == PIN["accused"] and want["report"] == PIN["report"]
    _honest_never_accused(c)
    st, signer = want["audit"]["frame_status"], want["audit"]["frame_signer"]
    assert (st == AR.ST_OK).all()
    for k in np.nonzero(tw)[0]:                                   # every OK twin's signer is accused in its instance
        assert int(signer[k]) in XR.accused(want, int(meta[k, 3]))
    assert want["report"]["records"] <= int(tw.sum())
    assert want["records"]["frame_b"].tolist() == np.nonzero(tw)[0].tolist()      # equality: the twin closes its group
    assert (want["records"]["frame_a"] == want["records"]["frame_b"] - 1).all()
    # a record is a proof: two accepted frames of one signer, code, height and round with two digests
    for r in want["records"]:
        a, b = (AR.parse(c["stream"][int(c["off"][k]):int(c["off"][k + 1])]) for k in (r["frame_a"], r["frame_b"]))
        assert signer[r["frame_a"]] == signer[r["frame_b"]] == r["signer"]
        assert (a["code"], a["height"], a["round"]) == (b["code"], b["height"], b["round"]) == (r["code"], r["height"], r["round"])
        assert a["digest"] != b["digest"]


def test_reference_on_the_plain_n7_trace():
    """without the twins every validator's frames carry one digest per group: nothing to accuse"""
    want = XC.twins("n7", True)["want"]
    assert want["report"] == dict(records=0, by_code=[0, 0, 0], accused=0, accused_instances=0, view_overflows=0)
    assert (want["frame_pair"] == XR.NONE).all() and not want["inst_accused"].any() and len(want["records"]) == 0


def test_reference_on_the_lossy_forged_n4_trace():
    """N = 4, 10 % drops, validator 2 forged (a Byzantine validator of instances 3 and 5): its frames, twins included,
    are NOT_VALIDATOR, so it is never accused; instance 4's equivocator, validator 3, is; no honest validator is"""
    c = XC.twins("n4")
    want, meta, ref = c["want"], c["meta"], c["ref"]
    assert ref["forged"] == (2,) and len(meta) == 1045
    tw = (meta[:, 2] & TW.TWIN) != 0
    st, signer = want["audit"]["frame_status"], want["audit"]["frame_signer"]
    forged = (meta[:, 2] & 1) != 0
    assert (st[forged] == AR.ST_NOT_VALIDATOR).all() and (st[~forged] == AR.ST_OK).all()
    assert int(tw.sum()) == 12 and int((tw & forged).sum()) == 6
    _honest_never_accused(c)
    assert [XR.accused(want, i) for i in range(3)] == [[], [3], []]
    assert want["report"] == dict(records=6, by_code=[2, 2, 2], accused=1, accused_instances=1, view_overflows=0)
    assert want["records"]["frame_b"].tolist() == np.nonzero(tw & ~forged)[0].tolist()
    for k in np.nonzero(tw & ~forged)[0]:
        assert int(signer[k]) in XR.accused(want, int(meta[k, 3]))
    assert XC.twins("n4", True)["want"]["report"]["records"] == 0


def test_reference_on_the_handmade_rules():
    XC.check_handmade(XC.handmade())


@pytest.mark.parametrize("case,plain", [("n7", False), ("n7", True), ("n4", False), ("n4", True)])
def test_host_build_equals_reference_on_twins(case, plain):
    _host(XC.twins(case, plain))


def test_host_build_equals_reference_on_the_handmade_rules():
    """three digests, a duplicate, an unrecoverable first frame, other rounds and codes, a round above 2^32, heights 0
    and max_heights + 1, RoundChanges, a SEAL_FOREIGN Commit, a pair 71 frames apart, an empty instance, 70 views; then
    view_cap 2 and rec_cap 1 over the same stream"""
    c = XC.handmade()
    got = _host(c)
    assert got["report"]["records"] == 8
    _host(c, "want_cap2", view_cap=2)
    one = _host(c, "want_rec1", rec_cap=1)
    assert len(one["records"]) == 1 and one["report"]["records"] == 8
    none = XL.accuse(c["stream"], c["off"], c["f0"], c["cfg"], c["heights"], rec_cap=0, obs=got["obs"])
    assert len(none["records"]) == 0 and none["report"] == c["want"]["report"]
    assert np.array_equal(none["frame_pair"], c["want"]["frame_pair"])


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_program_under_asan_ubsan():
    """the stand-alone program (its own main, run directly): the same walk and compaction over every case, from and
    into heap buffers of exactly the counted sizes (the view tables too), compared there with the reference"""
    exe = XL.build_san()
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    hm = XC.handmade()
    obs = XL.accuse(hm["stream"], hm["off"], hm["f0"], hm["cfg"], hm["heights"])
    runs = [("handmade", hm, obs, "want", 0, len(hm["off"]) - 1), ("view_cap 2", hm, obs, "want_cap2", 2, len(hm["off"]) - 1),
            ("rec_cap 1", hm, obs, "want_rec1", 0, 1)]
    for case, plain in (("n7", False), ("n7", True), ("n4", False)):
        c = XC.twins(case, plain)
        runs.append((f"{case} plain={plain}", c, XL.accuse(c["stream"], c["off"], c["f0"], c["cfg"], c["heights"]), "want", 0,
                     len(c["off"]) - 1))
    for name, c, got, key, view_cap, rec_cap in runs:
        want = c[key]
        r = subprocess.run([exe], input=XL.san_input(got, c["f0"], c["cfg"].n, view_cap, c["heights"], rec_cap, want),
                           capture_output=True, env=env, timeout=120)
        assert r.returncode == 0, (name, r.returncode, r.stdout[-2000:], r.stderr[-4000:])
        assert r.stdout.decode().strip() == f"ok {len(c['off']) - 1} frames {want['report']['records']} records", name
        assert b"runtime error" not in r.stderr and b"AddressSanitizer" not in r.stderr, r.stderr[-4000:]


def test_entry_points_are_bound_and_check_arguments():
    """bound; a null handle, out or report and a rec_cap without records refused, and the observer's argument errors
    are this call's, all before any device work and with nothing written (this runs without a GPU)"""
    from bftsim import _abi, runtime, trace
    from bftsim.configs import cfg1 as mk
    L = runtime.lib()
    rep, arep = _abi.CAccuseReport(), _abi.CAuditReport()
    o, arrs = _abi.alloc_accuse(2, 1)
    assert L.bftsim_accuse_trace(None, None, 0, None, 0, None, 0, 1, 0, 0, ctypes.byref(o), None, None, ctypes.byref(rep)) == -1
    assert L.bftsim_accuse_last_trace(None, 0, 0, 0, 0, ctypes.byref(o), None, None, ctypes.byref(rep)) == -1
    assert L.bftsim_accuse_last_ms(None, None, None, None, None) == -1
    for name in ("accuse_trace", "accuse_last_trace", "accuse_ms"):
        assert callable(getattr(runtime.Simulator, name))
    assert callable(trace.Accusation.proof) and callable(trace.Accusation.accused)
    assert _abi.ACCUSE_RECORD.itemsize == 32 and _abi.ACCUSE_RECORD == XR.RECORD
    c, keep = _abi.to_cconfig(mk(True, heights=6))
    h = ctypes.c_void_p()
    L.bftsim_create(ctypes.byref(c), 0, ctypes.byref(h))
    assert h.value
    stream = np.zeros(16, np.uint8)
    for a in arrs.values():
        a.view(np.uint8)[...] = 7
    rep.records, arep.frames = 77, 78

    def call(off, f0, frames=2, inst=1, heights=6, out=o, rep=rep, nbytes=16):
        off, f0 = np.array(off, np.uint64), np.array(f0, np.uint64)
        return L.bftsim_accuse_trace(h, stream.ctypes.data, nbytes, off.ctypes.data, frames, f0.ctypes.data, inst, heights, 0,
                                     0, ctypes.byref(out) if out is not None else None, None, ctypes.byref(arep),
                                     ctypes.byref(rep) if rep is not None else None)

    no_recs = _abi.CAccuseOut()
    no_recs.rec_cap = 4                                                 # records NULL
    assert call([0, 8, 16], [0, 2], rep=None) == -1                     # null report
    assert call([0, 8, 16], [0, 2], out=None) == -1                     # null out
    assert call([0, 8, 16], [0, 2], out=no_recs) == -1                  # rec_cap without records
    assert call([0, 9, 8], [0, 2], nbytes=8) == -1                      # the observer's: frame_off decreases
    assert call([0, 8, 15], [0, 2]) == -1
    assert call([0, 8, 16], [1, 2]) == -1
    assert call([0, 8, 16], [0, 2, 1, 2], inst=3) == -1
    assert call([0, 8, 16], [0, 2], heights=0) == -1
    assert call([0, 8, 16], [0, 2], frames=1 << 32) == -1
    assert L.bftsim_accuse_last_trace(h, 0, 1, 0, 0, ctypes.byref(o), None, ctypes.byref(arep), ctypes.byref(rep)) == -1   # no kept trace
    assert len(L.bftsim_last_error(h)) > 0 and rep.records == 77 and arep.frames == 78       # nothing written
    assert all((a.view(np.uint8) == 7).all() for a in arrs.values())
    del keep


def test_new_structs_bound_in_integration_md():
    """bftsim_accuse_record / _report / _out: INTEGRATION.md's #[repr(C)] structs against the header, by the checker of
    test_integration_binding (field names, types, offsets and sizes as gcc lays them out); the ctypes mirrors and the
    numpy record too"""
    import re
    import test_integration_binding as B
    from bftsim import _abi
    txt = re.sub(r"struct (bftsim_accuse_\w+) \{(.*?)\};\s*typedef struct \1 \1;", r"typedef struct \1 {\2} \1;",
                 B.header_text(), flags=re.S)
    decls = {k: v for k, v in B.c_struct_decls(txt).items() if k.startswith("bftsim_accuse_")}
    assert set(decls) == {"bftsim_accuse_record", "bftsim_accuse_report", "bftsim_accuse_out"}
    src = B.strip_rust_comments(B.rust_blocks())
    rs, consts = B.rust_structs(src), B.rust_consts(src)
    lay = B.gcc_layout({k: [f for f, _ in v] for k, v in decls.items()})
    for name, fields in decls.items():
        assert [f for f, _ in rs[name]] == [f for f, _ in fields], name
        assert [B.canon_rust(B.parse_rust_type(t), consts) for _, t in rs[name]] == [t for _, t in fields], name
        size, _, offs = B.struct_layout(name, rs, consts, {})
        assert size == lay[(name, "sizeof")]
        for f, o in offs.items():
            assert o == lay[(name, f)], (name, f)
    for name, cls in (("bftsim_accuse_report", _abi.CAccuseReport), ("bftsim_accuse_out", _abi.CAccuseOut)):
        assert ctypes.sizeof(cls) == lay[(name, "sizeof")]
        assert [f for f, _ in cls._fields_] == [f for f, _ in decls[name]]
        for f, _ in cls._fields_:
            assert getattr(cls, f).offset == lay[(name, f)], (name, f)
    assert _abi.ACCUSE_RECORD.itemsize == lay[("bftsim_accuse_record", "sizeof")] == 32
    for f, _ in decls["bftsim_accuse_record"]:
        assert _abi.ACCUSE_RECORD.fields[f][1] == lay[("bftsim_accuse_record", f)], f
    assert consts["BFTSIM_ACCUSE_VIEW_OVERFLOW"].strip() == "1"
