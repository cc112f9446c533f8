"""CPU: the archiver's pick, emit and heights steps (consensus-rs_amd/csrc/bft_archive.h, host build
tests/emu/archive_host.cpp over the observer's host build) against the independent Python archiver
(tests/archive_ref.py), array for array and slot for slot, over the reference traces, hostile variants of them and
one-height streams of 67 and 171 voters (tests/archive_cases.py); every archived ledger through the Python importer
(tests/ledger_ref.py); the emitter as a stand-alone program under ASan + UBSan; the C ABI's bindings and argument
checks."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import archive_cases as AC      # first: it puts oracle/ on the path
import archive_lib as ARL
import archive_ref as ARC
import audit_lib as AL
import audit_ref as AR
import ledger_ref as LR
import trace_ref as TR


@pytest.mark.parametrize("name", AC.NAMES)
def test_host_build_equals_reference(name):
    """the host build's ledger and arrays equal the Python archiver's, its observer half equals the Python observer,
    and the case shows what it was built to show under the Python importer"""
    c = AC.case(name)
    cfg, want = c["cfg"], c["want"]
    got = ARL.archive(c["stream"], c["off"], c["f0"], cfg, c["heights"], c["key_cap"])
    assert got["errors"] == 0
    AR.assert_same(got["audit"], want["audit"])
    ARC.assert_same(got, want)
    verdict = LR.verify(got["hdr"], got["hdr_len"], got["slot_bytes"], c["heights"], cfg, TR.genesis_hash(cfg))
    print(name, "archive", want["status"].tolist(), "import", verdict["status"].tolist(), want["report"])
    AC.check_expectations(c, got["status"], verdict)


def test_reference_ledger_layout_is_the_exporters():
    """archive_ref's headers are SPEC.md §7 Headers whose votes are the certificate's voters, ascending"""
    c = AC.case("cfg1")
    for x, h in enumerate(c["want"]["headers"][0]):
        d = LR.decode(h)
        assert d is not None and d["height"] == x + 1 and len(d["votes"]) == 4
        assert LR.block_hash(d) == bytes(c["ref"]["res"]["block_hash"][0, x])
        assert len(h) <= ARC.slot_bytes(5)


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_emitter_program_under_asan_ubsan():
    """the stand-alone program (its own main, run directly): a header from every truncation and every single-byte flip
    of each PrePrepare frame of the cfg1 stream, read from heap buffers of exactly the frame's length and written to a
    heap slot of exactly bftsim_ledger_slot_bytes(5)"""
    exe = ARL.build_san()
    c = AC.case("cfg1")
    ms = c["ref"]["inst"][0][3]
    off = [int(x) for x in c["off"]]
    frames = [c["stream"][off[k]:off[k + 1]] for k, m in enumerate(ms) if m["code"] == 1]
    assert len(frames) >= 6
    cfg = c["cfg"]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe], input=AL.san_input(cfg.address_bytes(), cfg.n, frames), capture_output=True, env=env, timeout=600)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    cases = sum(len(f) for f in frames) * 4
    assert r.stdout.decode().strip() == f"ok {len(frames)} frames {cases} cases"
    assert b"runtime error" not in r.stderr and b"AddressSanitizer" not in r.stderr, r.stderr[-4000:]


def test_entry_points_are_bound_and_check_arguments():
    """bound; a null handle, report, hdr or hdr_len, a short slot and every refusal of the observer are BFTSIM_EINVAL
    before any device work, and nothing is written (this runs without a GPU: the handle of a create that could not
    reach a device still checks arguments)"""
    from bftsim import _abi, ledger, runtime
    from bftsim.configs import cfg1 as mk
    L = runtime.lib()
    rep, arep = _abi.CArchiveReport(), _abi.CAuditReport()
    hdr, lens, out, arrs = _abi.alloc_archive(1, 6, 1024)
    assert L.bftsim_archive_trace(None, None, 0, None, 0, None, 0, 1, 0, hdr.ctypes.data, 1024, lens.ctypes.data, None, None,
                                  None, ctypes.byref(rep)) == -1
    assert L.bftsim_archive_last_trace(None, 0, 0, 0, hdr.ctypes.data, 1024, lens.ctypes.data, None, None, None,
                                       ctypes.byref(rep)) == -1
    assert L.bftsim_archive_last_ms(None, None, None, None, None) == -1
    for k in ("archive_trace", "archive_last_trace", "archive_ms"):
        assert hasattr(runtime.Simulator, k)
    assert callable(ledger.unpack) and hasattr(ledger.Archive, "names")
    c, keep = _abi.to_cconfig(mk(True, heights=6))
    h = ctypes.c_void_p()
    L.bftsim_create(ctypes.byref(c), 0, ctypes.byref(h))
    assert h.value
    slot = L.bftsim_ledger_slot_bytes(5)
    assert slot == ARC.slot_bytes(5) == ARL.slot_bytes(5) and slot <= 1024
    stream = np.zeros(16, np.uint8)

    def call(off=(0, 8, 16), f0=(0, 2), frames=2, inst=1, heights=6, nbytes=16, hdr_p=hdr.ctypes.data, slot_b=1024,
             len_p=lens.ctypes.data, rep_p=ctypes.byref(rep)):
        off, f0 = np.array(off, np.uint64), np.array(f0, np.uint64)
        return L.bftsim_archive_trace(h, stream.ctypes.data, nbytes, off.ctypes.data, frames, f0.ctypes.data, inst, heights, 0,
                                      hdr_p, slot_b, len_p, ctypes.byref(out), None, ctypes.byref(arep), rep_p)

    rep.headers, arep.frames = 77, 78
    hdr[...], lens[...] = 7, 7
    for a in arrs.values():
        a[...] = 7
    assert call(rep_p=None) == -1 and call(hdr_p=None) == -1 and call(len_p=None) == -1
    assert call(slot_b=slot - 1) == -1 and call(slot_b=0) == -1
    assert b"slot_bytes" in L.bftsim_last_error(h)
    assert call(off=(0, 9, 8), nbytes=8) == -1                          # the observer's refusals
    assert call(off=(0, 8, 15)) == -1
    assert call(f0=(1, 2)) == -1 and call(f0=(0, 1)) == -1 and call(f0=(0, 2, 1, 2), inst=3) == -1
    assert call(heights=0) == -1 and call(heights=65536) == -1 and call(frames=1 << 32) == -1
    assert len(L.bftsim_last_error(h)) > 0 and rep.headers == 77 and arep.frames == 78
    assert (hdr == 7).all() and (lens == 7).all() and all((a == 7).all() for a in arrs.values())
    del keep


def test_new_structs_bound_in_integration_md():
    """bftsim_archive_report / bftsim_archive_out: INTEGRATION.md's #[repr(C)] structs against the header, by the checker
    of test_integration_binding (field names, types, offsets and sizes as gcc lays them out); the ctypes mirrors too"""
    import re
    import test_integration_binding as B
    from bftsim import _abi
    txt = re.sub(r"struct (bftsim_archive_\w+) \{(.*?)\};\s*typedef struct \1 \1;", r"typedef struct \1 {\2} \1;",
                 B.header_text(), flags=re.S)
    decls = {k: v for k, v in B.c_struct_decls(txt).items() if k.startswith("bftsim_archive_")}
    assert set(decls) == {"bftsim_archive_report", "bftsim_archive_out"}
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
    for name, cls in (("bftsim_archive_report", _abi.CArchiveReport), ("bftsim_archive_out", _abi.CArchiveOut)):
        assert ctypes.sizeof(cls) == lay[(name, "sizeof")]
        assert [f for f, _ in cls._fields_] == [f for f, _ in decls[name]]
        for f, _ in cls._fields_:
            assert getattr(cls, f).offset == lay[(name, f)], (name, f)
    for k in ("BFTSIM_ARCHIVE_OK", "BFTSIM_ARCHIVE_NONE", "BFTSIM_ARCHIVE_NO_PROPOSAL"):
        assert k in consts
