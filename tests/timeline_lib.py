"""ctypes wrapper of tests/emu/libtimeline_host.so — TEST-ONLY host build of consensus-rs_amd/csrc/bft_timeline.h (the key
table, the vote, the row writers and the flags the chronicler's kernels run, SPEC.md §11h) behind the observer's host
build (tests/audit_lib.py); and the stand-alone sanitizer build of the same file (tests/emu/_san/timeline_san)."""
from __future__ import annotations

import ctypes
import os
import struct
import subprocess

import numpy as np

import audit_lib as AL
import timeline_ref as TR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU_DIR = os.path.join(ROOT, "tests", "emu")
LIB = os.path.join(EMU_DIR, "libtimeline_host.so")
SAN_EXE = os.path.join(EMU_DIR, "_san", "timeline_san")
SRCS = [os.path.join(EMU_DIR, "timeline_host.cpp")] + [
    os.path.join(ROOT, "consensus-rs_amd", "csrc", f) for f in ("bft_timeline.h", "bft_audit.h", "bft_wire.h", "bft_common.h",
                                                               "bft_wire_block.h", "bft_crypto.h")] + [
    os.path.join(ROOT, "include", "bftwire.h")]
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1"]
CNT_WORDS = 12
# the rows' arrays in the order of timeline_host's arguments: name -> (dtype, words per row)
ROWS = dict(prep_round=(np.uint16, 1), prep_digest=(np.uint8, 32), prep_voters=(np.uint64, 4), prep_frame=(np.uint32, 1),
            prep_quorums=(np.uint16, 1), rc_quorums=(np.uint16, 1), rc_max_round=(np.uint16, 1), rc_max_frame=(np.uint32, 1),
            rc_top_round=(np.uint16, 1), rc_frames=(np.uint32, 1), flags=(np.uint8, 1))
assert tuple(ROWS) == TR.ROWS
_lib = None


def _fresh(target):
    return os.path.exists(target) and all(os.path.getmtime(target) >= os.path.getmtime(s) for s in SRCS)


def build():
    if _fresh(LIB):
        return
    tmp = f"{LIB}.{os.getpid()}.tmp"      # private name + rename: safe under concurrent test workers
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-Wno-unknown-pragmas", "-o", tmp, SRCS[0]])
    os.replace(tmp, LIB)


def build_san():
    """the stand-alone program (its own main) under AddressSanitizer + UBSan; never loaded into python"""
    if _fresh(SAN_EXE):
        return SAN_EXE
    os.makedirs(os.path.dirname(SAN_EXE), exist_ok=True)
    tmp = f"{SAN_EXE}.{os.getpid()}.tmp"
    subprocess.check_call(["g++", "-std=c++17", "-Wno-unknown-pragmas", "-DTIMELINE_HOST_MAIN", "-o", tmp, SRCS[0]] + SAN)
    os.replace(tmp, SAN_EXE)
    return SAN_EXE


def lib():
    global _lib
    if _lib is None:
        build()
        _lib = ctypes.CDLL(LIB)
        _lib.timeline_host.restype = None
        _lib.timeline_host.argtypes = [ctypes.c_void_p] * 7 + [ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint32,
                                                               ctypes.c_uint32] + [ctypes.c_void_p] * 17
    return _lib


def _inputs(obs, inst_frame0):
    """the arrays the walk and the rows read, of an audit_lib.observe result"""
    rec = obs["recs"]
    F = len(obs["frame_status"])
    pad = lambda a: np.ascontiguousarray(a if len(a) else np.zeros((1,) + a.shape[1:], a.dtype))      # never empty
    return F, [pad(rec["code"][:F]), pad(rec["hx"][:F]), pad(rec["round"][:F]), pad(rec["digest"][:F]),
               pad(obs["frame_status"]), pad(obs["frame_signer"]), np.ascontiguousarray(inst_frame0, np.uint64)], \
        [np.ascontiguousarray(obs[k]) for k in ("cert_round", "cert_digest", "cert_frame")]


def report_of(counts) -> dict:
    return dict(zip(TR.REPORT, [int(x) for x in counts[:10]]))


def timeline(stream, frame_off, inst_frame0, cfg, max_heights: int, tl_cap: int = 0, obs=None) -> dict:
    """The host build over a frame stream (behind audit_lib.observe, or the result of one passed in): the arrays of
    bftsim_timeline_out shaped as timeline_ref.timeline shapes them, `report`, and `obs`."""
    obs = obs or AL.observe(stream, frame_off, inst_frame0, cfg, max_heights)
    F, ins, certs = _inputs(obs, inst_frame0)
    n_inst, H = len(inst_frame0) - 1, max_heights
    rows = n_inst * H
    out = {k: np.zeros(max(rows, 1) * w, dt) for k, (dt, w) in ROWS.items()}
    out.update(inst_flags=np.zeros(max(n_inst, 1), np.uint32), open_height=np.zeros(max(n_inst, 1), np.uint32))
    counts = np.zeros(CNT_WORDS, np.uint64)
    lib().timeline_host(*[a.ctypes.data for a in ins], n_inst, cfg.n, tl_cap, H, *[a.ctypes.data for a in certs],
                        *[a.ctypes.data for a in out.values()], counts.ctypes.data)
    got = {k: out[k][:rows * w].reshape((n_inst, H) + ((w,) if w > 1 else ())) for k, (_, w) in ROWS.items()}
    got.update(inst_flags=out["inst_flags"][:n_inst], open_height=out["open_height"][:n_inst])
    return dict(got, report=report_of(counts), obs=obs)


def san_input(got, inst_frame0, n: int, tl_cap: int, max_heights: int, want) -> bytes:
    """stdin of the stand-alone program (tests/emu/timeline_host.cpp): the observer's arrays of `got` (a timeline()
    result) and the expected outputs `want` (timeline_ref.timeline's, under the same tl_cap)"""
    obs = got["obs"]
    rec = obs["recs"]
    F, n_inst = len(obs["frame_status"]), len(inst_frame0) - 1
    counts = np.zeros(CNT_WORDS, np.uint64)
    counts[:10] = [want["report"][k] for k in TR.REPORT]
    parts = [struct.pack("<2Q4I", F, n_inst, n, tl_cap, max_heights, 0),
             rec["code"][:F], rec["hx"][:F], rec["round"][:F], rec["digest"][:F], obs["frame_status"], obs["frame_signer"],
             np.asarray(inst_frame0, np.uint64), obs["cert_round"], obs["cert_digest"], obs["cert_frame"]] + \
        [want[k] for k in TR.ARRAYS] + [counts]
    return b"".join(p if isinstance(p, bytes) else np.ascontiguousarray(p).tobytes() for p in parts)
