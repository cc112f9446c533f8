"""ctypes wrapper of tests/emu/libaccuse_host.so — TEST-ONLY host build of consensus-rs_amd/csrc/bft_accuse.h (the view
table, the group step and the record the accuser's kernels run, SPEC.md §11g) behind the observer's host build
(tests/audit_lib.py); and the stand-alone sanitizer build of the same file (tests/emu/_san/accuse_san)."""
from __future__ import annotations

import ctypes
import os
import struct
import subprocess

import numpy as np

import audit_lib as AL
from accuse_ref import RECORD

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU_DIR = os.path.join(ROOT, "tests", "emu")
LIB = os.path.join(EMU_DIR, "libaccuse_host.so")
SAN_EXE = os.path.join(EMU_DIR, "_san", "accuse_san")
SRCS = [os.path.join(EMU_DIR, "accuse_host.cpp")] + [
    os.path.join(ROOT, "consensus-rs_amd", "csrc", f) for f in ("bft_accuse.h", "bft_audit.h", "bft_wire.h", "bft_common.h",
                                                               "bft_wire_block.h", "bft_crypto.h")] + [
    os.path.join(ROOT, "include", "bftwire.h")]
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1"]
CNT_WORDS = 8
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
    subprocess.check_call(["g++", "-std=c++17", "-Wno-unknown-pragmas", "-DACCUSE_HOST_MAIN", "-o", tmp, SRCS[0]] + SAN)
    os.replace(tmp, SAN_EXE)
    return SAN_EXE


def lib():
    global _lib
    if _lib is None:
        build()
        _lib = ctypes.CDLL(LIB)
        _lib.accuse_host.restype = ctypes.c_uint64
        _lib.accuse_host.argtypes = [ctypes.c_void_p] * 7 + [ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint32,
                                                             ctypes.c_uint32] + [ctypes.c_void_p] * 4 + \
            [ctypes.c_uint64, ctypes.c_void_p]
    return _lib


def _inputs(obs, inst_frame0):
    """the arrays the walk reads, of an audit_lib.observe result"""
    rec = obs["recs"]
    F = len(obs["frame_status"])
    pad = lambda a: np.ascontiguousarray(a if len(a) else np.zeros((1,) + a.shape[1:], a.dtype))      # never empty
    return F, [pad(rec["code"][:F]), pad(rec["hx"][:F]), pad(rec["round"][:F]), pad(rec["digest"][:F]),
               pad(obs["frame_status"]), pad(obs["frame_signer"]), np.ascontiguousarray(inst_frame0, np.uint64)]


def accuse(stream, frame_off, inst_frame0, cfg, max_heights: int, view_cap: int = 0, rec_cap=None, obs=None) -> dict:
    """The host build over a frame stream (behind audit_lib.observe, or the result of one passed in): the arrays of
    bftsim_accuse_out shaped as accuse_ref.accuse shapes them, `report`, and `obs`."""
    obs = obs or AL.observe(stream, frame_off, inst_frame0, cfg, max_heights)
    F, ins = _inputs(obs, inst_frame0)
    n_inst = len(inst_frame0) - 1
    cap = F if rec_cap is None else rec_cap
    pair, acc = np.zeros(max(F, 1), np.uint32), np.zeros((max(n_inst, 1), 4), np.uint64)
    flags, recs, counts = np.zeros(max(n_inst, 1), np.uint32), np.zeros(max(cap, 1), RECORD), np.zeros(CNT_WORDS, np.uint64)
    total = lib().accuse_host(*[a.ctypes.data for a in ins], n_inst, F, cfg.n, view_cap, max_heights, pair.ctypes.data,
                              acc.ctypes.data, flags.ctypes.data, recs.ctypes.data, cap, counts.ctypes.data)
    c = [int(x) for x in counts]
    assert total == c[0]
    report = dict(records=c[0], by_code=c[1:4], accused=c[4], accused_instances=c[5], view_overflows=c[6])
    return dict(frame_pair=pair[:F], inst_accused=acc[:n_inst], inst_flags=flags[:n_inst], records=recs[:min(total, cap)],
                report=report, obs=obs, counts=counts)


def san_input(got, inst_frame0, n: int, view_cap: int, max_heights: int, rec_cap: int, want) -> bytes:
    """stdin of the stand-alone program (tests/emu/accuse_host.cpp): the observer's arrays of `got` (an accuse() result)
    and the expected outputs `want` (accuse_ref.accuse's, under the same view_cap and rec_cap)"""
    obs = got["obs"]
    rec = obs["recs"]
    F, n_inst = len(obs["frame_status"]), len(inst_frame0) - 1
    total = want["report"]["records"]
    assert len(want["records"]) == min(total, rec_cap)
    w = want["report"]
    counts = np.array([w["records"]] + list(w["by_code"]) + [w["accused"], w["accused_instances"], w["view_overflows"], 0],
                      np.uint64)
    parts = [struct.pack("<4Q4I", F, n_inst, rec_cap, total, n, view_cap, max_heights, 0),
             rec["code"][:F], rec["hx"][:F], rec["round"][:F], rec["digest"][:F], obs["frame_status"], obs["frame_signer"],
             np.asarray(inst_frame0, np.uint64), want["frame_pair"], want["inst_accused"], want["inst_flags"],
             want["records"], counts]
    return b"".join(p if isinstance(p, bytes) else np.ascontiguousarray(p).tobytes() for p in parts)
