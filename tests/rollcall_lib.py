"""ctypes wrapper of tests/emu/librollcall_host.so — TEST-ONLY host build of consensus-rs_amd/csrc/bft_rollcall.h (the
candidates, the view slot, the proposer, the PrePrepare match, the outcome and the row update the roll call's kernels run,
SPEC.md §11i) behind the observer's host build (tests/audit_lib.py); and the stand-alone sanitizer build of the same file
(tests/emu/_san/rollcall_san)."""
from __future__ import annotations

import ctypes
import os
import struct
import subprocess

import numpy as np

import audit_lib as AL
import rollcall_ref as RR
import timeline_lib as TLL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU_DIR = os.path.join(ROOT, "tests", "emu")
LIB = os.path.join(EMU_DIR, "librollcall_host.so")
SAN_EXE = os.path.join(EMU_DIR, "_san", "rollcall_san")
SRCS = [os.path.join(EMU_DIR, "rollcall_host.cpp"), os.path.join(ROOT, "consensus-rs_amd", "csrc", "bft_rollcall.h")] + TLL.SRCS[1:]
SAN = TLL.SAN
CNT_WORDS = 12
ROWS = dict(frames=4, last_height=1, last_frame=1, due=1, proposed=1, missed=1, won=1)      # words per row, all uint32
assert tuple(ROWS) == RR.ROWS
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
    subprocess.check_call(["g++", "-std=c++17", "-Wno-unknown-pragmas", "-DROLLCALL_HOST_MAIN", "-o", tmp, SRCS[0]] + SAN)
    os.replace(tmp, SAN_EXE)
    return SAN_EXE


def lib():
    global _lib
    if _lib is None:
        build()
        _lib = ctypes.CDLL(LIB)
        _lib.rollcall_host.restype = None
        _lib.rollcall_host.argtypes = [ctypes.c_void_p] * 7 + [ctypes.c_uint64] + [ctypes.c_uint32] * 4 + \
            [ctypes.c_void_p] * 15 + [ctypes.c_uint64, ctypes.c_void_p]
    return _lib


def _counts_of(rep) -> np.ndarray:
    counts = np.zeros(CNT_WORDS, np.uint64)
    counts[:10] = [rep["frames"], rep["out_of_range"], rep["views"], *rep["by_outcome"], rep["won"], rep["silent"],
                   rep["silent_instances"], rep["partial_instances"]]
    return counts


def report_of(counts) -> dict:
    c = [int(x) for x in counts]
    return dict(frames=c[0], out_of_range=c[1], views=c[2], by_outcome=c[3:6], won=c[6], silent=c[7], silent_instances=c[8],
                partial_instances=c[9])


def rollcall(stream, frame_off, inst_frame0, cfg, genesis: bytes, max_heights: int, tl_cap: int = 0, rec_cap: int = None,
             obs=None) -> dict:
    """The host build over a frame stream (behind audit_lib.observe, or the result of one passed in): the arrays of
    bftsim_rollcall_out shaped as rollcall_ref.rollcall shapes them, `records`, `report`, and `obs`."""
    obs = obs or AL.observe(stream, frame_off, inst_frame0, cfg, max_heights)
    F, ins, certs = TLL._inputs(obs, inst_frame0)
    n_inst, H, n = len(inst_frame0) - 1, max_heights, cfg.n
    rows = n_inst * n
    cap = n_inst * (H + (tl_cap or 4 * H + 64)) if rec_cap is None else rec_cap
    out = {k: np.zeros(max(rows, 1) * w, np.uint32) for k, w in ROWS.items()}
    out.update(inst_views=np.zeros(max(n_inst, 1), np.uint32), inst_silent=np.zeros(max(n_inst, 1) * 4, np.uint64),
               inst_flags=np.zeros(max(n_inst, 1), np.uint32), records=np.zeros(max(cap, 1), RR.RECORD))
    counts = np.zeros(CNT_WORDS, np.uint64)
    g = np.frombuffer(genesis, np.uint8)
    lib().rollcall_host(*[a.ctypes.data for a in ins], n_inst, n, tl_cap, H, int(cfg.seed_byte_order == 1), g.ctypes.data,
                        *[a.ctypes.data for a in certs], *[a.ctypes.data for a in out.values()], cap, counts.ctypes.data)
    got = {k: out[k][:rows * w].reshape((n_inst, n) + ((w,) if w > 1 else ())) for k, w in ROWS.items()}
    got.update(inst_views=out["inst_views"][:n_inst], inst_silent=out["inst_silent"][:n_inst * 4].reshape(n_inst, 4),
               inst_flags=out["inst_flags"][:n_inst], records=out["records"][:min(int(counts[2]), cap)])
    return dict(got, report=report_of(counts), obs=obs)


def san_input(obs, inst_frame0, cfg, genesis: bytes, tl_cap: int, max_heights: int, want) -> bytes:
    """stdin of the stand-alone program (tests/emu/rollcall_host.cpp): the observer's arrays `obs` (audit_lib.observe's)
    and the expected outputs `want` (rollcall_ref.rollcall's, under the same tl_cap)"""
    rec = obs["recs"]
    F, n_inst = len(obs["frame_status"]), len(inst_frame0) - 1
    parts = [struct.pack("<3Q4I", F, n_inst, len(want["records"]), cfg.n, tl_cap, max_heights, int(cfg.seed_byte_order == 1)),
             bytes(genesis), rec["code"][:F], rec["hx"][:F], rec["round"][:F], rec["digest"][:F], obs["frame_status"],
             obs["frame_signer"], np.asarray(inst_frame0, np.uint64), obs["cert_round"], obs["cert_digest"], obs["cert_frame"]] + \
        [want[k] for k in RR.ARRAYS] + [want["records"], _counts_of(want["report"])]
    return b"".join(p if isinstance(p, bytes) else np.ascontiguousarray(p).tobytes() for p in parts)
