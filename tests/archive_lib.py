"""ctypes wrapper of tests/emu/libarchive_host.so — TEST-ONLY host build of consensus-rs_amd/csrc/bft_archive.h (the pick,
emit and heights steps the archiver's kernels run), run over the records and certificate rows of the observer's host
build (tests/audit_lib.py); and the stand-alone sanitizer build of the same file (tests/emu/_san/archive_san)."""
from __future__ import annotations

import ctypes
import os
import subprocess

import numpy as np

import audit_lib as AL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU_DIR = os.path.join(ROOT, "tests", "emu")
LIB = os.path.join(EMU_DIR, "libarchive_host.so")
SAN_EXE = os.path.join(EMU_DIR, "_san", "archive_san")
SRCS = [os.path.join(EMU_DIR, "archive_host.cpp")] + [
    os.path.join(ROOT, "consensus-rs_amd", "csrc", f) for f in ("bft_archive.h", "bft_audit.h", "bft_wire.h", "bft_common.h",
                                                               "bft_wire_block.h", "bft_crypto.h")] + [
    os.path.join(ROOT, "include", "bftwire.h")]
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
    subprocess.check_call(["g++", "-std=c++17", "-Wno-unknown-pragmas", "-DARCHIVE_HOST_MAIN", "-o", tmp, SRCS[0]] + AL.SAN)
    os.replace(tmp, SAN_EXE)
    return SAN_EXE


def lib():
    global _lib
    if _lib is None:
        build()
        _lib = ctypes.CDLL(LIB)
        vp, u64, u32 = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32
        _lib.archive_host_run.restype = u64
        _lib.archive_host_run.argtypes = [vp, vp, u64, ctypes.POINTER(AL.Recs), vp, vp, vp, u64, u32, u32, vp, vp, vp, vp,
                                          vp, u64, vp, vp, vp, vp, vp, vp]
    return _lib


def slot_bytes(n: int) -> int:
    return (288 + 3 + n * 133 + 7) & ~7


def archive(stream, frame_off, inst_frame0, cfg, max_heights: int, key_cap: int = 0) -> dict:
    """The host builds over a frame stream: hdr / hdr_len / slot_bytes / heights (bftsim_export_ledger's layout), the
    arrays of bftsim_archive_out (shaped as bftsim.ledger.Archive shapes them), `report` (a dict of
    bftsim_archive_report), `errors` (rows the emit step refused) and `audit` (tests/audit_lib.observe's dict)."""
    L = lib()
    stream = np.frombuffer(bytes(stream), np.uint8) if not isinstance(stream, np.ndarray) else np.ascontiguousarray(stream)
    off = np.ascontiguousarray(frame_off, np.uint64)
    f0 = np.ascontiguousarray(inst_frame0, np.uint64)
    obs = AL.observe(stream, off, f0, cfg, max_heights, key_cap)
    F, n_inst, H = len(off) - 1, len(f0) - 1, max_heights
    rows, slot = n_inst * H, slot_bytes(cfg.n)
    rec = obs["recs"]
    r = AL.Recs(*[a.ctypes.data for a in rec.values()])
    pad = lambda a: np.ascontiguousarray(np.concatenate([a.reshape(-1), np.zeros(8, a.dtype)]))      # never empty
    status, signer = pad(obs["frame_status"]), pad(obs["frame_signer"])
    cert = [pad(obs[k]) for k in ("cert_round", "cert_digest", "cert_voters", "cert_frame")]
    Rx = max(rows, 1)
    hdr, lens = np.zeros(Rx * slot, np.uint8), np.zeros(Rx, np.uint32)
    out = dict(status=np.zeros(Rx, np.uint8), pp_frame=np.zeros(Rx, np.uint32), n_votes=np.zeros(Rx, np.uint16),
               archived_height=np.zeros(max(n_inst, 1), np.uint64))
    counts = np.zeros(CNT_WORDS, np.uint64)
    errors = L.archive_host_run(stream.ctypes.data, off.ctypes.data, F, ctypes.byref(r), status.ctypes.data, signer.ctypes.data,
                                f0.ctypes.data, n_inst, H, (2 * cfg.n) // 3, *[c.ctypes.data for c in cert], hdr.ctypes.data,
                                slot, lens.ctypes.data, *[a.ctypes.data for a in out.values()], counts.ctypes.data)
    c = [int(x) for x in counts]
    report = dict(headers=c[0], by_status=c[0:3], votes=c[3], foreign_seals=c[4], archived_instances=c[5])
    return dict(hdr=hdr[:rows * slot], hdr_len=lens[:rows], slot_bytes=slot, heights=H, status=out["status"][:rows].reshape(n_inst, H),
                pp_frame=out["pp_frame"][:rows].reshape(n_inst, H), n_votes=out["n_votes"][:rows].reshape(n_inst, H),
                archived_height=out["archived_height"][:n_inst], report=report, errors=int(errors), audit=obs)
