"""ctypes wrapper of tests/emu/libledger_host.so — TEST-ONLY host build of consensus-rs_amd/csrc/bft_ledger.h (the decode,
scatter, tally and link steps the importer's kernels run), with the recoveries taken from the C oracle
(oracle/secp_oracle.c); and the stand-alone sanitizer build of the same file (tests/emu/_san/ledger_san)."""
from __future__ import annotations

import ctypes
import os
import struct
import subprocess

import numpy as np

from audit_lib import oracle_recover

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU_DIR = os.path.join(ROOT, "tests", "emu")
LIB = os.path.join(EMU_DIR, "libledger_host.so")
SAN_EXE = os.path.join(EMU_DIR, "_san", "ledger_san")
SRCS = [os.path.join(EMU_DIR, "ledger_host.cpp")] + [
    os.path.join(ROOT, "consensus-rs_amd", "csrc", f) for f in ("bft_ledger.h", "bft_audit.h", "bft_wire.h", "bft_common.h",
                                                               "bft_wire_block.h", "bft_crypto.h")] + [
    os.path.join(ROOT, "include", "bftwire.h")]
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1"]
CNT_WORDS = 16
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
    subprocess.check_call(["g++", "-std=c++17", "-Wno-unknown-pragmas", "-DLEDGER_HOST_MAIN", "-o", tmp, SRCS[0]] + SAN)
    os.replace(tmp, SAN_EXE)
    return SAN_EXE


def lib():
    global _lib
    if _lib is None:
        build()
        _lib = ctypes.CDLL(LIB)
        vp, u64, u32 = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32
        _lib.ledger_host_rec_size.restype = u64
        _lib.ledger_host_decode.restype = u64
        _lib.ledger_host_decode.argtypes = [vp, u64, vp, u64, vp, vp]
        _lib.ledger_host_scatter.restype = None
        _lib.ledger_host_scatter.argtypes = [vp, u64, vp, u64, vp, vp, vp, vp, vp]
        _lib.ledger_host_finish.restype = None
        _lib.ledger_host_finish.argtypes = [vp, vp, u64, u32, ctypes.c_char_p, u32, u32, u32, ctypes.c_char_p, u64] + [vp] * 8
    return _lib


def verify(hdr, hdr_len, slot_bytes: int, heights: int, cfg, genesis_hash: bytes) -> dict:
    """The host build over a ledger in bftsim_export_ledger's layout: the arrays of bftsim_ledger_out (shaped as
    bftsim.ledger.Verdict shapes them) and `report` (a dict of bftsim_ledger_report)."""
    L = lib()
    hdr = np.ascontiguousarray(hdr, np.uint8).reshape(-1)
    lens = np.ascontiguousarray(hdr_len, np.uint32).reshape(-1)
    H = heights
    n_inst = len(lens) // H
    slots = n_inst * H
    recs = np.zeros(max(slots, 1) * L.ledger_host_rec_size(), np.uint8)
    vbase = np.zeros(slots + 1, np.uint64)
    V = L.ledger_host_decode(hdr.ctypes.data, slot_bytes, lens.ctypes.data, slots, recs.ctypes.data, vbase.ctypes.data)
    Vx = max(V, 1)
    vsig, vdig, vhdr = np.zeros((Vx, 65), np.uint8), np.zeros((Vx, 32), np.uint8), np.zeros(Vx, np.uint32)
    L.ledger_host_scatter(hdr.ctypes.data, slot_bytes, lens.ctypes.data, slots, recs.ctypes.data, vbase.ctypes.data,
                          vsig.ctypes.data, vhdr.ctypes.data, vdig.ctypes.data)
    vaddr, vok = oracle_recover(vdig[:V], vsig[:V])
    vaddr = np.ascontiguousarray(np.concatenate([vaddr, np.zeros((1, 20), np.uint8)]))       # never empty
    vok = np.ascontiguousarray(np.concatenate([np.asarray(vok, np.uint8), np.zeros(1, np.uint8)]))
    out = dict(status=np.zeros(max(slots, 1), np.uint8), block_hash=np.zeros(max(slots, 1) * 32, np.uint8),
               voters=np.zeros(max(slots, 1) * 4, np.uint64), n_votes=np.zeros(max(slots, 1), np.uint16),
               verified_height=np.zeros(max(n_inst, 1), np.uint64))
    counts = np.zeros(CNT_WORDS, np.uint64)
    L.ledger_host_finish(recs.ctypes.data, vbase.ctypes.data, n_inst, H, cfg.address_bytes(), cfg.n, (2 * cfg.n) // 3,
                         cfg.block_period, genesis_hash, cfg.genesis_time, vaddr.ctypes.data, vok.ctypes.data,
                         *[out[k].ctypes.data for k in ("status", "block_hash", "voters", "n_votes", "verified_height")],
                         counts.ctypes.data)
    c = [int(x) for x in counts]
    report = dict(headers=c[10], by_status=c[0:10], votes=int(V), recoveries=int(V), duplicate_votes=c[11],
                  verified_instances=c[12])
    return dict(status=out["status"][:slots].reshape(n_inst, H), block_hash=out["block_hash"][:slots * 32].reshape(n_inst, H, 32),
                voters=out["voters"][:slots * 4].reshape(n_inst, H, 4), n_votes=out["n_votes"][:slots].reshape(n_inst, H),
                verified_height=out["verified_height"][:n_inst], report=report, vote_header=vhdr[:V])


def san_input(headers) -> bytes:
    """stdin of the stand-alone program (tests/emu/ledger_host.cpp)"""
    return struct.pack("<I", len(headers)) + b"".join(struct.pack("<I", len(h)) + h for h in headers)
