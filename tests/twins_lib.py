"""ctypes wrapper of tests/emu/libtwins_host.so — TEST-ONLY host build of consensus-rs_amd/csrc/bft_twins.h (the mark
and merge steps the twin kernels run, SPEC.md §11f), checked against tests/twins_ref.py; and the stand-alone sanitizer
build of the same file (tests/emu/_san/twins_san)."""
from __future__ import annotations

import ctypes
import os
import struct
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU_DIR = os.path.join(ROOT, "tests", "emu")
LIB = os.path.join(EMU_DIR, "libtwins_host.so")
SAN_EXE = os.path.join(EMU_DIR, "_san", "twins_san")
SRCS = [os.path.join(EMU_DIR, "twins_host.cpp")] + [
    os.path.join(ROOT, "consensus-rs_amd", "csrc", f) for f in ("bft_twins.h", "bft_common.h")]
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1"]
F_TWIN = 1 << 63
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
    subprocess.check_call(["g++", "-std=c++17", "-Wno-unknown-pragmas", "-DTWINS_HOST_MAIN", "-o", tmp, SRCS[0]] + SAN)
    os.replace(tmp, SAN_EXE)
    return SAN_EXE


def lib():
    global _lib
    if _lib is None:
        build()
        _lib = ctypes.CDLL(LIB)
        _lib.twins_host_index.restype = ctypes.c_uint64
        _lib.twins_host_index.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint64,
                                          ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint64] + \
            [ctypes.c_void_p] * 5
    return _lib


def index(mlog, mlog_n, seed: int, first: int, n_val: int, byz_count: int):
    """-> dict(fmap [frames] u64, if0 [n + 1] u64, kind [messages] u32, byz [n, 4] u64, counts (pp, votes)) of a log
    [n][cap][8] with mlog_n [n] entries each"""
    mlog = np.ascontiguousarray(mlog, np.uint32)
    mlog_n = np.ascontiguousarray(mlog_n, np.uint32)
    n, cap = mlog.shape[0], mlog.shape[1]
    M = int(np.minimum(mlog_n, cap).sum())
    fmap, if0 = np.zeros(2 * M + 1, np.uint64), np.zeros(n + 1, np.uint64)
    kind, byz, counts = np.zeros(M + 1, np.uint32), np.zeros((max(n, 1), 4), np.uint64), np.zeros(2, np.uint64)
    frames = lib().twins_host_index(mlog.ctypes.data, mlog_n.ctypes.data, n, cap, seed, first, n_val, byz_count, 2 * M,
                                    fmap.ctypes.data, if0.ctypes.data, kind.ctypes.data, byz.ctypes.data, counts.ctypes.data)
    assert frames <= 2 * M
    return dict(fmap=fmap[:frames], if0=if0, kind=kind[:M], byz=byz[:n], counts=(int(counts[0]), int(counts[1])))


def san_input(mlog, mlog_n, seed: int, first: int, n_val: int, byz_count: int, fmap, if0) -> bytes:
    """stdin of the stand-alone program: the log and the expected index (tests/emu/twins_host.cpp)"""
    mlog = np.ascontiguousarray(mlog, np.uint32)
    mlog_n = np.ascontiguousarray(mlog_n, np.uint32)
    n, cap = (mlog.shape[0], mlog.shape[1]) if mlog.size else (len(mlog_n), 0)
    fmap, if0 = np.ascontiguousarray(fmap, np.uint64), np.ascontiguousarray(if0, np.uint64)
    assert len(if0) == n + 1
    return struct.pack("<5IQ", n, cap, first, n_val, byz_count, seed) + mlog_n.tobytes() + mlog.tobytes() + \
        struct.pack("<Q", len(fmap)) + fmap.tobytes() + if0.tobytes()
