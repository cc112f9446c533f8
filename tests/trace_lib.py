"""ctypes wrapper of tests/emu/libtrace_host.so — TEST-ONLY host build of consensus-rs_amd/csrc/bft_trace.h (the
frame emitter the trace kernels run), checked against tests/trace_ref.py; and the stand-alone sanitizer build of
the same file (tests/emu/_san/trace_san)."""
from __future__ import annotations

import ctypes
import os
import struct
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU_DIR = os.path.join(ROOT, "tests", "emu")
LIB = os.path.join(EMU_DIR, "libtrace_host.so")
SAN_EXE = os.path.join(EMU_DIR, "_san", "trace_san")
SRCS = [os.path.join(EMU_DIR, "trace_host.cpp")] + [
    os.path.join(ROOT, "consensus-rs_amd", "csrc", f) for f in ("bft_trace.h", "bft_wire.h", "bft_common.h",
                                                               "bft_wire_block.h", "bft_crypto.h")] + [
    os.path.join(ROOT, "include", "bftwire.h")]
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1"]
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
    subprocess.check_call(["g++", "-std=c++17", "-Wno-unknown-pragmas", "-DTRACE_HOST_MAIN", "-o", tmp, SRCS[0]] + SAN)
    os.replace(tmp, SAN_EXE)
    return SAN_EXE


def lib():
    global _lib
    if _lib is None:
        build()
        _lib = ctypes.CDLL(LIB)
        _lib.trace_host_frame.restype = ctypes.c_uint32
        _lib.trace_host_frame.argtypes = [ctypes.c_uint32, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint64,
                                          ctypes.c_char_p, ctypes.c_char_p, ctypes.c_uint32, ctypes.c_char_p,
                                          ctypes.c_char_p, ctypes.c_void_p, ctypes.c_uint32,
                                          ctypes.POINTER(ctypes.c_uint32)]
        _lib.trace_host_create_time.restype = ctypes.c_uint64
        _lib.trace_host_create_time.argtypes = [ctypes.c_uint32, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint32]
    return _lib


def frame(m: dict, cap: int = 4096):
    """-> (emitted bytes (at most cap), emitted length, counted length) of a trace_ref message dict"""
    buf = (ctypes.c_uint8 * max(cap, 1))()
    counted = ctypes.c_uint32()
    hdr = m["header"]
    n = lib().trace_host_frame(m["code"], m["ctime"], m["round"], m["height"], m["digest"], hdr,
                               len(hdr) if hdr else 0, m["sig"], m["seal"], buf, cap, ctypes.byref(counted))
    return bytes(buf[:min(n, cap)]), n, counted.value


def san_input(ms, frames) -> bytes:
    """stdin of the stand-alone program: the messages and their expected frames (tests/emu/trace_host.cpp)"""
    out = [struct.pack("<I", len(ms))]
    for m, f in zip(ms, frames):
        hdr = m["header"] or b""
        out.append(struct.pack("<IQQQ", m["code"], m["ctime"], m["round"], m["height"]) + m["digest"] +
                   struct.pack("<I", len(hdr)) + hdr + m["sig"] + bytes([1 if m["seal"] else 0]) + (m["seal"] or b"") +
                   struct.pack("<I", len(f)) + f)
    return b"".join(out)
