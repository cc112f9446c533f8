"""ctypes wrapper of tests/emu/libaudit_host.so — TEST-ONLY host build of consensus-rs_amd/csrc/bft_audit.h (the
per-frame parsing, classification and tally step the observer's kernels run), with the recoveries taken from the C
oracle (oracle/secp_oracle.c); and the stand-alone sanitizer build of the same file (tests/emu/_san/audit_san)."""
from __future__ import annotations

import ctypes
import os
import struct
import subprocess

import numpy as np

import oracle_lib as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU_DIR = os.path.join(ROOT, "tests", "emu")
LIB = os.path.join(EMU_DIR, "libaudit_host.so")
SAN_EXE = os.path.join(EMU_DIR, "_san", "audit_san")
SRCS = [os.path.join(EMU_DIR, "audit_host.cpp")] + [
    os.path.join(ROOT, "consensus-rs_amd", "csrc", f) for f in ("bft_audit.h", "bft_wire.h", "bft_common.h",
                                                               "bft_wire_block.h", "bft_crypto.h")] + [
    os.path.join(ROOT, "include", "bftwire.h")]
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1"]
CNT_WORDS = 16
_lib = None


class Recs(ctypes.Structure):
    _fields_ = [(k, ctypes.c_void_p) for k in ("st", "code", "hx", "round", "digest", "sdig", "sig", "seal_k", "pp_want",
                                               "seal_dig", "seal")]


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
    subprocess.check_call(["g++", "-std=c++17", "-Wno-unknown-pragmas", "-DAUDIT_HOST_MAIN", "-o", tmp, SRCS[0]] + SAN)
    os.replace(tmp, SAN_EXE)
    return SAN_EXE


def lib():
    global _lib
    if _lib is None:
        build()
        _lib = ctypes.CDLL(LIB)
        _lib.audit_host_decode.restype = ctypes.c_uint32
        _lib.audit_host_decode.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_char_p,
                                           ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, ctypes.POINTER(Recs)]
        _lib.audit_host_finish.restype = None
        _lib.audit_host_finish.argtypes = [ctypes.POINTER(Recs), ctypes.c_uint64, ctypes.c_char_p, ctypes.c_uint32] + \
            [ctypes.c_void_p] * 5 + [ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32] + [ctypes.c_void_p] * 9
    return _lib


def oracle_recover(digests: np.ndarray, sigs: np.ndarray):
    """[n, 32], [n, 65] -> ([n, 20] addresses, [n] ok) through the C oracle"""
    if len(digests) == 0:
        return np.zeros((0, 20), np.uint8), np.zeros(0, np.uint8)
    pubs, ok = O.secp_recover_batch(digests, sigs, threads=8)
    addr = np.zeros((len(pubs), 20), np.uint8)
    for i in range(len(pubs)):
        if ok[i]:
            addr[i] = np.frombuffer(O.keccak256(pubs[i].tobytes())[12:], np.uint8)
    return addr, ok


def records(frames, cfg, max_heights: int) -> dict:
    """the decode pass alone over a list of frames: its per-frame records (st, code, hx, round, digest, sdig, sig,
    seal_k, pp_want) and the dense seal list (seal_dig, seal, n_seals)"""
    L = lib()
    stream = np.frombuffer(b"".join(frames) + b"\0", np.uint8)
    off = np.zeros(len(frames) + 1, np.uint64)
    off[1:] = np.cumsum([len(f) for f in frames])
    F = max(len(frames), 1)
    rec = dict(st=np.zeros(F, np.uint8), code=np.zeros(F, np.uint8), hx=np.zeros(F, np.uint32),
               round=np.zeros(F, np.uint64), digest=np.zeros((F, 32), np.uint8), sdig=np.zeros((F, 32), np.uint8),
               sig=np.zeros((F, 65), np.uint8), seal_k=np.zeros(F, np.uint32), pp_want=np.zeros(F, np.uint32),
               seal_dig=np.zeros((F, 32), np.uint8), seal=np.zeros((F, 65), np.uint8))
    r = Recs(*[a.ctypes.data for a in rec.values()])
    rec["n_seals"] = L.audit_host_decode(stream.ctypes.data, off.ctypes.data, len(frames), cfg.address_bytes(), cfg.n,
                                         cfg.seed_byte_order, max_heights, ctypes.byref(r))
    return rec


def observe(stream, frame_off, inst_frame0, cfg, max_heights: int, key_cap: int = 0) -> dict:
    """The host build over a frame stream: the arrays of bftsim_audit_out (shaped as bftsim.trace.Audit shapes them),
    `report` (a dict of bftsim_audit_report) and `recs` (the decode pass's records)."""
    L = lib()
    stream = np.frombuffer(bytes(stream), np.uint8) if not isinstance(stream, np.ndarray) else np.ascontiguousarray(stream)
    off = np.ascontiguousarray(frame_off, np.uint64)
    f0 = np.ascontiguousarray(inst_frame0, np.uint64)
    F, n_inst, H = len(off) - 1, len(f0) - 1, max_heights
    Fx = max(F, 1)
    rec = dict(st=np.zeros(Fx, np.uint8), code=np.zeros(Fx, np.uint8), hx=np.zeros(Fx, np.uint32),
               round=np.zeros(Fx, np.uint64), digest=np.zeros((Fx, 32), np.uint8), sdig=np.zeros((Fx, 32), np.uint8),
               sig=np.zeros((Fx, 65), np.uint8), seal_k=np.zeros(Fx, np.uint32), pp_want=np.zeros(Fx, np.uint32),
               seal_dig=np.zeros((Fx, 32), np.uint8), seal=np.zeros((Fx, 65), np.uint8))
    r = Recs(*[a.ctypes.data for a in rec.values()])
    addresses = cfg.address_bytes()
    n_seals = L.audit_host_decode(stream.ctypes.data, off.ctypes.data, F, addresses, cfg.n, cfg.seed_byte_order, H,
                                  ctypes.byref(r))
    rec_addr, rec_ok = oracle_recover(rec["sdig"][:F], rec["sig"][:F])
    seal_addr, seal_ok = oracle_recover(rec["seal_dig"][:n_seals], rec["seal"][:n_seals])
    pad = lambda a, w: np.ascontiguousarray(np.concatenate([a, np.zeros((1,) + a.shape[1:], a.dtype)]))   # never empty
    rec_addr, rec_ok, seal_addr, seal_ok = pad(rec_addr, 20), pad(rec_ok, 1), pad(seal_addr, 20), pad(seal_ok, 1)
    rows = n_inst * H
    out = dict(frame_status=np.zeros(Fx, np.uint8), frame_signer=np.full(Fx, -1, np.int32),
               inst_flags=np.zeros(max(n_inst, 1), np.uint32), cert_round=np.full(rows, 0xffff, np.uint16),
               cert_digest=np.zeros(rows * 32, np.uint8), cert_voters=np.zeros(rows * 4, np.uint64),
               cert_frame=np.zeros(rows, np.uint32), cert_flags=np.zeros(rows, np.uint8))
    counts = np.zeros(CNT_WORDS, np.uint64)
    L.audit_host_finish(ctypes.byref(r), F, addresses, cfg.n, rec_addr.ctypes.data, rec_ok.ctypes.data,
                        seal_addr.ctypes.data, seal_ok.ctypes.data, f0.ctypes.data, n_inst, H, key_cap, (2 * cfg.n) // 3,
                        *[out[k].ctypes.data for k in ("frame_status", "frame_signer", "inst_flags", "cert_round",
                                                       "cert_digest", "cert_voters", "cert_frame", "cert_flags")],
                        counts.ctypes.data)
    c = [int(x) for x in counts]
    report = dict(frames=F, ok=c[0], undecodable=c[1], unrecoverable=c[2], not_validator=c[3], seal_bad=c[4],
                  seal_foreign=c[5], by_code=c[6:10], out_of_range=c[10], certified=c[11], conflicts=c[12],
                  key_overflows=c[13], recoveries=F + n_seals)
    return dict(frame_status=out["frame_status"][:F], frame_signer=out["frame_signer"][:F],
                inst_flags=out["inst_flags"][:n_inst], cert_round=out["cert_round"].reshape(n_inst, H),
                cert_digest=out["cert_digest"].reshape(n_inst, H, 32), cert_voters=out["cert_voters"].reshape(n_inst, H, 4),
                cert_frame=out["cert_frame"].reshape(n_inst, H), cert_flags=out["cert_flags"].reshape(n_inst, H),
                report=report, recs=rec)


def san_input(addresses: bytes, n: int, frames, catalogue=None) -> bytes:
    """stdin of the stand-alone program (tests/emu/audit_host.cpp); catalogue: [(frame, decodable)] or None"""
    out = struct.pack("<I", n) + addresses + struct.pack("<I", len(frames)) + \
        b"".join(struct.pack("<I", len(f)) + f for f in frames)
    if catalogue is not None:
        out += struct.pack("<I", len(catalogue)) + b"".join(bytes([int(bool(ok))]) + struct.pack("<I", len(f)) + f
                                                            for f, ok in catalogue)
    return out
