"""ctypes mirror of include/bftsim.h (structs + prototypes)."""
from __future__ import annotations

import ctypes

import numpy as np

from .configs import BftConfig


class CConfig(ctypes.Structure):
    _fields_ = [
        ("n", ctypes.c_uint32), ("heights", ctypes.c_uint32), ("max_ticks", ctypes.c_uint32),
        ("block_period", ctypes.c_uint32), ("genesis_time", ctypes.c_uint64),
        ("seed", ctypes.c_uint64), ("drop_ppm", ctypes.c_uint32), ("byz_count", ctypes.c_uint32),
        ("proposer_crash_ppm", ctypes.c_uint32), ("phase_cap", ctypes.c_uint32),
        ("silent_mask", ctypes.c_uint64 * 4), ("addresses", ctypes.c_void_p),
        ("genesis_proposer", ctypes.c_uint8 * 20), ("genesis_gas_used", ctypes.c_uint64),
        ("seed_byte_order", ctypes.c_uint32), ("header_encoding", ctypes.c_uint32),
        ("backlog_mode", ctypes.c_uint32), ("reserved", ctypes.c_uint32),
    ]


class CResult(ctypes.Structure):
    _fields_ = [(k, ctypes.c_void_p) for k in (
        "committed_height", "flags", "ticks", "views", "round", "proposer", "variant",
        "time_tick", "block_hash")] + [("capacity", ctypes.c_uint64)]


class CStats(ctypes.Structure):
    _fields_ = [("instances", ctypes.c_uint64), ("committed_heights", ctypes.c_uint64),
                ("views", ctypes.c_uint64), ("ticks", ctypes.c_uint64),
                ("flagged", ctypes.c_uint64 * 7), ("round_hist", ctypes.c_uint64 * 65),
                ("latency_hist", ctypes.c_uint64 * 65)]


class CCryptoReport(ctypes.Structure):
    _fields_ = [(k, ctypes.c_uint64) for k in (
        "messages", "seals", "forged", "recovered_as_sender", "mismatches", "seal_errors", "signatures",
        "recoveries", "log_overflows")]


class CAuditReport(ctypes.Structure):
    _fields_ = [(k, ctypes.c_uint64) for k in (
        "frames", "ok", "undecodable", "unrecoverable", "not_validator", "seal_bad", "seal_foreign")] + [
        ("by_code", ctypes.c_uint64 * 4)] + [(k, ctypes.c_uint64) for k in (
            "out_of_range", "certified", "conflicts", "key_overflows", "recoveries")]


class CAuditOut(ctypes.Structure):
    _fields_ = [(k, ctypes.c_void_p) for k in (
        "frame_status", "frame_signer", "inst_flags", "cert_round", "cert_digest", "cert_voters", "cert_frame",
        "cert_flags")]


class CLedgerReport(ctypes.Structure):
    _fields_ = [("headers", ctypes.c_uint64), ("by_status", ctypes.c_uint64 * 10)] + [(k, ctypes.c_uint64) for k in (
        "votes", "recoveries", "duplicate_votes", "verified_instances")]


class CLedgerOut(ctypes.Structure):
    _fields_ = [(k, ctypes.c_void_p) for k in ("status", "block_hash", "voters", "n_votes", "verified_height")]


class CArchiveReport(ctypes.Structure):
    _fields_ = [("headers", ctypes.c_uint64), ("by_status", ctypes.c_uint64 * 3)] + [(k, ctypes.c_uint64) for k in (
        "votes", "foreign_seals", "archived_instances")]


class CArchiveOut(ctypes.Structure):
    _fields_ = [(k, ctypes.c_void_p) for k in ("status", "pp_frame", "n_votes", "archived_height")]


class CAccuseReport(ctypes.Structure):
    _fields_ = [("records", ctypes.c_uint64), ("by_code", ctypes.c_uint64 * 3)] + [(k, ctypes.c_uint64) for k in (
        "accused", "accused_instances", "view_overflows")]


class CAccuseOut(ctypes.Structure):
    _fields_ = [(k, ctypes.c_void_p) for k in ("frame_pair", "inst_accused", "inst_flags", "records")] + [
        ("rec_cap", ctypes.c_uint64)]


# bftsim_accuse_record
ACCUSE_RECORD = np.dtype([("round", "<u8"), ("inst", "<u4"), ("height", "<u4"), ("signer", "<u4"), ("code", "<u4"),
                          ("frame_a", "<u4"), ("frame_b", "<u4")])


def alloc_accuse(frames: int, n_inst: int, rec_cap: int = None):
    """host buffers of bftsim_accuse_out -> (struct, arrays). rec_cap: frames by default (a frame closes one record at
    most, so no second call is ever needed; the pages of an np.empty cost nothing until they are written)"""
    cap = frames if rec_cap is None else rec_cap
    arrs = dict(frame_pair=np.full(frames, 0xffffffff, np.uint32), inst_accused=np.zeros(n_inst * 4, np.uint64),
                inst_flags=np.zeros(n_inst, np.uint32), records=np.empty(cap, ACCUSE_RECORD))
    o = CAccuseOut()
    for k, a in arrs.items():
        setattr(o, k, a.ctypes.data if a.size else None)
    o.rec_cap = cap
    return o, arrs


class CTimelineReport(ctypes.Structure):
    _fields_ = [(k, ctypes.c_uint64) for k in (
        "prepare_frames", "rc_frames", "out_of_range", "prepared", "rc_quorums", "rc_heights", "prepared_first",
        "cert_unprepared", "locked_open", "key_overflows")]


# bftsim_timeline_out: field -> (dtype, words per row, preset); the last two per instance, the others per row
TIMELINE_ROWS = dict(prep_round=(np.uint16, 1, 0xffff), prep_digest=(np.uint8, 32, 0), prep_voters=(np.uint64, 4, 0),
                     prep_frame=(np.uint32, 1, 0), prep_quorums=(np.uint16, 1, 0), rc_quorums=(np.uint16, 1, 0),
                     rc_max_round=(np.uint16, 1, 0xffff), rc_max_frame=(np.uint32, 1, 0), rc_top_round=(np.uint16, 1, 0xffff),
                     rc_frames=(np.uint32, 1, 0), flags=(np.uint8, 1, 0))
TIMELINE_INST = ("inst_flags", "open_height")


class CTimelineOut(ctypes.Structure):
    _fields_ = [(k, ctypes.c_void_p) for k in tuple(TIMELINE_ROWS) + TIMELINE_INST]


def alloc_timeline(n_inst: int, heights: int):
    """host buffers of bftsim_timeline_out -> (struct, arrays)"""
    rows = n_inst * heights
    arrs = {k: np.full(rows * w, fill, dt) for k, (dt, w, fill) in TIMELINE_ROWS.items()}
    arrs.update(inst_flags=np.zeros(n_inst, np.uint32), open_height=np.full(n_inst, heights + 1, np.uint32))
    o = CTimelineOut()
    for k, a in arrs.items():
        setattr(o, k, a.ctypes.data if a.size else None)
    return o, arrs


class CRollCallReport(ctypes.Structure):
    _fields_ = [("frames", ctypes.c_uint64), ("out_of_range", ctypes.c_uint64), ("views", ctypes.c_uint64),
                ("by_outcome", ctypes.c_uint64 * 3)] + [(k, ctypes.c_uint64) for k in (
                    "won", "silent", "silent_instances", "partial_instances")]


# bftsim_rollcall_out: the rows' fields -> words per (instance, validator) row, all uint32; then the instances' fields
ROLLCALL_ROWS = dict(frames=4, last_height=1, last_frame=1, due=1, proposed=1, missed=1, won=1)
ROLLCALL_INST = ("inst_views", "inst_silent", "inst_flags")


class CRollCallOut(ctypes.Structure):
    _fields_ = [(k, ctypes.c_void_p) for k in tuple(ROLLCALL_ROWS) + ROLLCALL_INST + ("records",)] + [
        ("rec_cap", ctypes.c_uint64)]


# bftsim_rollcall_record
ROLLCALL_RECORD = np.dtype([("round", "<u8"), ("inst", "<u4"), ("height", "<u4"), ("proposer", "<u4"), ("outcome", "<u4"),
                            ("start_frame", "<u4"), ("pp_frame", "<u4")])


def alloc_rollcall(n_inst: int, n: int, rec_cap: int):
    """host buffers of bftsim_rollcall_out -> (struct, arrays)"""
    rows = n_inst * n
    arrs = {k: np.zeros(rows * w, np.uint32) for k, w in ROLLCALL_ROWS.items()}
    arrs["last_frame"][:] = 0xffffffff
    arrs.update(inst_views=np.zeros(n_inst, np.uint32), inst_silent=np.zeros(n_inst * 4, np.uint64),
                inst_flags=np.zeros(n_inst, np.uint32), records=np.empty(rec_cap, ROLLCALL_RECORD))
    o = CRollCallOut()
    for k, a in arrs.items():
        setattr(o, k, a.ctypes.data if a.size else None)
    o.rec_cap = rec_cap
    return o, arrs


def alloc_archive(n_inst: int, heights: int, slot_bytes: int):
    """host buffers of bftsim_archive_trace: the header slots, their lengths and bftsim_archive_out -> (hdr, hdr_len,
    struct, arrays)"""
    rows = n_inst * heights
    arrs = dict(status=np.full(rows, 1, np.uint8), pp_frame=np.full(rows, 0xffffffff, np.uint32),
                n_votes=np.zeros(rows, np.uint16), archived_height=np.zeros(n_inst, np.uint64))
    o = CArchiveOut()
    for k, a in arrs.items():
        setattr(o, k, a.ctypes.data)
    return np.zeros(rows * slot_bytes, np.uint8), np.zeros(rows, np.uint32), o, arrs


def alloc_ledger(n_inst: int, heights: int):
    """host buffers of bftsim_ledger_out -> (struct, arrays)"""
    rows = n_inst * heights
    arrs = dict(status=np.zeros(rows, np.uint8), block_hash=np.zeros(rows * 32, np.uint8),
                voters=np.zeros(rows * 4, np.uint64), n_votes=np.zeros(rows, np.uint16),
                verified_height=np.zeros(n_inst, np.uint64))
    o = CLedgerOut()
    for k, a in arrs.items():
        setattr(o, k, a.ctypes.data)
    return o, arrs


def alloc_audit(frames: int, n_inst: int, heights: int):
    """host buffers of bftsim_audit_out (certificate rows preset to "none") -> (struct, arrays)"""
    rows = n_inst * heights
    arrs = dict(
        frame_status=np.zeros(frames, np.uint8), frame_signer=np.full(frames, -1, np.int32),
        inst_flags=np.zeros(n_inst, np.uint32), cert_round=np.full(rows, 0xffff, np.uint16),
        cert_digest=np.zeros(rows * 32, np.uint8), cert_voters=np.zeros(rows * 4, np.uint64),
        cert_frame=np.zeros(rows, np.uint32), cert_flags=np.zeros(rows, np.uint8))
    o = CAuditOut()
    for k, a in arrs.items():
        setattr(o, k, a.ctypes.data)
    return o, arrs


def to_cconfig(cfg: BftConfig):
    """Returns (struct, keepalive) — keep the second object alive while the struct is used."""
    c = CConfig()
    c.n, c.heights, c.max_ticks = cfg.n, cfg.heights, cfg.max_ticks
    c.block_period, c.genesis_time, c.seed = cfg.block_period, cfg.genesis_time, cfg.seed
    c.drop_ppm, c.byz_count = cfg.drop_ppm, cfg.byz_count
    c.proposer_crash_ppm, c.phase_cap = cfg.proposer_crash_ppm, cfg.phase_cap
    for i, m in enumerate(cfg.silent_mask()):
        c.silent_mask[i] = m
    addr = ctypes.create_string_buffer(cfg.address_bytes(), 20 * cfg.n)
    c.addresses = ctypes.cast(addr, ctypes.c_void_p)
    for i, b in enumerate(cfg.genesis_proposer):
        c.genesis_proposer[i] = b
    c.genesis_gas_used = cfg.genesis_gas_used
    c.seed_byte_order = cfg.seed_byte_order
    c.header_encoding = 0
    c.backlog_mode = cfg.backlog_mode
    return c, addr


def alloc_result(n_inst: int, heights: int):
    arrs = dict(
        committed_height=np.zeros(n_inst, np.uint64), flags=np.zeros(n_inst, np.uint32),
        ticks=np.zeros(n_inst, np.uint32), views=np.zeros(n_inst, np.uint64),
        round=np.zeros(n_inst * heights, np.uint16), proposer=np.zeros(n_inst * heights, np.uint16),
        variant=np.zeros(n_inst * heights, np.uint8), time_tick=np.zeros(n_inst * heights, np.uint32),
        block_hash=np.zeros(n_inst * heights * 32, np.uint8))
    r = CResult()
    for k, a in arrs.items():
        setattr(r, k, a.ctypes.data)
    r.capacity = n_inst
    return r, arrs


def shape_result(arrs, n_inst: int, heights: int):
    for k in ("round", "proposer", "variant", "time_tick"):
        arrs[k] = arrs[k].reshape(n_inst, heights)
    arrs["block_hash"] = arrs["block_hash"].reshape(n_inst, heights, 32)
    return arrs
