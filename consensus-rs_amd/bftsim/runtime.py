"""Host binding of libbftsim (the HIP path). Mirrors the reference's engine surface:
`Simulator` stands for one `create_bft_engine` per instance (src/consensus/consensus.rs:42-60),
batched. There is no CPU fallback: if the HIP library is missing this raises."""
from __future__ import annotations

import ctypes
import os

import numpy as np

from . import _abi
from .configs import BftConfig

PKG_DIR = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def lib_override(var: str):
    """A/B builds (scripts/gpu_ab*.sh) may point a binding at another library, but only when
    BFTSIM_TESTING=1 is set too: a stray BFTSIM_LIB-style variable never swaps the product library silently."""
    v = os.environ.get(var)
    if not v:
        return None
    if os.environ.get("BFTSIM_TESTING") != "1":
        raise RuntimeError(f"{var}={v} is set but BFTSIM_TESTING=1 is not: refusing to load a non-product library")
    import sys
    print(f"bftsim: {var} override -> {v} (BFTSIM_TESTING)", file=sys.stderr)
    return v


LIB_PATH = lib_override("BFTSIM_LIB") or os.path.join(PKG_DIR, "build", "libbftsim.so")

_lib = None
HEADER_SLOT = 288                       # BFTSIM_HEADER_SLOT (include/bftsim.h)


class BftsimError(RuntimeError):
    pass


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise BftsimError(f"libbftsim.so not built ({LIB_PATH}); run __graft_entry__.build()")
        L = ctypes.CDLL(LIB_PATH)
        L.bftsim_create.argtypes = [ctypes.POINTER(_abi.CConfig), ctypes.c_int, ctypes.POINTER(ctypes.c_void_p)]
        L.bftsim_destroy.argtypes = [ctypes.c_void_p]
        L.bftsim_last_error.argtypes = [ctypes.c_void_p]
        L.bftsim_last_error.restype = ctypes.c_char_p
        L.bftsim_run.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint64, ctypes.POINTER(_abi.CResult)]
        L.bftsim_prepare.argtypes = [ctypes.c_void_p, ctypes.c_uint64]
        L.bftsim_launch.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p]
        L.bftsim_sync.argtypes = [ctypes.c_void_p]
        L.bftsim_fetch.argtypes = [ctypes.c_void_p, ctypes.POINTER(_abi.CResult)]
        L.bftsim_stats_get.argtypes = [ctypes.c_void_p, ctypes.POINTER(_abi.CStats)]
        L.bftsim_stats_allreduce.argtypes = [ctypes.c_void_p, ctypes.POINTER(_abi.CStats)]
        L.bftsim_comm_unique_id.argtypes = [ctypes.c_void_p]
        L.bftsim_set_crypto.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_uint32]
        L.bftsim_ledger_slot_bytes.argtypes = [ctypes.c_uint32]
        L.bftsim_ledger_slot_bytes.restype = ctypes.c_uint64
        L.bftsim_export_ledger.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint64,
                                           ctypes.c_void_p]
        L.bftsim_crypto_verify.argtypes = [ctypes.c_void_p, ctypes.POINTER(_abi.CCryptoReport), ctypes.c_uint64,
                                           ctypes.c_void_p, ctypes.c_void_p]
        L.bftsim_set_trace_keep.argtypes = [ctypes.c_void_p, ctypes.c_int]
        L.bftsim_trace_sizes.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p]
        L.bftsim_export_trace.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_void_p,
                                          ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p,
                                          ctypes.c_void_p]
        L.bftsim_trace_last_ms.argtypes = [ctypes.c_void_p] + [ctypes.POINTER(ctypes.c_float)] * 3
        L.bftsim_set_trace_twins.argtypes = [ctypes.c_void_p, ctypes.c_int]
        L.bftsim_trace_twin_counts.argtypes = [ctypes.c_void_p] + [ctypes.POINTER(ctypes.c_uint64)] * 2
        L.bftsim_trace_twins_last_ms.argtypes = [ctypes.c_void_p] + [ctypes.POINTER(ctypes.c_float)] * 3
        L.bftsim_audit_trace.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p,
                                         ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32,
                                         ctypes.c_uint32, ctypes.POINTER(_abi.CAuditOut),
                                         ctypes.POINTER(_abi.CAuditReport)]
        L.bftsim_audit_last_trace.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint32,
                                              ctypes.POINTER(_abi.CAuditOut), ctypes.POINTER(_abi.CAuditReport)]
        L.bftsim_audit_last_ms.argtypes = [ctypes.c_void_p] + [ctypes.POINTER(ctypes.c_float)] * 4
        tail = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.POINTER(_abi.CArchiveOut),
                ctypes.POINTER(_abi.CAuditOut), ctypes.POINTER(_abi.CAuditReport), ctypes.POINTER(_abi.CArchiveReport)]
        L.bftsim_archive_trace.argtypes = L.bftsim_audit_trace.argtypes[:9] + tail
        L.bftsim_archive_last_trace.argtypes = L.bftsim_audit_last_trace.argtypes[:4] + tail
        L.bftsim_archive_last_ms.argtypes = [ctypes.c_void_p] + [ctypes.POINTER(ctypes.c_float)] * 4
        if not os.environ.get("BFTSIM_LIB") or hasattr(L, "bftsim_accuse_trace"):
            # (an A/B build of an earlier commit may lack them, scripts/accuse_bench.py --parent-lib; the product must not)
            tail = [ctypes.c_uint32, ctypes.POINTER(_abi.CAccuseOut), ctypes.POINTER(_abi.CAuditOut),
                    ctypes.POINTER(_abi.CAuditReport), ctypes.POINTER(_abi.CAccuseReport)]
            L.bftsim_accuse_trace.argtypes = L.bftsim_audit_trace.argtypes[:9] + tail
            L.bftsim_accuse_last_trace.argtypes = L.bftsim_audit_last_trace.argtypes[:4] + tail
            L.bftsim_accuse_last_ms.argtypes = [ctypes.c_void_p] + [ctypes.POINTER(ctypes.c_float)] * 4
        if not os.environ.get("BFTSIM_LIB") or hasattr(L, "bftsim_timeline_trace"):
            # (an A/B build of an earlier commit may lack them, scripts/timeline_bench.py --parent-lib; the product must not)
            tail = [ctypes.c_uint32, ctypes.POINTER(_abi.CTimelineOut), ctypes.POINTER(_abi.CAuditOut),
                    ctypes.POINTER(_abi.CAuditReport), ctypes.POINTER(_abi.CTimelineReport)]
            L.bftsim_timeline_trace.argtypes = L.bftsim_audit_trace.argtypes[:9] + tail
            L.bftsim_timeline_last_trace.argtypes = L.bftsim_audit_last_trace.argtypes[:4] + tail
            L.bftsim_timeline_last_ms.argtypes = [ctypes.c_void_p] + [ctypes.POINTER(ctypes.c_float)] * 4
        if not os.environ.get("BFTSIM_LIB") or hasattr(L, "bftsim_rollcall_trace"):
            # (an A/B build of an earlier commit may lack them, scripts/rollcall_bench.py --parent-lib; the product must not)
            tail = [ctypes.c_uint32, ctypes.POINTER(_abi.CRollCallOut), ctypes.POINTER(_abi.CRollCallReport),
                    ctypes.POINTER(_abi.CAuditOut), ctypes.POINTER(_abi.CAuditReport),
                    ctypes.POINTER(_abi.CTimelineOut), ctypes.POINTER(_abi.CTimelineReport)]
            L.bftsim_rollcall_trace.argtypes = L.bftsim_audit_trace.argtypes[:9] + tail
            L.bftsim_rollcall_last_trace.argtypes = L.bftsim_audit_last_trace.argtypes[:4] + tail
            L.bftsim_rollcall_last_ms.argtypes = [ctypes.c_void_p] + [ctypes.POINTER(ctypes.c_float)] * 6
        L.bftsim_set_ledger_votes.argtypes = [ctypes.c_void_p, ctypes.c_uint32]
        L.bftsim_verify_ledger.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p,
                                           ctypes.c_uint64, ctypes.c_uint32, ctypes.POINTER(_abi.CLedgerOut),
                                           ctypes.POINTER(_abi.CLedgerReport)]
        L.bftsim_ledger_last_ms.argtypes = [ctypes.c_void_p] + [ctypes.POINTER(ctypes.c_float)] * 4
        L.bftsim_launched_count.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint64),
                                            ctypes.POINTER(ctypes.c_uint64)]
        L.bftsim_comm_init.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_char_p]
        L.bftsim_last_kernel_ms.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_float),
                                            ctypes.POINTER(ctypes.c_float)]
        L.bftsim_kernel_ms_sum.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_double),
                                           ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_uint32)]
        L.bftsim_set_pipeline.argtypes = [ctypes.c_void_p, ctypes.c_int]
        L.bftsim_set_hash_batch.argtypes = [ctypes.c_void_p, ctypes.c_uint32]
        L.bftsim_set_fast.argtypes = [ctypes.c_void_p, ctypes.c_int]
        L.bftsim_set_trace.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32]
        L.bftsim_set_window.argtypes = [ctypes.c_void_p, ctypes.c_uint32]
        if hasattr(L, "bftsim_set_rcs_capacity"):     # (absent from A/B builds of earlier rounds)
            L.bftsim_set_rcs_capacity.argtypes = [ctypes.c_void_p, ctypes.c_uint32]
        L.bftsim_fetch_summary.argtypes = [ctypes.c_void_p, ctypes.c_uint64] + [ctypes.c_void_p] * 5
        L.bftsim_two_thirds_majority.restype = ctypes.c_uint32
        L.bftsim_seed_from_hash.restype = ctypes.c_uint32
        L.bftsim_seed_from_hash.argtypes = [ctypes.c_char_p, ctypes.c_uint32]
        L.bftsim_seed_from_hash_order.restype = ctypes.c_uint32
        L.bftsim_seed_from_hash_order.argtypes = [ctypes.c_char_p, ctypes.c_uint32, ctypes.c_uint32]
        L.bftsim_two_thirds_majority.argtypes = [ctypes.c_uint32]
        L.bftsim_calc_proposer.restype = ctypes.c_uint32
        L.bftsim_calc_proposer.argtypes = [ctypes.c_char_p, ctypes.c_uint32, ctypes.c_uint64]
        L.bftsim_keccak256.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_void_p]
        L.bftsim_genesis_hash.argtypes = [ctypes.POINTER(_abi.CConfig), ctypes.c_void_p]
        L.bftsim_view_cmp.argtypes = [ctypes.c_uint64] * 4
        L.bftsim_export_headers.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p]
        _lib = L
    return _lib


def keccak256(data: bytes) -> bytes:
    """Keccak-256 (`hash`, cryptocurrency-kit) through libbftsim (host code, no GPU needed)."""
    out = ctypes.create_string_buffer(32)
    lib().bftsim_keccak256(data, len(data), out)
    return out.raw


def _check(h, rc, what):
    if rc != 0:
        msg = lib().bftsim_last_error(h).decode() if h else ""
        raise BftsimError(f"{what} failed ({rc}): {msg}")


class Simulator:
    """Runs many independent seeded consensus-rs clusters of one configuration on one GPU."""

    def __init__(self, cfg: BftConfig, device: int = 0):
        self.cfg = cfg
        self._c, self._keep = _abi.to_cconfig(cfg)
        h = ctypes.c_void_p()
        rc = lib().bftsim_create(ctypes.byref(self._c), device, ctypes.byref(h))
        self.h = h.value
        _check(self.h, rc, "bftsim_create")
        self.n_prepared = 0
        self.n_launched = 0             # instances of the last launch: what fetch / crypto_verify read

    def close(self):
        if self.h:
            lib().bftsim_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def run(self, first: int, n: int, trace_ticks: int = 0):
        r, arrs = _abi.alloc_result(n, self.cfg.heights)
        tr = None
        if trace_ticks:
            tr = np.zeros(n * trace_ticks * self.cfg.n, np.uint64)
            _check(self.h, lib().bftsim_set_trace(self.h, tr.ctypes.data, trace_ticks), "set_trace")
        try:
            _check(self.h, lib().bftsim_run(self.h, first, n, ctypes.byref(r)), "bftsim_run")
            self.n_prepared = self.n_launched = n
        finally:
            if trace_ticks:
                lib().bftsim_set_trace(self.h, None, 0)
        arrs = _abi.shape_result(arrs, n, self.cfg.heights)
        if tr is not None:
            arrs["trace"] = tr.reshape(n, trace_ticks, self.cfg.n)
        st = self.stats()
        arrs["round_hist"] = np.array(st["round_hist"], np.uint64)
        arrs["latency_hist"] = np.array(st["latency_hist"], np.uint64)
        return arrs

    def set_window(self, window: int):
        """Keep a ring of `window` canonical rows per instance (0: every height); see bftsim.h."""
        _check(self.h, lib().bftsim_set_window(self.h, window), "bftsim_set_window")

    def set_rcs_capacity(self, rounds: int):
        """RoundChangeSet rounds kept per validator (bftsim_set_rcs_capacity); run() re-runs an
        overflowing batch at twice the capacity."""
        _check(self.h, lib().bftsim_set_rcs_capacity(self.h, rounds), "bftsim_set_rcs_capacity")

    def launched(self):
        """(first, n) of the last launch: the rows the fetch family writes (bftsim_launched_count)."""
        a, b = ctypes.c_uint64(), ctypes.c_uint64()
        _check(self.h, lib().bftsim_launched_count(self.h, ctypes.byref(a), ctypes.byref(b)), "bftsim_launched_count")
        return a.value, b.value

    def fetch_summary(self, n: int = None, tips: bool = True):
        """Per-instance outputs of the last launch into buffers of `n` instances (default: the launched
        count; a smaller n is refused by the library, bftsim.h)."""
        if n is None:
            n = self.launched()[1]
        out = dict(committed_height=np.zeros(n, np.uint64), flags=np.zeros(n, np.uint32),
                   ticks=np.zeros(n, np.uint32), views=np.zeros(n, np.uint64))
        if tips:
            out["tip_hash"] = np.zeros((n, 32), np.uint8)
        _check(self.h, lib().bftsim_fetch_summary(
            self.h, n, out["committed_height"].ctypes.data, out["flags"].ctypes.data, out["ticks"].ctypes.data,
            out["views"].ctypes.data, out["tip_hash"].ctypes.data if tips else None), "bftsim_fetch_summary")
        return out

    def run_stream(self, first: int, n: int, window: int = 256):
        """Windowed run (long horizons): per-instance outputs, tip hashes and histograms."""
        self.set_window(window)
        self.prepare(n)
        self.launch(first)
        out = self.fetch_summary(n)
        st = self.stats()
        out["round_hist"] = np.array(st["round_hist"], np.uint64)
        out["latency_hist"] = np.array(st["latency_hist"], np.uint64)
        return out

    # device-resident path (bench)
    def prepare(self, n: int):
        _check(self.h, lib().bftsim_prepare(self.h, n), "bftsim_prepare")
        self.n_prepared = n

    def launch(self, first: int, stream: int = 0):
        _check(self.h, lib().bftsim_launch(self.h, first, ctypes.c_void_p(stream)), "bftsim_launch")
        self.n_launched = self.n_prepared

    def fetch(self):
        """Per-height results of the last launch (all its instances), as run() returns them. Sized by the
        launch, not by a later prepare: the C side writes the launched count."""
        n = self.n_launched
        r, arrs = _abi.alloc_result(n, self.cfg.heights)
        _check(self.h, lib().bftsim_fetch(self.h, ctypes.byref(r)), "bftsim_fetch")
        return _abi.shape_result(arrs, n, self.cfg.heights)

    def export_headers(self, n: int = None):
        """Ledger export of the last run / launch (core/ledger.rs:193-245): ([n, H] list of the Header
        bytes of every committed height, empty beyond it). Keccak-256 of each is its block hash."""
        if n is None:
            n = self.launched()[1]
        H = self.cfg.heights
        slot = HEADER_SLOT
        buf = np.zeros(n * H * slot, np.uint8)
        lens = np.zeros(n * H, np.uint32)
        _check(self.h, lib().bftsim_export_headers(self.h, n, buf.ctypes.data, lens.ctypes.data),
               "bftsim_export_headers")
        buf = buf.reshape(n, H, slot)
        lens = lens.reshape(n, H)
        return [[bytes(buf[i, x, :lens[i, x]]) for x in range(H)] for i in range(n)]

    def sync(self):
        _check(self.h, lib().bftsim_sync(self.h), "bftsim_sync")

    def kernel_ms(self):
        a, b = ctypes.c_float(), ctypes.c_float()
        _check(self.h, lib().bftsim_last_kernel_ms(self.h, ctypes.byref(a), ctypes.byref(b)), "kernel_ms")
        return a.value, b.value

    def kernel_ms_sum(self):
        """(consensus ms, hash ms, launches) summed over the launches since the previous call."""
        a, b, n = ctypes.c_double(), ctypes.c_double(), ctypes.c_uint32()
        _check(self.h, lib().bftsim_kernel_ms_sum(self.h, ctypes.byref(a), ctypes.byref(b), ctypes.byref(n)),
               "kernel_ms_sum")
        return a.value, b.value, n.value

    def set_fast(self, on: bool):
        """Verification switch: False runs N = 64 through the full kernel alone (identical results)."""
        _check(self.h, lib().bftsim_set_fast(self.h, 1 if on else 0), "bftsim_set_fast")

    def set_pipeline(self, on, depth: int = 2):
        """Batch throughput mode: a ring of `depth` row-table sets; the hash pass of each launch overlaps
        the following launches (include/bftsim.h bftsim_set_pipeline)."""
        _check(self.h, lib().bftsim_set_pipeline(self.h, depth if on else 0), "bftsim_set_pipeline")

    def set_hash_batch(self, launches: int):
        """Pipelined launches: the chains of this many consecutive launches as one kernel (include/bftsim.h)."""
        _check(self.h, lib().bftsim_set_hash_batch(self.h, launches), "bftsim_set_hash_batch")

    @staticmethod
    def _stats_dict(s):
        return dict(instances=s.instances, committed_heights=s.committed_heights, views=s.views,
                    ticks=s.ticks, flagged=list(s.flagged), round_hist=list(s.round_hist),
                    latency_hist=list(s.latency_hist))

    def stats(self):
        s = _abi.CStats()
        _check(self.h, lib().bftsim_stats_get(self.h, ctypes.byref(s)), "bftsim_stats_get")
        return self._stats_dict(s)

    def set_crypto(self, secrets, forged=(), log_cap: int = 0):
        """Real-crypto mode (include/bftsim.h bftsim_set_crypto, SPEC.md §11): `secrets` = one 32-byte
        key per validator in the sorted validator order (None turns the mode off); `forged` = indices
        that sign with a key that is not theirs. Applies at the next prepare."""
        if secrets is None:
            _check(self.h, lib().bftsim_set_crypto(self.h, None, None, 0), "bftsim_set_crypto")
            return
        assert len(secrets) == self.cfg.n and all(len(k) == 32 for k in secrets)
        fb = bytes(1 if v in set(forged) else 0 for v in range(self.cfg.n))
        _check(self.h, lib().bftsim_set_crypto(self.h, b"".join(secrets), fb, log_cap), "bftsim_set_crypto")

    def crypto_verify(self):
        """The batched sign / recover pass over the last launch's messages: report dict, per-instance
        checksum [n, 32] (XOR of keccak(signature || seal)) and message counts [n]."""
        n = self.n_launched
        rep = _abi.CCryptoReport()
        ck = np.zeros((n, 32), np.uint8)
        cnt = np.zeros(n, np.uint32)
        _check(self.h, lib().bftsim_crypto_verify(self.h, ctypes.byref(rep), n, ck.ctypes.data, cnt.ctypes.data),
               "bftsim_crypto_verify")
        out = {k: getattr(rep, k) for k, _ in _abi.CCryptoReport._fields_}
        out["checksum"], out["inst_messages"] = ck, cnt
        return out

    def export_ledger(self):
        """The ledger Headers with votes of the last launch (after crypto_verify): per instance a list of
        header byte strings, height 1..committed (include/bftsim.h bftsim_export_ledger)."""
        n, H = self.n_launched, self.cfg.heights
        slot = lib().bftsim_ledger_slot_bytes(self.cfg.n)
        buf = np.zeros(n * H * slot, np.uint8)
        lens = np.zeros(n * H, np.uint32)
        _check(self.h, lib().bftsim_export_ledger(self.h, n, buf.ctypes.data, slot, lens.ctypes.data),
               "bftsim_export_ledger")
        out = []
        for i in range(n):
            row = []
            for x in range(H):
                k = int(lens[i * H + x])
                if k == 0:
                    break
                o = (i * H + x) * slot
                row.append(bytes(buf[o:o + k]))
            out.append(row)
        return out

    def set_trace_keep(self, on: bool):
        """crypto_verify keeps on the device what export_trace needs, until the next launch (bftsim_set_trace_keep)."""
        _check(self.h, lib().bftsim_set_trace_keep(self.h, 1 if on else 0), "bftsim_set_trace_keep")

    def set_trace_twins(self, on):
        """The next keeping crypto_verify adds every equivocating broadcast's second frame to the trace
        (bftsim_set_trace_twins, SPEC.md §11f); on: a bool, or 0 / 1 (anything else is refused)."""
        _check(self.h, lib().bftsim_set_trace_twins(self.h, int(on)), "bftsim_set_trace_twins")

    def trace_twin_counts(self):
        """(PrePrepare twins, vote twins) of the last kept trace (bftsim_trace_twin_counts)."""
        a, b = ctypes.c_uint64(), ctypes.c_uint64()
        _check(self.h, lib().bftsim_trace_twin_counts(self.h, ctypes.byref(a), ctypes.byref(b)), "bftsim_trace_twin_counts")
        return a.value, b.value

    def trace_twins_ms(self):
        """(mark + scan + merge, digests, signing) of the last verify's twin passes, device ms."""
        return self._last_ms("bftsim_trace_twins_last_ms", 3)

    def trace_sizes(self):
        """(frames [n] u32, stream bytes [n] u64) per instance of the last launch's trace (after crypto_verify)."""
        n = self.n_launched
        fr, by = np.zeros(n, np.uint32), np.zeros(n, np.uint64)
        _check(self.h, lib().bftsim_trace_sizes(self.h, n, fr.ctypes.data, by.ctypes.data), "bftsim_trace_sizes")
        return fr, by

    def export_trace(self, begin: int = 0, count: int = None):
        """The signed wire frames of instances [begin, begin + count) of the last launch (default: to its end), as
        a bftsim.trace.Trace (include/bftsim.h bftsim_export_trace, SPEC.md §11b)."""
        from .trace import Trace
        if count is None:
            count = self.n_launched - begin
        fr, by = self.trace_sizes()
        if begin < 0 or count < 0 or begin + count > len(fr):
            raise BftsimError(f"export_trace: instances [{begin}, {begin + count}) outside the last launch of {len(fr)}")
        frames, nbytes = int(fr[begin:begin + count].sum()), int(by[begin:begin + count].sum())
        stream = np.zeros(nbytes, np.uint8)
        off = np.zeros(frames + 1, np.uint64)
        meta = np.zeros((frames, 4), np.uint32)
        f0 = np.zeros(count + 1, np.uint64)
        _check(self.h, lib().bftsim_export_trace(self.h, begin, count, stream.ctypes.data, nbytes, off.ctypes.data,
                                                 frames, meta.ctypes.data, f0.ctypes.data), "bftsim_export_trace")
        return Trace(stream, off, meta, f0, begin)

    def _host_trace(self, trace, max_heights):
        """what the *_trace methods pass on of a bftsim.trace.Trace, or anything with its stream / frame_off /
        inst_frame0 -> (stream, frame_off, inst_frame0, frames, instances, max_heights, the heights buffers are sized
        by: 0 where the library refuses max_heights)"""
        H = self.cfg.heights if max_heights is None else max_heights
        stream = np.ascontiguousarray(trace.stream, np.uint8)
        off = np.ascontiguousarray(trace.frame_off, np.uint64)
        f0 = np.ascontiguousarray(trace.inst_frame0, np.uint64)
        return stream, off, f0, len(off) - 1, len(f0) - 1, H, H if 0 < H <= 65535 else 0

    def _kept_range(self, what, begin, count):
        """instances [begin, begin + count) of the kept trace (count None: to the launch's end) -> (count, frames)"""
        if count is None:
            count = self.n_launched - begin
        fr, _ = self.trace_sizes()
        if begin < 0 or count < 0 or begin + count > len(fr):
            raise BftsimError(f"{what}: instances [{begin}, {begin + count}) outside the last launch of {len(fr)}")
        return count, int(fr[begin:begin + count].sum())

    def _last_ms(self, getter, k):
        """the k phase times, device ms, that a *_last_ms entry point stores"""
        v = [ctypes.c_float() for _ in range(k)]
        _check(self.h, getattr(lib(), getter)(self.h, *[ctypes.byref(x) for x in v]), getter)
        return tuple(x.value for x in v)

    def trace_ms(self):
        """(size pass + scan, emit kernel, device-to-host copies) of the last trace calls, device ms."""
        return self._last_ms("bftsim_trace_last_ms", 3)

    def audit_trace(self, trace, max_heights: int = None, key_cap: int = 0):
        """The observer (include/bftsim.h bftsim_audit_trace, SPEC.md §11c) over a bftsim.trace.Trace, or anything
        with its stream / frame_off / inst_frame0: per-frame statuses and signers, per-height commit certificates and
        the safety verdict, all computed on the device from the bytes. -> bftsim.trace.Audit"""
        from .trace import Audit
        stream, off, f0, frames, n, H, Hb = self._host_trace(trace, max_heights)
        o, arrs = _abi.alloc_audit(frames, n, Hb)
        rep = _abi.CAuditReport()
        _check(self.h, lib().bftsim_audit_trace(self.h, stream.ctypes.data, len(stream), off.ctypes.data, frames,
                                                f0.ctypes.data, n, H, key_cap, ctypes.byref(o), ctypes.byref(rep)),
               "bftsim_audit_trace")
        return Audit(arrs, rep, n, H)

    def audit_last_trace(self, begin: int = 0, count: int = None, key_cap: int = 0):
        """The same over the kept trace of the last launch (after crypto_verify with set_trace_keep), instances
        [begin, begin + count): emitted and audited on the device (bftsim_audit_last_trace)."""
        from .trace import Audit
        count, frames = self._kept_range("audit_last_trace", begin, count)
        o, arrs = _abi.alloc_audit(frames, count, self.cfg.heights)
        rep = _abi.CAuditReport()
        _check(self.h, lib().bftsim_audit_last_trace(self.h, begin, count, key_cap, ctypes.byref(o), ctypes.byref(rep)),
               "bftsim_audit_last_trace")
        return Audit(arrs, rep, count, self.cfg.heights)

    def audit_ms(self):
        """(decode, recoveries, classify + tally, copies) of the last audit, device ms (bftsim_audit_last_ms)."""
        return self._last_ms("bftsim_audit_last_ms", 4)

    def archive_trace(self, trace, max_heights: int = None, key_cap: int = 0):
        """The archiver (include/bftsim.h bftsim_archive_trace, SPEC.md §11e) over a bftsim.trace.Trace, or anything with
        its stream / frame_off / inst_frame0: the ledger of the heights the observer certifies, each header assembled on
        the device from the PrePrepare frame's block and the voters' commit seals. -> (ledger, bftsim.ledger.Archive);
        ledger is the (hdr, hdr_len, slot_bytes, heights) that verify_ledger takes."""
        from .ledger import Archive
        from .trace import Audit
        stream, off, f0, frames, n, H, Hb = self._host_trace(trace, max_heights)
        slot = lib().bftsim_ledger_slot_bytes(self.cfg.n)
        hdr, lens, o, arrs = _abi.alloc_archive(n, Hb, slot)
        ao, aarrs = _abi.alloc_audit(frames, n, Hb)
        rep, arep = _abi.CArchiveReport(), _abi.CAuditReport()
        _check(self.h, lib().bftsim_archive_trace(self.h, stream.ctypes.data, len(stream), off.ctypes.data, frames,
                                                  f0.ctypes.data, n, H, key_cap, hdr.ctypes.data, slot, lens.ctypes.data,
                                                  ctypes.byref(o), ctypes.byref(ao), ctypes.byref(arep), ctypes.byref(rep)),
               "bftsim_archive_trace")
        return (hdr, lens, slot, H), Archive(arrs, rep, n, H, Audit(aarrs, arep, n, H))

    def archive_last_trace(self, begin: int = 0, count: int = None, key_cap: int = 0):
        """The same over the kept trace of the last launch (after crypto_verify with set_trace_keep), instances
        [begin, begin + count): emitted, audited and archived on the device (bftsim_archive_last_trace)."""
        from .ledger import Archive
        from .trace import Audit
        count, frames = self._kept_range("archive_last_trace", begin, count)
        H = self.cfg.heights
        slot = lib().bftsim_ledger_slot_bytes(self.cfg.n)
        hdr, lens, o, arrs = _abi.alloc_archive(count, H, slot)
        ao, aarrs = _abi.alloc_audit(frames, count, H)
        rep, arep = _abi.CArchiveReport(), _abi.CAuditReport()
        _check(self.h, lib().bftsim_archive_last_trace(self.h, begin, count, key_cap, hdr.ctypes.data, slot, lens.ctypes.data,
                                                       ctypes.byref(o), ctypes.byref(ao), ctypes.byref(arep), ctypes.byref(rep)),
               "bftsim_archive_last_trace")
        return (hdr, lens, slot, H), Archive(arrs, rep, count, H, Audit(aarrs, arep, count, H))

    def archive_ms(self):
        """(the observer's passes, pick, emit + heights, copies) of the last archive call, device ms
        (bftsim_archive_last_ms)."""
        return self._last_ms("bftsim_archive_last_ms", 4)

    def accuse_trace(self, trace, max_heights: int = None, key_cap: int = 0, view_cap: int = 0, rec_cap: int = None):
        """The accuser (include/bftsim.h bftsim_accuse_trace, SPEC.md §11g) over a bftsim.trace.Trace, or anything with
        its stream / frame_off / inst_frame0: every validator that signed two digests for one (code, height, round)
        among the frames the observer accepts, each with the two frames that prove it, found on the device.
        -> bftsim.trace.Accusation (its .audit: the observer's outputs of the same call)"""
        from .trace import Accusation, Audit
        stream, off, f0, frames, n, H, Hb = self._host_trace(trace, max_heights)
        o, arrs = _abi.alloc_accuse(frames, n, rec_cap)
        ao, aarrs = _abi.alloc_audit(frames, n, Hb)
        rep, arep = _abi.CAccuseReport(), _abi.CAuditReport()
        _check(self.h, lib().bftsim_accuse_trace(self.h, stream.ctypes.data, len(stream), off.ctypes.data, frames,
                                                 f0.ctypes.data, n, H, key_cap, view_cap, ctypes.byref(o), ctypes.byref(ao),
                                                 ctypes.byref(arep), ctypes.byref(rep)), "bftsim_accuse_trace")
        return Accusation(arrs, rep, n, Audit(aarrs, arep, n, H))

    def accuse_last_trace(self, begin: int = 0, count: int = None, key_cap: int = 0, view_cap: int = 0,
                          rec_cap: int = None):
        """The same over the kept trace of the last launch (after crypto_verify with set_trace_keep; an equivocator's
        second frames are there with set_trace_twins), instances [begin, begin + count): emitted, audited and accused on
        the device (bftsim_accuse_last_trace)."""
        from .trace import Accusation, Audit
        count, frames = self._kept_range("accuse_last_trace", begin, count)
        H = self.cfg.heights
        o, arrs = _abi.alloc_accuse(frames, count, rec_cap)
        ao, aarrs = _abi.alloc_audit(frames, count, H)
        rep, arep = _abi.CAccuseReport(), _abi.CAuditReport()
        _check(self.h, lib().bftsim_accuse_last_trace(self.h, begin, count, key_cap, view_cap, ctypes.byref(o),
                                                      ctypes.byref(ao), ctypes.byref(arep), ctypes.byref(rep)),
               "bftsim_accuse_last_trace")
        return Accusation(arrs, rep, count, Audit(aarrs, arep, count, H))

    def accuse_ms(self):
        """(the observer's passes, walk, mark + scan + gather, copies) of the last accuse call, device ms
        (bftsim_accuse_last_ms)."""
        return self._last_ms("bftsim_accuse_last_ms", 4)

    def timeline_trace(self, trace, max_heights: int = None, key_cap: int = 0, tl_cap: int = 0):
        """The chronicler (include/bftsim.h bftsim_timeline_trace, SPEC.md §11h) over a bftsim.trace.Trace, or anything
        with its stream / frame_off / inst_frame0: per height the first prepare certificate, the round-change quorums and
        the verdicts that join them to the observer's commit certificate, tallied on the device over the Prepare and
        RoundChange frames the observer accepts. -> bftsim.trace.Timeline (its .audit: the observer's outputs of the
        same call)"""
        from .trace import Audit, Timeline
        stream, off, f0, frames, n, H, Hb = self._host_trace(trace, max_heights)
        o, arrs = _abi.alloc_timeline(n, Hb)
        ao, aarrs = _abi.alloc_audit(frames, n, Hb)
        rep, arep = _abi.CTimelineReport(), _abi.CAuditReport()
        _check(self.h, lib().bftsim_timeline_trace(self.h, stream.ctypes.data, len(stream), off.ctypes.data, frames,
                                                   f0.ctypes.data, n, H, key_cap, tl_cap, ctypes.byref(o), ctypes.byref(ao),
                                                   ctypes.byref(arep), ctypes.byref(rep)), "bftsim_timeline_trace")
        return Timeline(arrs, rep, n, H, Audit(aarrs, arep, n, H))

    def timeline_last_trace(self, begin: int = 0, count: int = None, key_cap: int = 0, tl_cap: int = 0):
        """The same over the kept trace of the last launch (after crypto_verify with set_trace_keep), instances
        [begin, begin + count): emitted, audited and chronicled on the device (bftsim_timeline_last_trace)."""
        from .trace import Audit, Timeline
        count, frames = self._kept_range("timeline_last_trace", begin, count)
        H = self.cfg.heights
        o, arrs = _abi.alloc_timeline(count, H)
        ao, aarrs = _abi.alloc_audit(frames, count, H)
        rep, arep = _abi.CTimelineReport(), _abi.CAuditReport()
        _check(self.h, lib().bftsim_timeline_last_trace(self.h, begin, count, key_cap, tl_cap, ctypes.byref(o),
                                                        ctypes.byref(ao), ctypes.byref(arep), ctypes.byref(rep)),
               "bftsim_timeline_last_trace")
        return Timeline(arrs, rep, count, H, Audit(aarrs, arep, count, H))

    def timeline_ms(self):
        """(the observer's passes, walk, rows, copies) of the last timeline call, device ms (bftsim_timeline_last_ms)."""
        return self._last_ms("bftsim_timeline_last_ms", 4)

    def _rollcall_result(self, call, what, frames, n, H, rec_cap, tl_cap):
        from .trace import Audit, RollCall, Timeline
        if self.cfg.n > 256:
            raise BftsimError(f"{what}: more than 256 validators")
        cap = tl_cap or 4 * H + 64
        o, arrs = _abi.alloc_rollcall(n, self.cfg.n, n * (H + cap) if rec_cap is None else rec_cap)
        ao, aarrs = _abi.alloc_audit(frames, n, H)
        to, tarrs = _abi.alloc_timeline(n, H)
        rep, arep, trep = _abi.CRollCallReport(), _abi.CAuditReport(), _abi.CTimelineReport()
        _check(self.h, call(ctypes.byref(o), ctypes.byref(rep), ctypes.byref(ao), ctypes.byref(arep), ctypes.byref(to),
                            ctypes.byref(trep)), what)
        audit = Audit(aarrs, arep, n, H)
        return RollCall(arrs, rep, n, self.cfg.n, audit, Timeline(tarrs, trep, n, H, audit))

    def rollcall_trace(self, trace, max_heights: int = None, key_cap: int = 0, tl_cap: int = 0, rec_cap: int = None):
        """The roll call (include/bftsim.h bftsim_rollcall_trace, SPEC.md §11i) over a bftsim.trace.Trace, or anything
        with its stream / frame_off / inst_frame0: per validator what it signed, and per view the wire proves started
        its proposer and whether that proposer's PrePrepare is there, found on the device behind the observer and the
        chronicler. rec_cap: every possible view by default (the pages of an np.empty cost nothing until written).
        -> bftsim.trace.RollCall (its .audit and .timeline: their outputs of the same call)"""
        stream, off, f0, frames, n, H, Hb = self._host_trace(trace, max_heights)
        call = lambda *tail: lib().bftsim_rollcall_trace(self.h, stream.ctypes.data, len(stream), off.ctypes.data, frames,
                                                         f0.ctypes.data, n, H, key_cap, tl_cap, *tail)
        return self._rollcall_result(call, "bftsim_rollcall_trace", frames, n, Hb, rec_cap, tl_cap)

    def rollcall_last_trace(self, begin: int = 0, count: int = None, key_cap: int = 0, tl_cap: int = 0, rec_cap: int = None):
        """The same over the kept trace of the last launch (after crypto_verify with set_trace_keep), instances
        [begin, begin + count): emitted, audited, chronicled and called on the device (bftsim_rollcall_last_trace)."""
        count, frames = self._kept_range("rollcall_last_trace", begin, count)
        call = lambda *tail: lib().bftsim_rollcall_last_trace(self.h, begin, count, key_cap, tl_cap, *tail)
        return self._rollcall_result(call, "bftsim_rollcall_last_trace", frames, count, self.cfg.heights, rec_cap, tl_cap)

    def rollcall_ms(self):
        """(the observer's passes, the chronicler's walk + rows, views, walk, scan + gather, copies) of the last roll
        call, device ms (bftsim_rollcall_last_ms)."""
        return self._last_ms("bftsim_rollcall_last_ms", 6)

    def set_ledger_votes(self, kind: str):
        """What the next crypto_verify keeps as the ledger's votes: "signatures" (the Commit messages' signatures, the
        default and the reference's) or "seals" (the Commits' seals, which verify_ledger can check;
        bftsim_set_ledger_votes, SPEC.md §11d)."""
        from .ledger import VOTE_KINDS
        if kind not in VOTE_KINDS:
            raise BftsimError(f"set_ledger_votes: {kind!r} is neither 'signatures' nor 'seals'")
        _check(self.h, lib().bftsim_set_ledger_votes(self.h, VOTE_KINDS[kind]), "bftsim_set_ledger_votes")

    def verify_ledger(self, ledger):
        """The importer (include/bftsim.h bftsim_verify_ledger, SPEC.md §11d) over what export_ledger() returns (per
        instance a list of header byte strings), or over raw (hdr, hdr_len, slot_bytes, heights) arrays in
        bftsim_export_ledger's layout: every header verified from its bytes on the device. -> bftsim.ledger.Verdict"""
        from .ledger import Verdict, pack
        if isinstance(ledger, tuple):
            hdr, lens, slot, H = ledger
        else:
            hdr, lens, slot, H = pack(ledger, heights=self.cfg.heights)
        hdr = np.ascontiguousarray(hdr, np.uint8).reshape(-1)
        lens = np.ascontiguousarray(lens, np.uint32).reshape(-1)
        ok = 0 < H <= 65535                        # the library refuses it; no buffers are sized by it here
        n = len(lens) // H if ok else 0
        o, arrs = _abi.alloc_ledger(n, H if ok else 0)
        rep = _abi.CLedgerReport()
        _check(self.h, lib().bftsim_verify_ledger(self.h, hdr.ctypes.data, slot, lens.ctypes.data, n, H, ctypes.byref(o),
                                                  ctypes.byref(rep)), "bftsim_verify_ledger")
        return Verdict(arrs, rep, n, H)

    def ledger_ms(self):
        """(decode, recoveries, tally + link, copies) of the last verify_ledger, device ms (bftsim_ledger_last_ms)."""
        return self._last_ms("bftsim_ledger_last_ms", 4)

    @staticmethod
    def comm_available():
        """raises unless librccl opens with every entry point libbftsim uses (bftsim_comm_available): the
        pre-flight each rank runs, and the ranks agree on, before any of them enters ncclCommInitRank"""
        rc = lib().bftsim_comm_available()
        if rc != 0:
            raise BftsimError(f"bftsim_comm_available failed ({rc}): librccl.so.1 cannot be opened")

    @staticmethod
    def comm_unique_id() -> bytes:
        """rank 0: the 128-byte RCCL id every rank passes to comm_init (include/bftsim.h)"""
        buf = ctypes.create_string_buffer(128)
        rc = lib().bftsim_comm_unique_id(buf)
        if rc != 0:
            raise BftsimError(f"bftsim_comm_unique_id failed ({rc})")
        return buf.raw

    def comm_init(self, world: int, rank: int, unique_id: bytes):
        assert len(unique_id) == 128
        _check(self.h, lib().bftsim_comm_init(self.h, world, rank, unique_id), "bftsim_comm_init")

    def stats_allreduce(self):
        """bftsim_stats of the last launch summed over every rank: one RCCL all-reduce in libbftsim"""
        s = _abi.CStats()
        _check(self.h, lib().bftsim_stats_allreduce(self.h, ctypes.byref(s)), "bftsim_stats_allreduce")
        return self._stats_dict(s)
