"""GPU: the trace (include/bftsim.h bftsim_set_trace_keep / bftsim_trace_sizes / bftsim_export_trace, SPEC.md §11b):
a run's consensus traffic as signed wire frames. Small shapes equal the Python reference (tests/trace_ref.py) byte
for byte; larger ones are checked by structure and by the receiver's side (bftsim.trace.audit: decode, recover,
membership), and tied to the verify pass through its per-instance signature checksum."""
import numpy as np
import pytest

import trace_ref as TR
from bftsim.configs import BftConfig, cfg3, cfg4

pytestmark = pytest.mark.gpu


def _sim(cfg, secrets, forged=(), log_cap=0, keep=True):
    from bftsim.runtime import Simulator
    sim = Simulator(cfg)
    sim.set_crypto(secrets, forged, log_cap)
    sim.set_trace_keep(keep)
    return sim


def _keyed(cfg, seed):
    from bftsim.crypto import synthetic_secrets, keyed_config, gpu_addresses
    sec = synthetic_secrets(cfg.n, seed)
    return keyed_config(cfg, sec, gpu_addresses(sec))


def _same(tr, want):
    stream, off, meta, f0 = want
    assert np.array_equal(tr.frame_off, off)
    assert tr.stream.tobytes() == stream
    assert np.array_equal(tr.meta, meta)
    assert np.array_equal(tr.inst_frame0, f0)


def _structure(tr, inst_messages):
    """offsets strictly increasing from 0 to the stream's end; each instance's slice splits into its frames"""
    from bftsim import wire
    off = tr.frame_off.astype(np.int64)
    assert off[0] == 0 and off[-1] == len(tr.stream) and (np.diff(off) > 4).all()
    assert np.array_equal(tr.inst_frame0, np.concatenate([[0], np.cumsum(inst_messages)]).astype(np.uint64))
    for i in range(len(inst_messages)):
        a, b = int(tr.inst_frame0[i]), int(tr.inst_frame0[i + 1])
        assert np.array_equal(wire.split_frames(tr.instance_stream(i), max_frames=b - a + 1).astype(np.int64),
                              off[a:b + 1] - off[a])
        assert (tr.instance[a:b] == i).all()


def _audit(tr, cfg, rep):
    """the receiver's side: every honest frame recovers to its sender, no forged one to any validator; the XOR of
    keccak(signature || seal or zeros) over the decoded frames is the verify pass's checksum"""
    from bftsim.runtime import keccak256
    from bftsim.sig import Signer
    from bftsim.trace import audit
    from bftsim.wire import Codec
    cd, sg = Codec(), Signer()
    try:
        dec = {}
        who = audit(tr, cfg.addresses, cd, sg, decoded=dec)
    finally:
        cd.close()
        sg.close()
    forged = (tr.flags & 1) != 0
    assert np.array_equal(who[~forged], tr.sender[~forged].astype(np.int32))
    assert (who[forged] == -1).all()
    assert np.array_equal(dec["has_seal"], tr.code == 3)
    ck = np.zeros((len(tr.inst_frame0) - 1, 32), np.uint8)
    zeros = bytes(65)
    for k in range(len(tr)):
        term = keccak256(dec["signature"][k].tobytes() + (dec["commit_seal"][k].tobytes() if dec["has_seal"][k] else zeros))
        ck[tr.instance[k]] ^= np.frombuffer(term, np.uint8)
    assert np.array_equal(ck, rep["checksum"])
    return who


def test_cfg1_equals_reference():
    """cfg1 N=5, c1..c5 keys, 6 heights: round changes (the 9-byte create_time), Preprepare frames, Commit seals"""
    ref = TR.reference("cfg1")
    sim = _sim(ref["cfg"], ref["secrets"])
    try:
        sim.run(0, 1)
        rep = sim.crypto_verify()
        fr, by = sim.trace_sizes()
        tr = sim.export_trace()
    finally:
        sim.close()
    _same(tr, TR.joined(ref))
    assert int(fr[0]) == len(tr) and int(by[0]) == len(tr.stream)
    assert {1, 2, 3, 4} <= set(tr.code.tolist())
    assert tr.frames(0)[0] == TR.frame_of(ref["inst"][0][3][0])
    # keep changes nothing the verify pass reports
    sim = _sim(ref["cfg"], ref["secrets"], keep=False)
    try:
        sim.run(0, 1)
        off = sim.crypto_verify()
    finally:
        sim.close()
    for k, v in rep.items():
        assert np.array_equal(v, off[k]), k


def test_lossy_forged_ranges_equal_reference():
    """N=4, seed 21, drops, instances 3..5, validator 2 forged: unequal counts, a non-zero first instance, forged
    frames, non-canonical blocks; a range is the matching piece of the whole"""
    ref = TR.reference("n4")
    sim = _sim(ref["cfg"], ref["secrets"], forged=ref["forged"], log_cap=1024)    # 514 messages in instance 5
    try:
        sim.run(ref["first"], 3)
        rep = sim.crypto_verify()
        fr, by = sim.trace_sizes()
        full = sim.export_trace(0, 3)
        tail = sim.export_trace(1, 2)
        one = sim.export_trace(2)
    finally:
        sim.close()
    assert np.array_equal(rep["inst_messages"], ref["res"]["mlog_n"]) and len(set(fr.tolist())) == 3
    _same(full, TR.joined(ref))
    _same(tail, TR.joined(ref, 1, 2))
    _same(one, TR.joined(ref, 2, 1))
    assert np.array_equal(full.inst_frame0, np.concatenate([[0], np.cumsum(ref["res"]["mlog_n"])]).astype(np.uint64))
    k, b = int(full.inst_frame0[1]), int(full.frame_off[int(full.inst_frame0[1])])
    assert tail.stream.tobytes() == full.stream[b:].tobytes()
    assert np.array_equal(tail.frame_off, full.frame_off[k:] - np.uint64(b))
    assert np.array_equal(tail.meta[:, :3], full.meta[k:, :3]) and np.array_equal(tail.meta[:, 3] + 1, full.meta[k:, 3])
    assert np.array_equal(fr, np.diff(full.inst_frame0).astype(np.uint32))
    assert np.array_equal(by, np.diff(full.frame_off[full.inst_frame0.astype(np.int64)]))
    assert (full.flags & 1).any() and ((full.flags & 1) != 0).sum() == rep["forged"]
    _structure(full, rep["inst_messages"])


def test_cfg3_round_trip():
    """cfg3, 4 heights, 4 instances, validators 0 and 5 forged (round-change storms: too many frames for Python
    signing) through the receiver"""
    cfg, secrets = _keyed(cfg3(heights=4), 3)
    sim = _sim(cfg, secrets, forged=(0, 5), log_cap=16384)
    try:
        sim.run(0, 4)
        rep = sim.crypto_verify()
        fr, by = sim.trace_sizes()
        tr = sim.export_trace()
    finally:
        sim.close()
    assert rep["mismatches"] == 0 and rep["forged"] > 0 and len(tr) == rep["messages"] > 4096
    assert np.array_equal(fr, rep["inst_messages"]) and int(by.sum()) == len(tr.stream)
    _structure(tr, rep["inst_messages"])
    who = _audit(tr, cfg, rep)
    assert (who >= 0).sum() == rep["recovered_as_sender"]


def test_n100_round_trip():
    """N=100 (a segment-kernel log, senders above 63), 2 heights, synthetic keys"""
    cfg, secrets = _keyed(cfg4(100, heights=2), 5)
    sim = _sim(cfg, secrets)
    try:
        sim.run(0, 1)
        rep = sim.crypto_verify()
        tr = sim.export_trace()
    finally:
        sim.close()
    assert len(tr) == rep["messages"] > 0 and int(tr.sender.max()) > 63
    _structure(tr, rep["inst_messages"])
    _audit(tr, cfg, rep)


def test_error_paths_write_nothing():
    """keep off, no verify since the launch, a short stream or frame buffer, a range past the launch:
    BFTSIM_EINVAL, a last-error text, and the caller's buffers untouched"""
    from bftsim.runtime import Simulator, lib
    cfg, secrets = _keyed(BftConfig(n=4, heights=3, seed=2), 1)
    L = lib()
    stream, off = np.full(1 << 20, 0xA5, np.uint8), np.full(4096, 0xA5A5A5A5A5A5A5A5, np.uint64)
    meta, f0 = np.full((4096, 4), 0xA5A5A5A5, np.uint32), np.full(8, 0xA5A5A5A5A5A5A5A5, np.uint64)

    def export(sim, begin, count, stream_cap, frame_cap):
        return L.bftsim_export_trace(sim.h, begin, count, stream.ctypes.data, stream_cap, off.ctypes.data, frame_cap,
                                     meta.ctypes.data, f0.ctypes.data)

    def refused(rc, sim):
        assert rc == -1 and len(L.bftsim_last_error(sim.h)) > 0
        assert (stream == 0xA5).all() and (off == 0xA5A5A5A5A5A5A5A5).all() and (meta == 0xA5A5A5A5).all() and \
            (f0 == 0xA5A5A5A5A5A5A5A5).all()

    sim = Simulator(cfg)
    try:
        sim.set_crypto(secrets)
        sim.run(0, 2)
        sim.crypto_verify()
        refused(export(sim, 0, 2, len(stream), 4095), sim)                     # keep off
        assert L.bftsim_trace_sizes(sim.h, 2, None, None) == -1
        sim.set_trace_keep(True)
        refused(export(sim, 0, 2, len(stream), 4095), sim)                     # keep on after that verify: nothing kept
        sim.run(0, 2)
        refused(export(sim, 0, 2, len(stream), 4095), sim)                     # no verify since the launch
        sim.crypto_verify()
        fr, by = sim.trace_sizes()
        frames, nbytes = int(fr.sum()), int(by.sum())
        assert 0 < frames < 4095 and nbytes < len(stream)
        refused(export(sim, 0, 2, nbytes - 1, frames), sim)                    # stream one byte short
        refused(export(sim, 0, 2, nbytes, frames - 1), sim)                    # frame buffers one short
        refused(export(sim, 0, 3, len(stream), 4095), sim)                     # range past the launch
        refused(export(sim, 3, 0, len(stream), 4095), sim)
        refused(export(sim, 1, 2, len(stream), 4095), sim)
        assert L.bftsim_trace_sizes(sim.h, 1, fr.ctypes.data, by.ctypes.data) == -1      # capacity below the launch
        assert export(sim, 0, 2, nbytes, frames) == 0                          # exact capacities are enough
        assert int(off[frames]) == nbytes and int(f0[2]) == frames and (stream[nbytes:] == 0xA5).all()
        stream[:], off[:], meta[:], f0[:] = 0xA5, 0xA5A5A5A5A5A5A5A5, 0xA5A5A5A5, 0xA5A5A5A5A5A5A5A5
        sim.launch(0)
        sim.sync()
        refused(export(sim, 0, 2, len(stream), 4095), sim)                     # the next launch dropped it
    finally:
        sim.close()
