"""secp256k1 on the GPU through the C ABI (include/bftsig.h): bit-exact against the CPU oracle
(oracle/secp256k1_ref.py) and the golden vectors, plus size-independent properties at full batch
sizes (sign -> recover round trip, verify_address, corruption rejected)."""
import json
import os
import random
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "consensus-rs_amd"))
import secp256k1_ref as S  # noqa: E402
import oracle_lib as O  # noqa: E402

pytestmark = pytest.mark.gpu
GOLD = json.load(open(os.path.join(ROOT, "tests", "golden", "sig_vectors.json")))


@pytest.fixture(scope="module")
def signer():
    from bftsim.sig import Signer
    s = Signer(0)
    yield s
    s.close()


def arr(rows):
    return np.frombuffer(b"".join(rows), dtype=np.uint8).reshape(len(rows), -1).copy()


def test_reference_keys_on_gpu(signer):
    secs = arr([bytes.fromhex(k["secret"]) for k in GOLD["reference_keys"]])
    pub, addr, ok = signer.secret_to_address(secs)
    assert ok.cpu().numpy().tolist() == [1] * 5
    assert [bytes(a).hex() for a in addr.cpu().numpy()] == [k["address"] for k in GOLD["reference_keys"]]


def test_golden_vectors_on_gpu(signer):
    V = GOLD["vectors"]
    secs = arr([bytes.fromhex(v["secret"]) for v in V])
    digs = arr([bytes.fromhex(v["digest"]) for v in V])
    pub, addr, ok = signer.secret_to_address(secs)
    assert (ok.cpu().numpy() == 1).all()
    assert [bytes(p).hex() for p in pub.cpu().numpy()] == [v["pub"] for v in V]
    sig, ok = signer.sign(secs, digs)
    assert (ok.cpu().numpy() == 1).all()
    assert [bytes(s).hex() for s in sig.cpu().numpy()] == [v["sig"] for v in V]
    rpub, raddr, ok = signer.recover(digs, sig)
    assert (ok.cpu().numpy() == 1).all()
    assert [bytes(a).hex() for a in raddr.cpu().numpy()] == [v["address"] for v in V]
    bad = GOLD["invalid"]
    _, baddr, bok = signer.recover(arr([bytes.fromhex(b["digest"]) for b in bad]),
                                   arr([bytes.fromhex(b["sig"]) for b in bad]))
    assert (bok.cpu().numpy() == 0).all() and (baddr.cpu().numpy() == 0).all()


def test_seeded_batch_matches_oracle(signer):
    rng = random.Random(5)
    n = 96
    secs = [rng.randrange(1, S.N).to_bytes(32, "big") for _ in range(n)]
    digs = [bytes(rng.randrange(256) for _ in range(32)) for _ in range(n)]
    sig, ok = signer.sign(arr(secs), arr(digs))
    sig = sig.cpu().numpy()
    assert (ok.cpu().numpy() == 1).all()
    for i in range(n):
        assert bytes(sig[i]) == S.sign(secs[i], digs[i]), i
    # recover with random recovery ids: valid or not, GPU and oracle agree
    mangled = [bytes(sig[i][:64]) + bytes([rng.randrange(4)]) for i in range(n)]
    pub, addr, ok = signer.recover(arr(digs), arr(mangled))
    pub, ok = pub.cpu().numpy(), ok.cpu().numpy()
    for i in range(n):
        want = S.recover(digs[i], mangled[i])
        assert ok[i] == (want is not None), i
        if want is not None:
            assert bytes(pub[i]) == want, i


def test_key_index_and_invalid_secrets(signer):
    secs = arr([bytes(32), bytes.fromhex(GOLD["reference_keys"][0]["secret"]), S.N.to_bytes(32, "big")])
    digs = arr([O.keccak256(b"m%d" % i) for i in range(6)])
    sig, ok = signer.sign(secs, digs, key_index=[1, 0, 2, 1, 1, 0])
    assert ok.cpu().numpy().tolist() == [1, 0, 0, 1, 1, 0]
    sig = sig.cpu().numpy()
    assert bytes(sig[0]) == S.sign(bytes.fromhex(GOLD["reference_keys"][0]["secret"]), bytes(digs[0]))
    assert not sig[1].any()


def test_full_batch_round_trip(signer):
    """65,536 signatures (the per-height message volume of 1,024 N=64 clusters): every one recovers to
    its signer's address and passes verify_address; one flipped digest bit fails it."""
    import torch
    n, keys = 65_536, 64
    g = torch.Generator().manual_seed(9)
    secs = torch.randint(0, 256, (keys, 32), dtype=torch.uint8, generator=g)
    secs[:, 0] &= 0x7f                                  # < n
    digs = torch.randint(0, 256, (n, 32), dtype=torch.uint8, generator=g)
    kidx = torch.arange(n, dtype=torch.int32) % keys
    _, kaddr, kok = signer.secret_to_address(secs)
    assert bool((kok == 1).all())
    sig, ok = signer.sign(secs, digs, key_index=kidx)
    assert bool((ok == 1).all())
    s = sig.cpu().numpy()
    assert (s[:, 64] <= 1).all()                        # R.x >= n never happens in practice
    assert all(int.from_bytes(bytes(s[i, 32:64]), "big") <= S.N // 2 for i in range(0, n, 4099))
    _, addr, ok = signer.recover(digs, sig, want_pub=False)
    assert bool((ok == 1).all())
    want = kaddr[kidx.to(kaddr.device).long()]
    assert bool((addr == want).all())
    assert bool((signer.verify_address(want, digs, sig) == 1).all())
    d2 = digs.clone()
    d2[:, 31] ^= 1
    assert not bool(signer.verify_address(want, d2, sig).any())
    for i in (0, 12345, n - 1):                        # spot checks against the oracle
        assert bytes(s[i]) == S.sign(bytes(secs[i % keys].numpy()), bytes(digs[i].numpy()))


def test_recover_matches_c_oracle_4096(signer):
    """4,096 recoveries with random recovery ids (about half do not recover, or recover another key):
    GPU and the C oracle (oracle/secp_oracle.c, an independent implementation) agree item by item."""
    import torch
    g = torch.Generator().manual_seed(17)
    n, keys = 4096, 32
    secs = torch.randint(0, 256, (keys, 32), dtype=torch.uint8, generator=g)
    secs[:, 0] &= 0x7f
    digs = torch.randint(0, 256, (n, 32), dtype=torch.uint8, generator=g)
    sig, ok = signer.sign(secs, digs, key_index=torch.arange(n, dtype=torch.int32) % keys)
    assert bool((ok == 1).all())
    s = sig.cpu().numpy().copy()
    s[:, 64] = torch.randint(0, 4, (n,), generator=g).numpy()
    pub, _, ok = signer.recover(digs, s)
    want, wok = O.secp_recover_batch(digs.numpy(), s, threads=16)
    assert (ok.cpu().numpy() == wok).all()
    assert (pub.cpu().numpy()[wok == 1] == want[wok == 1]).all()
    assert (pub.cpu().numpy()[wok == 0] == 0).all()


# ---- forged signatures that reach the rare branches (tests/sig_cases.py), through sig_recover_kernel's TabLds path
@pytest.fixture(scope="module")
def forged():
    """every recover case, padded with seeded valid signatures to 64 k + 1 items (one live lane in the last block),
    with the oracle's public key (zero where none), address and ok of each item: the Python oracle's for the cases,
    the C oracle's for the padding (signed by the host build, as tests/ledger_ref.py seals); computed once, read-only"""
    import sig_cases as SC
    import sig_lib
    cases = SC.recover_cases()
    want = list(SC.recover_expected())
    digs, sigs = [c[1] for c in cases], [c[2] for c in cases]
    rng = random.Random(SC.SEED + 2)
    n = ((len(cases) + 63) // 64 + 1) * 64 + 1
    assert len(cases) < 64 < n < 300
    while len(digs) < n:
        sec = rng.randrange(1, S.N).to_bytes(32, "big")
        d = bytes(rng.randrange(256) for _ in range(32))
        digs.append(d), sigs.append(sig_lib.sign(sec, d)), want.append(O.secp_pubkey(sec))
        assert O.secp_recover(d, sigs[-1]) == want[-1] is not None
    ok = np.array([w is not None for w in want], np.uint8)
    pub = arr([w if w is not None else bytes(64) for w in want])
    addr = arr([S.address(w, O.keccak256) if w is not None else bytes(20) for w in want])
    names = [c[0] for c in cases] + ["padding"] * (n - len(cases))
    out = dict(n=n, names=names, dig=arr(digs), sig=arr(sigs), ok=ok, pub=pub, addr=addr)
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


def _check_recover(signer, F, idx):
    """the items idx of the forged batch, in that order, through recover (with and without pub) and verify_address"""
    idx = np.asarray(idx)
    dig, sig = F["dig"][idx].copy(), F["sig"][idx].copy()
    wok, wpub, waddr = F["ok"][idx], F["pub"][idx], F["addr"][idx]
    names = [F["names"][k] for k in idx]
    diff = lambda got, exp: [names[k] for k in np.nonzero((np.asarray(got).reshape(len(idx), -1) !=
                                                           np.asarray(exp).reshape(len(idx), -1)).any(axis=1))[0]]
    pub, addr, ok = signer.recover(dig, sig)
    assert not diff(ok.cpu().numpy(), wok), ("ok", diff(ok.cpu().numpy(), wok))
    assert not diff(pub.cpu().numpy(), wpub), ("pub", diff(pub.cpu().numpy(), wpub))      # zero where it failed
    assert not diff(addr.cpu().numpy(), waddr), ("addr", diff(addr.cpu().numpy(), waddr))
    none, addr, ok = signer.recover(dig, sig, want_pub=False)
    assert none is None
    assert not diff(ok.cpu().numpy(), wok) and not diff(addr.cpu().numpy(), waddr)
    got = signer.verify_address(waddr.copy(), dig, sig).cpu().numpy()
    assert not diff(got, wok), ("verify_address", diff(got, wok))
    flipped = waddr.copy()
    flipped[np.arange(len(idx)), np.arange(len(idx)) % 20] ^= (1 << (np.arange(len(idx)) % 8)).astype(np.uint8)
    assert not signer.verify_address(flipped, dig, sig).cpu().numpy().any()
    # against the all-zero address nothing that fails to recover may pass (the kernel's address is unset there)
    got = signer.verify_address(np.zeros((len(idx), 20), np.uint8), dig, sig).cpu().numpy()
    assert not got[wok == 0].any(), [names[k] for k in np.nonzero(got)[0]]
    assert waddr[wok == 1].any(axis=1).all() and not got.any()


@pytest.mark.parametrize("order", ["forward", "reversed"])
def test_forged_batch_matches_oracle(signer, forged, order):
    """rejects, infinite results and full recoveries share wavefronts; each case meets other lane neighbours in the
    reversed batch, where the single lane of the last block is a recovery id 2 case"""
    idx = np.arange(forged["n"])
    assert forged["n"] % 64 == 1 and forged["names"][0].startswith("high-x")
    assert {0, 1} == set(forged["ok"][:64].tolist())
    _check_recover(signer, forged, idx if order == "forward" else idx[::-1])


def test_forged_batch_shape_edges(signer, forged):
    """n = 1 (a recovery id 2 signature alone in its block) and n = 65 (a full block and one lane)"""
    assert forged["sig"][0, 64] & 2 and forged["ok"][0] == 1
    _check_recover(signer, forged, [0])
    _check_recover(signer, forged, np.arange(65))


def test_keys_at_the_table_corners_on_gpu(signer):
    """secrets 256^w and 255 * 256^w: the first and the last entry of every window of the uploaded fixed-base table,
    each alone in its scalar; the ends of the secret range; invalid secrets zeroed"""
    import sig_cases as SC
    K = SC.key_cases()
    pub, addr, ok = signer.secret_to_address(arr([k[1] for k in K]))
    pub, addr, ok = pub.cpu().numpy(), addr.cpu().numpy(), ok.cpu().numpy()
    assert len(K) == 70 and ok.tolist() == [int(k[2]) for k in K]
    for i, (name, sec, valid) in enumerate(K):
        want = S.pubkey(sec) if valid else bytes(64)
        assert bytes(pub[i]) == want, name
        assert bytes(addr[i]) == (S.address(want, O.keccak256) if valid else bytes(20)), name


def test_signing_at_the_digest_edges_on_gpu(signer):
    """secrets 1, n - 1 and a reference key over the digests 0, n - 1, n, n + 1, 2^256 - 1, in one call through
    key_index; every signature the oracle's, and recovered on the GPU to its signer's address"""
    import sig_cases as SC
    secrets, items = SC.sign_cases()
    digs = arr([d for _, d in items])
    kidx = [k for k, _ in items]
    sig, ok = signer.sign(arr(secrets), digs, key_index=kidx)
    assert len(items) == 15 and (ok.cpu().numpy() == 1).all()
    s = sig.cpu().numpy()
    for i, (k, d) in enumerate(items):
        assert bytes(s[i]) == S.sign(secrets[k], d), (k, d.hex())
    _, kaddr, kok = signer.secret_to_address(arr(secrets))
    assert (kok.cpu().numpy() == 1).all()
    want = kaddr.cpu().numpy()[kidx]
    assert [bytes(a) for a in want] == [S.address(S.pubkey(secrets[k]), O.keccak256) for k in kidx]
    _, addr, ok = signer.recover(digs, sig)
    assert (ok.cpu().numpy() == 1).all() and (addr.cpu().numpy() == want).all()
    assert (signer.verify_address(want, digs, sig).cpu().numpy() == 1).all()
