"""CPU: the forged signatures of tests/sig_cases.py, which reach the rare branches of secp256k1.h (the second wrap of
fe_reduce_wide, the fourth fold of sc_reduce_wide, recovery ids 2 and 3, jac_add_aff on equal and opposite points inside
mul_g, u1 = 0, an infinite result, the GLV and digit edges), through the host build of that source against the Python
oracle and the C oracle, item by item; the wrapping operands on the primitives themselves; keys at the corners of every
fixed-base window; signing at the edges of the digest range. No GPU needed."""
import numpy as np

import sig_cases as SC          # first: it puts oracle/ on the path
import oracle_lib as O
import secp256k1_ref as S
import sig_lib as H


def test_generator_reaches_what_it_claims():
    """the generator's own asserts ran (they fail loudly when a case stops reaching its branch); here its shape"""
    cases = SC.recover_cases()
    names = [c[0] for c in cases]
    for head, count in (("high-x", 6), ("fe_sqr wrap", 2), ("fe_mul wrap", 2), ("sc_mul wrap", 1), ("u1=0", 2),
                        ("digest e+n", 1), ("Q infinity", 1), ("mul_g doubling", 2), ("cancel mid-way", 1),
                        ("mul_var", len(SC.GLV_EDGES)), ("reject", 7)):
        assert sum(n.startswith(head) for n in names) == count, head
    assert sorted({c[2][64] for c in cases if c[0].startswith("high-x")}) == [2, 3]
    want = SC.recover_expected()
    none = [n for n, w in zip(names, want) if w is None]
    assert none == [n for n in names if n.startswith("reject") or n == "Q infinity"]
    # rejects and accepts interleave: no two rejects side by side, none at either end
    idx = [k for k, n in enumerate(names) if n.startswith("reject")]
    assert idx[0] > 0 and idx[-1] < len(names) - 1 and all(b - a > 1 for a, b in zip(idx, idx[1:]))
    assert SC.case("u1=0 digest 0")[1] == bytes(32) and SC.case("u1=0 digest n")[1] == S.N.to_bytes(32, "big")
    assert want[names.index("u1=0 digest 0")] == want[names.index("u1=0 digest n")] is not None
    # random operands do not reach the wraps (why the cases are constructed)
    import random
    rng = random.Random(1)
    assert not any(SC.fe_wraps(rng.randrange(S.P), rng.randrange(S.P)) for _ in range(2000))
    assert not any(SC.sc_wraps(rng.randrange(S.N), rng.randrange(S.N)) for _ in range(2000))


def test_recover_cases_three_way():
    """S.recover, the host build of secp256k1.h and the C oracle (alone and batched) agree on every case, on the public
    key or on None; the host build's address is the Keccak address of that key"""
    cases, want = SC.recover_cases(), SC.recover_expected()
    pubs, ok = O.secp_recover_batch(np.frombuffer(b"".join(c[1] for c in cases), np.uint8).reshape(-1, 32),
                                    np.frombuffer(b"".join(c[2] for c in cases), np.uint8).reshape(-1, 65), threads=3)
    for k, (name, dig, sig, why) in enumerate(cases):
        got = H.recover(dig, sig)
        if want[k] is None:
            assert got is None, (name, why)
        else:
            assert got is not None and got[0] == want[k], (name, why)
            assert got[1] == S.address(want[k], O.keccak256), (name, why)
        assert O.secp_recover(dig, sig) == want[k], (name, why)
        assert bool(ok[k]) == (want[k] is not None) and (want[k] is None or bytes(pubs[k]) == want[k]), (name, why)


def test_wrap_operands_on_the_primitives():
    W = SC.wrap_operands()
    assert [t - SC.C for _, t in W["fe_sqr"]] == [1, 3] and [t - SC.C for _, t in W["fe_mul"]] == [0, 1]
    for x, t in W["fe_sqr"]:
        assert SC.fe_wraps(x, x) and H.op("fe_sqr", x) == t, hex(x)
        assert H.op("fe_mul", x, x) == t, hex(x)
    for x, t in W["fe_mul"]:
        assert SC.fe_wraps(x, SC.BETA) and H.op("fe_mul", x, SC.BETA) == t == H.op("fe_mul", SC.BETA, x), hex(x)
    for s, rinv, u2, _ in W["sc_mul"]:
        assert u2 - SC.NC == 2 and SC.sc_wraps(s, rinv) and H.op("sc_mul", s, rinv) == u2 == H.op("sc_mul", rinv, s)
    pairs = SC.sc_wrap_pairs()
    assert 100 <= len(pairs) <= 300
    for a, b, t in pairs:
        assert H.op("sc_mul", a, b) == t == a * b % S.N, (hex(a), hex(b))


def test_keys_at_the_table_corners():
    """entry 1 and entry 255 of each of the 32 fixed-base windows alone, and the ends of the secret range"""
    for name, sec, valid in SC.key_cases():
        got = H.pub(sec)
        if not valid:
            assert got is None, name
            continue
        want = S.pubkey(sec)
        assert got == (want, S.address(want, O.keccak256)), name
        assert O.secp_pubkey(sec) == want, name


def test_signing_at_the_digest_edges():
    secrets, items = SC.sign_cases()
    for k, dig in items:
        sig = H.sign(secrets[k], dig)
        assert sig == S.sign(secrets[k], dig), (k, dig.hex())
        assert H.recover(dig, sig)[0] == S.pubkey(secrets[k])
