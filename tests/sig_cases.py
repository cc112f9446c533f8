"""Forged recoverable signatures that steer secp256k1.h's `recover` into the branches random inputs never reach, shared
by the CPU and the GPU tests (not a test file). For a chosen curve point R = (x, y) and chosen scalars u1, u2 the
signature r = x (or x - n with recid |= 2), s = u2 r, digest = -u1 r (mod n), recid & 1 = y & 1 makes `recover` compute
exactly u1 G + u2 R, so the caller decides which table entries meet which accumulator and which operands the
reductions see. Only oracle/secp256k1_ref.py (S) is imported: the expected results are the oracle's, and every "this
case reaches that branch" claim is an assert here, on models of the reduction folds written from the arithmetic or on
point equalities by S.point_mul. Deterministic: one fixed seed."""
from __future__ import annotations

import functools
import json
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import secp256k1_ref as S  # noqa: E402

P, N = S.P, S.N
C = 2 ** 32 + 977                    # 2^256 mod p
NC = 2 ** 256 - N                    # 2^256 mod n
LAMBDA = 0x5363AD4CC05C30E0A5261C028812645A122E22EA20816678DF02967C1B23BD72
BETA = 0x7AE96A2B657C07106E64479EAC3434E99CF0497512F58995C1396C28719501EE
SEED = 20260
# the scalars of test_sig_cpu.test_glv_mul_var_edge_scalars, then the small ones around the radix-8 digit range
GLV_EDGES = (1, 2, 15, 16, 17, N - 1, N - 2, N // 2, N // 2 + 1, LAMBDA, N - LAMBDA, 2 ** 128 - 1, 2 ** 128, 2 ** 128 + 1,
             int("7" * 64, 16), int("8" * 63, 16), (LAMBDA * 3) % N, 3, 4, 5, 7, 8, 9)
GOLD = json.load(open(os.path.join(ROOT, "tests", "golden", "sig_vectors.json")))


def b32(v: int) -> bytes:
    return v.to_bytes(32, "big")


def inv_n(v: int) -> int:
    return pow(v, N - 2, N)


def neg(pt):
    return None if pt is None else (pt[0], (P - pt[1]) % P)


def pub64(pt) -> bytes:
    return b32(pt[0]) + b32(pt[1])


def lift(x: int, odd):
    """the curve point with this x and this y parity, or None"""
    if not 0 <= x < P:
        return None
    y2 = (x * x * x + 7) % P
    y = pow(y2, (P + 1) // 4, P)
    if y * y % P != y2:
        return None
    return (x, y if (y & 1) == (1 if odd else 0) else P - y)


def split_r(R):
    """(r, recid) of a signature whose R is this point: r = x mod n, recid = (x >= n) << 1 | y & 1"""
    x, y = R
    r, rid = (x - N, 2) if x >= N else (x, 0)
    return r, rid | (y & 1)


def sig_of(u2: int, R) -> bytes:
    """r || s || recid with s = u2 r: over a digest e it recovers to (-e / r) G + u2 R"""
    r, recid = split_r(R)
    s = u2 * r % N
    assert 0 < r < N and s != 0
    return b32(r) + b32(s) + bytes([recid])


def forge(u1: int, u2: int, R):
    """-> (digest32, sig65) on which recover computes u1 G + u2 R"""
    sig = sig_of(u2, R)
    r = int.from_bytes(sig[:32], "big")
    return b32(-u1 * r % N), sig


def forge_infinity(digest: bytes, k: int) -> bytes:
    """a signature that recovers to infinity over a GIVEN digest e != 0 (mod n): R = k G, s = e / k, so that
    u1 G + u2 R = (-e / r) G + (e / (r k)) k G"""
    e = int.from_bytes(digest, "big") % N
    R = S.point_mul(k)
    r, recid = split_r(R)
    s = e * inv_n(k) % N
    assert 0 < r < N and s != 0
    return b32(r) + b32(s) + bytes([recid])


def fe_wraps(a: int, b: int) -> bool:
    """fe_reduce_wide(a * b) takes its second wrap: with the product lo + hi 2^256, the first fold gives
    v1 = lo + hi C; its part above 2^256 is folded once more, and that sum passes 2^256 again"""
    t = a * b
    v1 = (t % 2 ** 256) + (t >> 256) * C
    top, r = v1 >> 256, v1 % 2 ** 256
    return r + top * C >= 2 ** 256


def sc_wraps(a: int, b: int) -> bool:
    """sc_reduce_wide(a * b) needs its fourth fold: three folds of 2^256 -> 2^256 - n leave a value >= 2^256"""
    t = a * b
    for _ in range(3):
        t = (t % 2 ** 256) + (t >> 256) * NC
    return t >= 2 ** 256


def glv_split(k: int):
    """k = k1 + k2 lambda (mod n) as split_lambda computes it (libsecp256k1's published lattice constants and rounded
    multiplications), both halves as signed integers"""
    g1 = 0x3086D221A7D46BCDE86C90E49284EB153DAA8A1471E8CA7FE893209A45DBB031
    g2 = 0xE4437ED6010E88286F547FA90ABFE4C4221208AC9DF506C61571B4AE8AC47F71
    mb1 = 0xE4437ED6010E88286F547FA90ABFE4C3
    mb2 = 0xFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFE8A280AC50774346DD765CDA83DB1562C
    c1, c2 = (k * g1 + 2 ** 383) >> 384, (k * g2 + 2 ** 383) >> 384
    k2 = (c1 * mb1 + c2 * mb2) % N
    k1 = (k - k2 * LAMBDA) % N
    assert (k1 + k2 * LAMBDA - k) % N == 0
    return tuple(v - N if v > N // 2 else v for v in (k1, k2))


def high_x_points(count: int = 3):
    """the first `count` x in (n, p) on the curve, each with its even-y and its odd-y point"""
    out, x = [], N + 1
    while len(out) < count:
        if lift(x, 0) is not None:
            out.append((lift(x, 0), lift(x, 1)))
        x += 1
    return out


@functools.lru_cache(maxsize=None)
def wrap_operands() -> dict:
    """the operands that make a reduction wrap, with the product each must give:
    fe_sqr [(x, t)]: x^2 = t (mod p);  fe_mul [(x, t)]: x beta = t (mod p);  sc_mul [(s, rinv, u2, R)]: s / r = u2 (mod n)
    every x is below n and on the curve, so it can be a signature's r"""
    sqr, t = [], C
    while len(sqr) < 2:
        root = pow(t, (P + 1) // 4, P)
        if root * root % P == t:
            for x in sorted((root, P - root)):
                if x < N and lift(x, 0) is not None and fe_wraps(x, x):
                    sqr.append((x, t))
                    break
        t += 1
    mul, t = [], C
    binv = pow(BETA, P - 2, P)
    while len(mul) < 2:
        x = t * binv % P
        if x < N and lift(x, 0) is not None and fe_wraps(x, BETA):
            mul.append((x, t))
        t += 1
    R = S.point_mul(0x1234567)
    r = R[0]
    assert r < N
    rinv, i = inv_n(r), 0
    while not sc_wraps((NC + i) * r % N, rinv):
        i += 1
    u2 = NC + i
    for x, t in sqr:
        assert x * x % P == t and fe_wraps(x, x)
    for x, t in mul:
        assert x * BETA % P == t and fe_wraps(x, BETA)
    assert (u2 * r % N) * rinv % N == u2 and sc_wraps(u2 * r % N, rinv)
    return dict(fe_sqr=sqr, fe_mul=mul, sc_mul=[(u2 * r % N, rinv, u2, R)])


@functools.lru_cache(maxsize=None)
def sc_wrap_pairs(candidates: int = 2000):
    """[(a, b, t)] with a b = t (mod n) for a small t >= 2^256 - n, those of `candidates` seeded pairs that take
    sc_reduce_wide's fourth fold (about one in twelve)"""
    rng = random.Random(SEED + 1)
    out = []
    for i in range(candidates):
        a = rng.randrange(1, N)
        t = NC + i
        b = t * inv_n(a) % N
        if sc_wraps(a, b):
            out.append((a, b, t))
    assert len(out) >= 100, len(out)
    return out


@functools.lru_cache(maxsize=None)
def _recover_cases():
    rng = random.Random(SEED)
    rs = lambda: rng.randrange(2 ** 200, N)            # an arbitrary scalar that is none of the edges below
    base = S.point_mul(12345)
    out = []

    def add(name, dig, sig, why, expect="key"):
        got = S.recover(dig, sig)                      # the expected result, kept as the case's fifth field
        assert (got is None) == (expect is None), name
        if expect not in (None, "key"):
            assert got == pub64(expect), name
        out.append((name, dig, sig, why, got))

    # recovery ids 2 and 3 with x = r + n < p
    for pair in high_x_points(3):
        for R in pair:
            r, recid = split_r(R)
            assert N < R[0] < P and recid == 2 | (R[1] & 1) and S.on_curve(R)
            u1, u2 = rs(), rs()
            dig, sig = forge(u1, u2, R)
            assert sig[64] == recid and int.from_bytes(sig[:32], "big") == R[0] - N
            add(f"high-x r={r} recid={recid}", dig, sig, "recid & 2 with r + n < p",
                S.point_add(S.point_mul(u1), S.point_mul(u2, R)))
    assert {c[2][64] for c in out} == {2, 3}
    W = wrap_operands()
    # the second wrap of fe_reduce_wide, in fe_sqr(x) at the top of recover
    for x, t in W["fe_sqr"]:
        dig, sig = forge(rs(), rs(), lift(x, 0))
        add(f"fe_sqr wrap t=C+{t - C}", dig, sig, "fe_reduce_wide's second wrap in fe_sqr(x)")
    # ... and in fe_mul(x, beta): u2 = lambda splits into (0, 1), so the lambda half adds (beta x, y)
    for x, t in W["fe_mul"]:
        R = lift(x, 1)
        assert S.point_mul(LAMBDA, R) == (t, R[1]) and glv_split(LAMBDA) == (0, 1)
        dig, sig = forge(rs(), LAMBDA, R)
        add(f"fe_mul wrap t=C+{t - C}", dig, sig, "fe_reduce_wide's second wrap in fe_mul(x, beta) of mul_var")
    # the fourth fold of sc_reduce_wide, in u2 = sc_mul(s, 1 / r)
    for s, rinv, u2, R in W["sc_mul"]:
        dig, sig = forge(rs(), u2, R)
        assert int.from_bytes(sig[32:64], "big") == s and inv_n(int.from_bytes(sig[:32], "big")) == rinv
        add(f"sc_mul wrap u2=2^256-n+{u2 - NC}", dig, sig, "sc_reduce_wide's fourth fold in sc_mul(s, 1 / r)")
    # u1 = 0: every window of mul_g is zero; the digest n is the digest 0
    u2 = rs()
    dig, sig = forge(0, u2, base)
    assert dig == bytes(32)
    add("u1=0 digest 0", dig, sig, "no fixed-base addition at all", S.point_mul(u2, base))
    add("u1=0 digest n", b32(N), sig, "digest = n reduces to 0", S.point_mul(u2, base))
    # a digest >= n: e + n still fits 32 bytes when e < 2^256 - n
    e = rng.randrange(2 ** 100, 2 ** 120)
    u2 = rs()
    u1 = -e * inv_n(base[0]) % N
    dig, sig = forge(u1, u2, base)
    assert dig == b32(e) and e + N < 2 ** 256
    add("digest e+n", b32(e + N), sig, "sc_from_u256 subtracts n")
    assert out[-1][4] == pub64(S.point_add(S.point_mul(u1), S.point_mul(u2, base)))
    # Q = infinity: u1 G = -(u2 R)
    k, u2 = rs(), rs()
    dig, sig = forge(-u2 * k % N, u2, S.point_mul(k))
    add("Q infinity", dig, sig, "the last mul_g addition cancels the accumulator: ok = 0", None)
    # mul_g adds the table entry the accumulator already is: jac_add_aff's doubling path
    dig, sig = forge(1, 1, S.G)
    add("mul_g doubling G", dig, sig, "u2 R = G = table entry (0, 1)", S.point_mul(2))
    w, j = 3, 200
    R = S.point_mul(j * 256 ** w)
    assert S.point_mul(1, R) == S.point_mul(j * 256 ** w)           # u2 R is entry j of window w
    dig, sig = forge(j * 256 ** w, 1, R)
    add(f"mul_g doubling w={w} j={j}", dig, sig, "u2 R = table entry (3, 200)", S.point_mul(2 * j * 256 ** w))
    # ... and its negative: the accumulator is infinity after window 0, then window 1 adds onto infinity
    R = neg(S.G)
    assert S.point_add(S.point_mul(1, R), S.G) is None
    dig, sig = forge(1 + 5 * 256, 1, R)
    add("cancel mid-way", dig, sig, "infinity after window 0, entry (1, 5) after it", S.point_mul(5 * 256))
    # the GLV split and the signed digits at their edges
    u1 = rs()
    for u2 in GLV_EDGES:
        dig, sig = forge(u1, u2, base)
        add(f"mul_var u2={u2:#x}", dig, sig, "GLV / radix-8 digit edge")
    # the rejected signatures of the golden file, spread among the others
    bad = [(f"reject: {b['name']}", bytes.fromhex(b["digest"]), bytes.fromhex(b["sig"]), "rejected before any curve arithmetic",
            None) for b in GOLD["invalid"]]
    assert len(bad) == 7 and all(S.recover(b[1], b[2]) is None for b in bad)
    step = len(out) // len(bad)
    for k, b in enumerate(bad):
        out.insert(k * (step + 1) + step // 2, b)
    assert len({c[0] for c in out}) == len(out)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def recover_cases():
    """[(name, digest32, sig65, why)]; the expected result of each is S.recover's (recover_expected)"""
    return tuple(c[:4] for c in _recover_cases())


def recover_expected():
    """S.recover of every recover case, in order: 64 bytes or None"""
    return tuple(c[4] for c in _recover_cases())


def case(name: str):
    return [c for c in recover_cases() if c[0].startswith(name)][0]


def key_cases():
    """[(name, secret32, valid)]: the first and the last entry of every fixed-base window, the ends of the range"""
    out = []
    for w in range(32):
        out.append((f"256^{w}", b32(256 ** w), True))
        out.append((f"255*256^{w}", b32(255 * 256 ** w), True))
    assert 255 * 256 ** 31 < N
    out += [("1", b32(1), True), ("n-1", b32(N - 1), True), ("n-2", b32(N - 2), True),
            ("0", bytes(32), False), ("n", b32(N), False), ("2^256-1", b32(2 ** 256 - 1), False)]
    return out


def sign_cases():
    """(secrets, [(secret index, digest32)]): three secrets by five digests around 0, n and 2^256"""
    secrets = [b32(1), b32(N - 1), bytes.fromhex(GOLD["reference_keys"][0]["secret"])]
    digests = [bytes(32), b32(N - 1), b32(N), b32(N + 1), b32(2 ** 256 - 1)]
    return secrets, [(k, d) for k in range(len(secrets)) for d in digests]
