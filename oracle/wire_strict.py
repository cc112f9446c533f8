"""wire_strict.py — the strict reference of the wire decoders, written from the grammar of SPEC.md §9 ("Decoder
grammar") and not from the C++. TEST INFRASTRUCTURE ONLY: the checker behind oracle/wire_ref.py's decode*,
tests/audit_ref.parse and tests/ledger_ref.decode, never on the product path.

Structure: every nesting level is materialised. A frame's body is read to the end, which yields the payload as a
byte string; that byte string is read by a reader of its own, which yields `msg` as a byte string; that one is read
in turn. (The decoders under test stream the three levels through nested sources instead.) Nothing here uses the
msgpack package: the accepted forms are exactly the ones spelled out below.
"""
from __future__ import annotations

P2P_BLOCK, P2P_CONSENSUS, P2P_SYNC = 3, 4, 5
MAX_FRAME = 1028                 # bftwire_decode's span limit: 4 + MAX_MSG_SIZE (codec.rs:12)
MAX_PEER, MAX_EXTRA, MAX_VOTES, MAX_TX, MAX_PAYLOAD = 64, 32, 16, 2, 64
_HEX = frozenset(b"0123456789abcdefABCDEF")


class Bad(Exception):
    pass


class Reader:
    """One nesting level: unsigned integers in any of their five forms, arrays in any of their three, nil where an
    Option stands, a str header of the three short forms for an address; every other byte in those places is Bad"""

    def __init__(self, b: bytes):
        self.b, self.i = b, 0

    def get(self) -> int:
        if self.i >= len(self.b):
            raise Bad
        self.i += 1
        return self.b[self.i - 1]

    def be(self, k: int) -> int:
        if self.i + k > len(self.b):
            raise Bad
        v = int.from_bytes(self.b[self.i:self.i + k], "big")
        self.i += k
        return v

    def uint_tag(self, t: int) -> int:
        if t < 0x80:
            return t
        if t in (0xcc, 0xcd, 0xce, 0xcf):
            return self.be(1 << (t - 0xcc))
        raise Bad

    def uint(self) -> int:
        return self.uint_tag(self.get())

    def arr_tag(self, t: int) -> int:
        if t & 0xf0 == 0x90:
            return t & 15
        if t == 0xdc:
            return self.be(2)
        if t == 0xdd:
            return self.be(4)
        raise Bad

    def arr(self) -> int:
        return self.arr_tag(self.get())

    def struct(self, n: int):
        if self.arr() != n:
            raise Bad

    def byte_list(self, n: int) -> bytes:
        out = bytearray()
        for _ in range(n):
            v = self.uint()
            if v > 255:
                raise Bad
            out.append(v)
        return bytes(out)

    def fixed(self, n: int) -> bytes:
        if self.arr() != n:
            raise Bad
        return self.byte_list(n)

    def var(self, mx: int | None = None) -> bytes:
        n = self.arr()
        if mx is not None and n > mx:
            raise Bad
        return self.byte_list(n)

    def opt(self, read):
        """Option<T>: nil, or the value as read(tag)"""
        t = self.get()
        return None if t == 0xc0 else read(t)

    def opt_fixed(self, n: int):
        def some(t):
            if self.arr_tag(t) != n:
                raise Bad
            return self.byte_list(n)
        return self.opt(some)

    def opt_var(self, mx: int):
        def some(t):
            n = self.arr_tag(t)
            if n > mx:
                raise Bad
            return self.byte_list(n)
        return self.opt(some)

    def address_tag(self, t: int) -> bytes:
        if t == 0xd9:
            n = self.be(1)
        elif t & 0xe0 == 0xa0:
            n = t & 31
        elif t == 0xda:
            n = self.be(2)
        else:
            raise Bad
        if n != 42:
            raise Bad
        s = bytes(self.get() for _ in range(42))
        if s[:1] != b"0" or s[1:2] not in (b"x", b"X") or any(c not in _HEX for c in s[2:]):
            raise Bad
        return bytes.fromhex(s[2:].decode("ascii"))

    def address(self) -> bytes:
        return self.address_tag(self.get())

    def unit_variant(self) -> int:
        self.struct(2)
        idx = self.uint()
        self.struct(0)
        if idx > 255:
            raise Bad
        return idx

    def end(self):
        if self.i != len(self.b):
            raise Bad


def read_header(r: Reader, max_votes: int = MAX_VOTES, max_extra: int = MAX_EXTRA) -> dict:
    """Header (SPEC.md §7): 11 to 13 fields, `extra` and `votes` None when absent or nil"""
    hf = r.arr()
    if not 11 <= hf <= 13:
        raise Bad
    d = dict(prev_hash=r.fixed(32), proposer=r.address(), root=r.fixed(32), tx_hash=r.fixed(32), receipt_hash=r.fixed(32))
    for k in ("bloom", "difficulty", "height", "gas_limit", "gas_used", "time"):
        d[k] = r.uint()
    d["extra"] = r.opt_var(max_extra) if hf >= 12 else None
    d["votes"] = None
    if hf >= 13:
        def some(t):
            n = r.arr_tag(t)
            if n > max_votes:
                raise Bad
            return [r.fixed(65) for _ in range(n)]
        d["votes"] = r.opt(some)
    return d


def read_tx(r: Reader) -> dict:
    r.struct(7)
    t = dict(nonce=r.uint(), price=r.uint(), gas_limit=r.uint(), recipient=r.opt(r.address_tag), amount=r.uint())
    t["payload"] = r.var(MAX_PAYLOAD)
    t["sig"] = r.opt_fixed(65)
    return t


def read_block(r: Reader) -> dict:
    r.struct(2)
    b = read_header(r)
    n = r.arr()
    if n > MAX_TX:
        raise Bad
    b["txs"] = [read_tx(r) for _ in range(n)]
    return b


def _envelope(fr: bytes, code: int):
    """frame -> (payload bytes, ttl, raw_time, peer_id): the size prefix, then the body read to its end"""
    if len(fr) < 4 or int.from_bytes(fr[:4], "big") != len(fr) - 4:
        raise Bad
    r = Reader(bytes(fr[4:]))
    r.struct(2)
    r.struct(4)
    if r.unit_variant() != code:
        raise Bad
    ttl, rtime = r.uint(), r.uint()
    peer = r.opt_var(MAX_PEER)
    payload = r.var()
    r.end()
    return payload, ttl, rtime, peer


def _gossip(payload: bytes):
    """GossipMessage bytes -> (MessageType index, create_time, msg bytes, signature, commit_seal)"""
    r = Reader(payload)
    n = r.arr()
    if not 3 <= n <= 5:
        raise Bad
    idx, ctime, msg = r.unit_variant(), r.uint(), r.var()
    sig = r.opt_fixed(65) if n >= 4 else None
    seal = r.opt_fixed(65) if n >= 5 else None
    r.end()
    return idx, ctime, msg, sig, seal


def _decode(fr: bytes):
    payload, ttl, rtime, peer = _envelope(fr, P2P_CONSENSUS)
    idx, ctime, msg, sig, seal = _gossip(payload)
    if not 1 <= idx <= 3:
        raise Bad
    r = Reader(msg)
    r.struct(2)
    r.struct(2)
    rnd, height = r.uint(), r.uint()
    digest = r.fixed(32)
    r.end()
    return dict(code=idx + 1, create_time=ctime, round=rnd, height=height, digest=digest, signature=sig, commit_seal=seal,
                ttl=ttl, raw_time=rtime, peer_id=peer)


def _decode_preprepare(fr: bytes):
    payload, ttl, rtime, _ = _envelope(fr, P2P_CONSENSUS)
    idx, ctime, msg, sig, seal = _gossip(payload)
    if idx != 0:
        raise Bad
    r = Reader(msg)
    r.struct(2)
    r.struct(2)
    rnd, height = r.uint(), r.uint()
    blk = read_block(r)
    r.end()
    return dict(round=rnd, height=height, create_time=ctime, ttl=ttl, raw_time=rtime, signature=sig, block=blk), seal


def _try(f, *a):
    try:
        return f(*a)
    except Bad:
        return None


def decode(fr: bytes):
    """frame -> the fields of a Subject-carrying Consensus frame (Prepare, Commit, RoundChange), or None; a span above
    MAX_FRAME bytes is rejected (this entry point only: the observer's bound is 2^20)"""
    return None if len(fr) > MAX_FRAME else _try(_decode, fr)


def decode_preprepare(fr: bytes):
    d = _try(_decode_preprepare, fr)
    return None if d is None else d[0]


def decode_blocks(fr: bytes, max_per_frame: int | None = None):
    """frame -> the list of its blocks, or None; more than max_per_frame blocks do not decode"""
    def go():
        payload = _envelope(fr, P2P_BLOCK)[0]
        r = Reader(payload)
        n = r.arr()
        if max_per_frame is not None and n > max_per_frame:
            raise Bad
        out = [read_block(r) for _ in range(n)]
        r.end()
        return out
    return _try(go)


def decode_sync(fr: bytes):
    def go():
        r = Reader(_envelope(fr, P2P_SYNC)[0])
        h = r.uint()
        r.end()
        return h
    return _try(go)


def observe_fields(fr: bytes):
    """the observer's reading of a frame (SPEC.md §11c row 1): a decodable Subject or Preprepare frame that is signed,
    with a seal on a Commit and on nothing else -> dict(code, create_time, round, height, digest (None for a
    Preprepare), sig, seal, block (None for a Subject frame)), else None"""
    d = _try(_decode, fr)
    if d is not None:
        if d["signature"] is None or (d["commit_seal"] is not None) != (d["code"] == 3):
            return None
        return dict(code=d["code"], create_time=d["create_time"], round=d["round"], height=d["height"], digest=d["digest"],
                    sig=d["signature"], seal=d["commit_seal"], block=None)
    p = _try(_decode_preprepare, fr)
    if p is None or p[0]["signature"] is None or p[1] is not None:
        return None
    p = p[0]
    return dict(code=1, create_time=p["create_time"], round=p["round"], height=p["height"], digest=None, sig=p["signature"],
                seal=None, block=p["block"])


def observe_parse(fr: bytes):
    """observe_fields plus what the observer derives: the canonical unsigned payload, re-encoded from the decoded
    fields by the msgpack encoders of oracle/wire_ref.py, and a Preprepare's digest (Keccak-256 of its header with
    votes nil) -> dict(code, round, height, digest, sign_payload, sig, seal, block) or None (UNDECODABLE)"""
    import msgpack
    import wire_ref as R
    f = observe_fields(fr)
    if f is None:
        return None
    if f["code"] == 1:
        from oracle_lib import keccak256
        blk = f["block"]
        pm = msgpack.packb([[f["round"], f["height"]], R.block_obj(blk)])
        sp = msgpack.packb([[0, []], f["create_time"], list(pm), None, None])
        digest = keccak256(msgpack.packb(R.header_obj(dict(blk, votes=None))))
    else:
        digest = f["digest"]
        sp = R.gossip(f["code"], f["create_time"], R.subject(f["round"], f["height"], digest), None, f["seal"])
    return dict(code=f["code"], round=f["round"], height=f["height"], digest=digest, sign_payload=sp, sig=f["sig"],
                seal=f["seal"], block=f["block"])
