"""The catalogue of hostile frames, enumerated from the decoder grammar of SPEC.md §9 (test infrastructure only).

A canonical frame is parsed, by a schema of the structs of SPEC.md §9 / §9b, into a token tree over its three nesting
levels (body, payload bytes, `msg` bytes). A case mutates one node; the inner levels are then serialised again and every
enclosing array length and the size prefix follow, so the case meets the rule it names and not a length mismatch (the
class `shape.stale` leaves the lengths alone on purpose). Every case carries its class and the verdict the grammar
gives it at the entry point of its kind (`accept`) and at the observer (`observe`; None where the observer never
accepts: Blocks and Sync frames). At every other entry point a case is rejected: each case is built from a frame of
one kind.

Base frames, signed with the validators' keys of tests/timeline_cases.py (N = 7): a Prepare, a Commit with its seal, a
RoundChange with a wide create_time; a minimal Preprepare (no extra, votes or txs) and a full one with every field at
its BFTWIRE_MAX_* (used by the limit classes only); Blocks frames of 0, 1 and 3 blocks (MAX_PER_FRAME = 3); one Sync.

Two classes are about bftwire_decode's own span limit (1028 bytes): each Subject base frame grown to exactly 1028 and to
1029 bytes by valid wide encodings. The observer accepts both.

Positions: every node that is no element of a byte array is mutated; of the elements of a byte array (the payload and
`msg` arrays included) the first, a middle and the last one. Nothing is sampled: the catalogue is the same list in the
same order on every call.

Size: 7,163 cases in 5.6 MB (`python tests/wire_mutations.py` prints the table class by class), of which 988 are
accepted at their entry point; 854 more for the bare Header (header_catalogue). The strict reference
(oracle/wire_strict.py) decodes the whole catalogue at all four entry points and at the observer in about 5 s on one
core, and building it takes about 3 s, so no position had to be cut.
"""
from __future__ import annotations

import copy
import functools

import twins_ref as TW          # first: it puts oracle/ on the path
import oracle_lib as O
import secp256k1_ref as S
import wire_ref as R
import wire_strict as WS

MAX_PER_FRAME = 3
KINDS = ("subject", "preprepare", "blocks", "sync")
CLASSES = ("base", "accept.int_wider", "accept.array_wider", "accept.address", "accept.limit_max", "accept.gossip_short",
           "accept.header_short", "accept.peer_some", "accept.span_max",
           "type.int", "type.array", "type.option", "type.address",
           "value.byte_256", "value.byte_high", "value.variant_256", "value.p2p_code", "value.msg_code",
           "shape.array_plus", "shape.array_minus", "shape.trailing", "shape.stale", "shape.prefix", "shape.array_huge",
           "shape.limit_over", "shape.address", "shape.span_over",
           "observer.unsigned", "observer.commit_unsealed", "observer.sealed")

# ---- the schema of the frames (SPEC.md §9, §9b)
U, AD = ("u",), ("addr",)
BY, H32, S65 = ("bytes", None), ("bytes", 32), ("bytes", 65)      # Vec<u8>, Hash, Signature
OPT = lambda s: ("opt", s)              # noqa: E731
ST = lambda *f: ("struct", f)           # noqa: E731
STD = lambda lo, *f: ("struct", f, lo)  # a struct with a #[serde(default)] tail: lo to len(f) elements  # noqa: E731
LS = lambda s: ("list", s)              # noqa: E731
LV = lambda s: ("level", s)             # noqa: E731
UV = ("struct", (("idx", U), ("unit", ("struct", ()))), "variant")
VIEW = ST(("round", U), ("height", U))
SUBJECT = ST(("view", VIEW), ("digest", H32))
TX = ST(("nonce", U), ("price", U), ("gas_limit", U), ("recipient", OPT(AD)), ("amount", U), ("payload", BY), ("sign", OPT(S65)))
HEADER = STD(11, ("prev_hash", H32), ("proposer", AD), ("root", H32), ("tx_hash", H32), ("receipt_hash", H32), ("bloom", U),
             ("difficulty", U), ("height", U), ("gas_limit", U), ("gas_used", U), ("time", U), ("extra", OPT(BY)),
             ("votes", OPT(LS(S65))))
BLOCK = ST(("header", HEADER), ("transactions", LS(TX)))
PREPREPARE = ST(("view", VIEW), ("proposal", BLOCK))
GOSSIP = lambda msg: STD(3, ("code", UV), ("create_time", U), ("msg", LV(msg)), ("signature", OPT(S65)), ("commit_seal", OPT(S65)))  # noqa: E731
RAW = lambda p: ST(("header", ST(("code", UV), ("ttl", U), ("create_time", U), ("peer_id", OPT(BY)))), ("payload", LV(p)))  # noqa: E731
SCHEMA = dict(subject=RAW(GOSSIP(SUBJECT)), preprepare=RAW(GOSSIP(PREPREPARE)), blocks=RAW(LS(BLOCK)), sync=RAW(U))


class N:
    """a token: kind 'int' (val: the value; role 'int', 'byte' or 'idx'), 'arr' (val: children; role 'struct', 'bytes',
    'list', 'unit' or 'variant'), 'nil', 'addr' (val: the 42 characters), 'level' (val: the root of the inner level;
    tail: bytes after it; elem: {index: bytes} elements of the byte array written otherwise). form None: the shortest.
    count: the array header's count when it is not the number of children. raw: bytes written in the node's place.
    lo: of an array whose count the schema fixes, the smallest count it allows (below the number of children only for
    the two structs with a #[serde(default)] tail); None for a list or a Vec<u8> of any length."""
    __slots__ = ("kind", "role", "name", "val", "form", "opt", "count", "raw", "tail", "elem", "lo")

    def __init__(self, kind, role, name, val, opt=False):
        self.kind, self.role, self.name, self.val, self.opt = kind, role, name, val, opt
        self.form = self.count = self.raw = None
        self.tail, self.elem, self.lo = b"", None, None

    def state(self):
        return [getattr(self, k) for k in self.__slots__]

    def restore(self, st):
        for k, v in zip(self.__slots__, st):
            setattr(self, k, v)


UINT_FORMS = ("fix", "cc", "cd", "ce", "cf")
ARR_FORMS = ("fix", "dc", "dd")


def uint_form(v: int) -> str:
    return "fix" if v < 128 else "cc" if v < 256 else "cd" if v < 65536 else "ce" if v < 1 << 32 else "cf"


def arr_form(n: int) -> str:
    return "fix" if n < 16 else "dc" if n < 65536 else "dd"


def ser_uint(v: int, form=None) -> bytes:
    form = form or uint_form(v)
    if form == "fix":
        return bytes([v])
    k = UINT_FORMS.index(form)
    return bytes([0xcb + k]) + v.to_bytes(1 << (k - 1), "big")


def ser_arr(n: int, form=None) -> bytes:
    form = form or arr_form(n)
    return bytes([0x90 | n]) if form == "fix" else b"\xdc" + n.to_bytes(2, "big") if form == "dc" else b"\xdd" + n.to_bytes(4, "big")


def ser(n: N) -> bytes:
    if n.raw is not None:
        return n.raw
    if n.kind == "int":
        return ser_uint(n.val, n.form)
    if n.kind == "nil":
        return b"\xc0"
    if n.kind == "addr":
        hdr = {None: b"\xd9" + bytes([len(n.val)]), "da": b"\xda" + len(n.val).to_bytes(2, "big"),
               "db": b"\xdb" + len(n.val).to_bytes(4, "big")}[n.form]
        return hdr + n.val
    if n.kind == "arr":
        return ser_arr(len(n.val) if n.count is None else n.count, n.form) + b"".join(ser(c) for c in n.val)
    data = ser(n.val) + n.tail
    els = [ser_uint(b) for b in data]
    for i, e in (n.elem or {}).items():
        els[i] = e
    return ser_arr(len(data) if n.count is None else n.count, n.form) + b"".join(els)


def frame_of(root: N, tail: bytes = b"", prefix_delta: int = 0) -> bytes:
    body = ser(root) + tail
    return (len(body) + prefix_delta).to_bytes(4, "big") + body


def parse(schema, r: WS.Reader, name: str, opt=False) -> N:
    """a canonical encoding -> its token tree"""
    if schema[0] == "opt":
        if r.b[r.i] == 0xc0:
            r.get()
            n = N("nil", schema[1][0], name, schema[1], opt=True)      # val: the schema of Some
            return n
        return parse(schema[1], r, name, True)
    if schema[0] == "u":
        return N("int", "int", name, r.uint(), opt)
    if schema[0] == "addr":
        assert r.get() == 0xd9 and r.get() == 42
        return N("addr", "addr", name, bytes(r.get() for _ in range(42)), opt)
    if schema[0] == "bytes":
        n = N("arr", "bytes", name, [N("int", "byte", f"{name}[{i}]", r.uint()) for i in range(r.arr())], opt)
        assert schema[1] in (None, len(n.val))
        n.lo = schema[1]
        return n
    if schema[0] == "list":
        return N("arr", "list", name, [parse(schema[1], r, f"{name}[{i}]") for i in range(r.arr())], opt)
    if schema[0] == "struct":
        assert r.arr() == len(schema[1])
        kids = [parse(s, r, f"{name}.{k}") for k, s in schema[1]]
        variant = len(schema) == 3 and schema[2] == "variant"
        if variant:
            kids[0].role = "idx"
        n = N("arr", "variant" if variant else "unit" if not schema[1] else "struct", name, kids, opt)
        n.lo = schema[2] if len(schema) == 3 and not variant else len(kids)
        return n
    assert schema[0] == "level"
    inner = WS.Reader(r.var())
    n = N("level", "level", name, parse(schema[1], inner, name + ":"), opt)
    inner.end()
    return n


def tree_of(kind: str, fr: bytes) -> N:
    r = WS.Reader(fr[4:])
    root = parse(SCHEMA[kind], r, kind)
    r.end()
    assert frame_of(root) == fr, kind
    return root


def walk(n: N, out=None) -> list:
    out = [] if out is None else out
    out.append(n)
    if n.kind == "arr":
        for c in n.val:
            walk(c, out)
    elif n.kind == "level":
        walk(n.val, out)
    return out


def find(root: N, name: str) -> N:
    return next(n for n in walk(root) if n.name == name)


def _three(k: int) -> list:
    return sorted({0, k // 2, k - 1}) if k else []


# the forbidden forms in the place of a value: each a whole MessagePack object
def forbidden(small: int = 5, content: bytes = b"\x05") -> dict:
    bn = b"\xc4" + bytes([len(content)]) + content if len(content) < 256 else b"\xc5" + len(content).to_bytes(2, "big") + content
    return {"nil": b"\xc0", "true": b"\xc3", "float32": b"\xca\x3f\x80\x00\x00", "float64": b"\xcb\x3f\xf0" + bytes(6),
            "negative fixint": b"\xff", "int8": b"\xd0" + bytes([small]), "int16": b"\xd1\x00" + bytes([small]),
            "int32": b"\xd2" + bytes(3) + bytes([small]), "int64": b"\xd3" + bytes(7) + bytes([small]), "fixstr": b"\xa1a",
            "bin8": bn, "fixmap": b"\x80", "fixext": b"\xd4\x01\x05", "0xc1": b"\xc1"}


def _bytes_node(name: str, b: bytes, opt=False) -> N:
    return N("arr", "bytes", name, [N("int", "byte", f"{name}[{i}]", x) for i, x in enumerate(b)], opt)


def _content(n: N) -> bytes:
    if n.kind == "level":
        return ser(n.val)
    if n.kind == "arr" and n.role == "bytes":
        return bytes(c.val for c in n.val)
    return b"\x05"


class _Builder:
    def __init__(self, framer=None):
        self.cases, self.framer = [], framer or frame_of

    def add(self, kind, cls, what, fr, accept, observe, base):
        assert cls in CLASSES
        if kind in ("blocks", "sync", "header"):
            observe = None
        self.cases.append(dict(kind=kind, cls=cls, name=what, frame=fr, accept=accept, observe=observe, base=base))

    def mutated(self, kind, cls, what, root, nodes, change, accept, observe, base, **fk):
        """one case: change() applied to `nodes`, the frame serialised, the nodes put back"""
        saved = [(n, n.state()) for n in nodes]
        try:
            change()
            self.add(kind, cls, what, self.framer(root, **fk), accept, observe, base)
        finally:
            for n, st in saved:
                n.restore(st)


def _signed_bases():
    """-> (cfg, secrets, [(kind, name, frame, signer)])"""
    from bftsim.configs import BftConfig
    cfg, sec = TW._keyed(BftConfig(n=7, heights=6, seed=5), 7)
    h = lambda s: O.keccak256(b"wire mutations " + s)               # noqa: E731
    out = []
    for v, (name, code, ht, rnd, dg, ct) in enumerate((("prepare", 2, 2, 1, h(b"A"), 0), ("commit", 3, 3, 0, h(b"B"), 0),
                                                        ("round change", 4, 4, 2, bytes(32), (1 << 40) + 3))):
        d = dict(code=code, create_time=ct, round=rnd, height=ht, digest=dg)
        if code == 3:
            d["commit_seal"] = S.sign(sec[v], O.keccak256(b"\x03" + dg))
        d["signature"] = S.sign(sec[v], O.keccak256(R.encode(d)[2]))
        out.append(("subject", name, R.encode(d)[0], v))
    blk = dict(prev_hash=h(b"prev"), proposer=bytes(cfg.addresses[3]), root=h(b"root"), tx_hash=h(b"tx"),
               receipt_hash=h(b"receipt"), bloom=0, difficulty=1, height=5, gas_limit=300, gas_used=70000, time=1 << 33,
               extra=None, votes=None, txs=[])
    tx = lambda k: dict(nonce=k, price=1 << 20, gas_limit=21000, amount=(1 << 64) - 1, recipient=h(b"to")[:20],     # noqa: E731
                        payload=(h(b"p") * 2)[:64], sig=(h(b"s") * 3)[:65])
    full = dict(blk, extra=h(b"extra"), votes=[(h(b"vote%d" % k) * 3)[:65] for k in range(16)], txs=[tx(0), tx(1)])
    for v, (name, b) in ((3, ("preprepare", blk)), (4, ("full preprepare", full))):
        m = dict(round=0, height=5, create_time=0, ttl=10, raw_time=0, signature=None, block=b)
        m["signature"] = S.sign(sec[v], O.keccak256(R.preprepare_frame(m)[1]))
        out.append(("preprepare", name, R.preprepare_frame(m)[0], v))
    rich = dict(blk, extra=b"abc", votes=[full["votes"][0]], txs=[dict(tx(7), recipient=None)])
    three = [dict(blk, height=6 + k, prev_hash=h(b"prev%d" % k)) for k in range(3)]
    three[1] = dict(three[1], txs=[dict(tx(1), sig=None, payload=b"")], extra=b"")
    for name, bl in (("no block", []), ("one block", [rich]), ("three blocks", three)):
        out.append(("blocks", name, R.blocks_frame(bl, 10, 1000), None))
    out.append(("sync", "sync", R.sync_frame((1 << 33) + 1, 10, 7), None))
    return cfg, sec, out


def _structure_cases(B: _Builder, kind, bname, root, base, signed_ok=True):
    """the exhaustive classes over one base frame's tree"""
    ok = signed_ok
    nodes = walk(root)
    byte_pick = set()
    for n in nodes:
        if n.kind == "arr" and n.role == "bytes":
            byte_pick |= {id(n.val[i]) for i in _three(len(n.val))}
    for n in nodes:
        at = f"{bname}: {n.name}"
        if n.kind == "int" and n.role == "byte" and id(n) not in byte_pick:
            continue
        mut = lambda cls, what, change, accept, observe=False, **fk: B.mutated(      # noqa: E731
            kind, cls, f"{at} {what}", root, [n], change, accept, observe and ok, base, **fk)
        if n.kind == "int":
            for form in UINT_FORMS[UINT_FORMS.index(uint_form(n.val)) + 1:]:
                mut("accept.int_wider", form, lambda: setattr(n, "form", form), True, True)
            for fname, raw in forbidden(n.val if n.val < 128 else 5).items():
                mut("type.int", fname, lambda: setattr(n, "raw", raw), False)
            if n.role == "byte":
                mut("value.byte_256", "256", lambda: setattr(n, "raw", b"\xcd\x01\x00"), False)
                for k, form in ((2, 0xcd), (4, 0xce), (8, 0xcf)):
                    mut("value.byte_high", hex(form), lambda: setattr(n, "raw", bytes([form, 1]) + bytes(k - 2) + bytes([n.val])), False)
            if n.role == "idx":
                mut("value.variant_256", "256", lambda: setattr(n, "val", 256), False)
                msg = n.name.count(":") == 1
                right = {"subject": (1, 2, 3), "preprepare": (0,)}[kind] if msg else (n.val,)
                for v in range(7):
                    if v != n.val and not (msg and v in right):
                        mut("value.msg_code" if msg else "value.p2p_code", str(v), lambda: setattr(n, "val", v), False)
            continue
        if n.kind in ("arr", "level"):
            size = len(n.val) if n.kind == "arr" else len(ser(n.val))
            for form in ARR_FORMS[ARR_FORMS.index(arr_form(size)) + 1:]:
                mut("accept.array_wider", form, lambda: setattr(n, "form", form), True, True)
            for fname, raw in forbidden(5, _content(n)).items():
                if not (fname == "nil" and n.opt):
                    mut("type.option" if n.opt else "type.array", fname, lambda: setattr(n, "raw", raw), False)
            def huge():
                n.form, n.count = "dd", 0xffffffff
            mut("shape.array_huge", "dd ff ff ff ff", huge, False)
            for d in (1, -1):
                if size + d >= 0:
                    mut("shape.stale", f"count {d:+d}", lambda: setattr(n, "count", size + d), False)
            if n.kind == "level":
                # its elements: the first, a middle and the last byte of the inner level, as a byte array's are
                data = ser(n.val)
                for i in _three(len(data)):
                    for form in UINT_FORMS[UINT_FORMS.index(uint_form(data[i])) + 1:]:
                        mut("accept.int_wider", f"[{i}] {form}", lambda: setattr(n, "elem", {i: ser_uint(data[i], form)}), True, True)
                    for fname, raw in forbidden(data[i] if data[i] < 128 else 5).items():
                        mut("type.int", f"[{i}] {fname}", lambda: setattr(n, "elem", {i: raw}), False)
                    mut("value.byte_256", f"[{i}] 256", lambda: setattr(n, "elem", {i: b"\xcd\x01\x00"}), False)
                    for k, form in ((2, 0xcd), (4, 0xce), (8, 0xcf)):
                        mut("value.byte_high", f"[{i}] {hex(form)}",
                            lambda: setattr(n, "elem", {i: bytes([form, 1]) + bytes(k - 2) + bytes([data[i]])}), False)
                for t in (b"\x00", b"\xc0"):
                    mut("shape.trailing", f"trailing {t.hex()} inside", lambda: setattr(n, "tail", t), False)
                mut("shape.array_minus", "one byte fewer", lambda: setattr(n, "raw", ser_arr(len(data) - 1) + b"".join(
                    ser_uint(b) for b in data[:-1])), False)
                continue
            # exact-count arrays: structs, unit arrays and the fixed byte arrays; lists and Vec<u8> of any length are
            # the limit classes' business, and the two serde-default structs may lose elements (accept.*_short)
            if n.lo is not None:
                def plus():
                    n.val = n.val + [copy.deepcopy(n.val[-1]) if n.val else N("int", "int", n.name + "[+]", 0)]
                mut("shape.array_plus", "one element more", plus, False)
                if n.lo == len(n.val) > 0:
                    mut("shape.array_minus", "one element fewer", lambda: setattr(n, "val", n.val[:-1]), False)
                elif n.lo < len(n.val):             # a serde-default tail: one fewer than the fewest it allows
                    mut("shape.array_minus", f"{n.lo - 1} elements", lambda: setattr(n, "val", n.val[:n.lo - 1]), False)
            continue
        if n.kind == "nil":
            for fname, raw in forbidden().items():
                if fname != "nil":
                    mut("type.option", fname, lambda: setattr(n, "raw", raw), False)
            continue
        assert n.kind == "addr"
        for fname, raw in forbidden().items():
            if not (fname == "nil" and n.opt):
                mut("type.address", fname, lambda: setattr(n, "raw", raw), False)
        mut("accept.address", "str16", lambda: setattr(n, "form", "da"), True, True)
        mut("accept.address", "upper-case digits", lambda: setattr(n, "val", n.val[:2] + n.val[2:].upper()), True, True)
        mut("accept.address", "0X", lambda: setattr(n, "val", b"0X" + n.val[2:]), True, True)
        mut("shape.address", "str32", lambda: setattr(n, "form", "db"), False)
        mut("shape.address", "41 characters", lambda: setattr(n, "val", n.val[:-1]), False)
        mut("shape.address", "43 characters", lambda: setattr(n, "val", n.val + b"0"), False)
        mut("shape.address", "non-hex digit", lambda: setattr(n, "val", n.val[:20] + b"g" + n.val[21:]), False)
        mut("shape.address", "space inside the digits", lambda: setattr(n, "val", n.val[:30] + b" " + n.val[31:]), False)
        mut("shape.address", "no 0x", lambda: setattr(n, "val", b"00" + n.val[2:]), False)
    at = f"{bname}: body"
    for t in (b"\x00", b"\xc0"):
        B.add(kind, "shape.trailing", f"{at} trailing {t.hex()}", B.framer(root, tail=t), False, False, base)
    if kind == "header":
        return
    for d in (1, -1):
        B.add(kind, "shape.prefix", f"{at} prefix {d:+d}", frame_of(root, prefix_delta=d), False, False, base)
    B.add(kind, "shape.stale", f"{at} one byte cut, prefix kept", frame_of(root)[:-1], False, False, base)
    B.add(kind, "shape.stale", f"{at} one byte added, prefix kept", frame_of(root) + b"\x00", False, False, base)


def _field_cases(B: _Builder, kind, bname, root, base, seal: bytes):
    """the classes about one named field of a base frame"""
    def mut(cls, what, nodes, change, accept, observe):
        B.mutated(kind, cls, f"{bname}: {what}", root, nodes, change, accept, observe, base)
    peer = find(root, f"{kind}.header.peer_id")
    for k in (0, 34, 64, 65):
        def some():
            peer.kind, peer.role, peer.val = "arr", "bytes", _bytes_node(peer.name, bytes(range(100, 100 + k)), True).val
        if k <= 64:
            mut("accept.peer_some", f"peer_id of {k} bytes", [peer], some, True, True)
        if k >= 64:
            mut("accept.limit_max" if k == 64 else "shape.limit_over", f"peer_id of {k} bytes", [peer], some, k == 64, k == 64)
    if kind in ("blocks", "sync"):
        return
    g = find(root, f"{kind}.payload:")
    code = find(root, f"{kind}.payload:.code.idx").val + 1
    for k in (3, 4):
        mut("accept.gossip_short", f"GossipMessage of {k} elements", [g], lambda: setattr(g, "val", g.val[:k]), True,
            k == 4 and code != 3)
    sig, sl = g.val[3], g.val[4]

    def to_nil(x):
        x.kind, x.val = "nil", BY
    mut("observer.unsigned", "signature nil", [sig], lambda: to_nil(sig), True, False)
    if code == 3:
        mut("observer.commit_unsealed", "commit_seal nil", [sl], lambda: to_nil(sl), True, False)
    else:
        def sealed():
            sl.kind, sl.role, sl.val = "arr", "bytes", _bytes_node(sl.name, seal, True).val
        mut("observer.sealed", "commit_seal Some", [sl], sealed, True, False)


def _span_cases(B: _Builder, kind, bname, root, base):
    """a Subject frame grown to exactly MAX_FRAME bytes, and to one more, by writing elements of its payload array in
    wider unsigned forms (each a valid encoding of the same byte): bftwire_decode takes the first and not the second;
    the observer, whose bound is 2^20, takes both"""
    pl = find(root, "subject.payload")
    data = ser(pl.val)
    for target, cls in ((WS.MAX_FRAME, "accept.span_max"), (WS.MAX_FRAME + 1, "shape.span_over")):
        left, elem = target - len(frame_of(root)), {}
        assert left > 0
        for i, b in enumerate(data):
            form = next((f for f in ("cf", "ce", "cd", "cc") if 0 < len(ser_uint(b, f)) - len(ser_uint(b)) <= left), None)
            if form:
                elem[i] = ser_uint(b, form)
                left -= len(elem[i]) - len(ser_uint(b))
        assert left == 0
        B.mutated(kind, cls, f"{bname}: {target} bytes, payload elements widened", root, [pl], lambda: setattr(pl, "elem", elem),
                  target <= WS.MAX_FRAME, True, base)
        assert len(B.cases[-1]["frame"]) == target


def _header_short(B: _Builder, kind, bname, root, base):
    for hd in [n for n in walk(root) if n.kind == "arr" and n.lo == 11 and len(n.val) == 13]:
        for k in (11, 12):
            # the observer re-encodes the decoded header: the signature stands only if the dropped fields were None
            same = all(c.kind == "nil" for c in hd.val[k:])
            B.mutated(kind, "accept.header_short", f"{bname}: {hd.name} of {k} fields", root, [hd],
                      lambda: setattr(hd, "val", hd.val[:k]), True, same, base)


def _limit_cases(B: _Builder, kind, bname, root, base):
    """the full Preprepare (every field at its limit, accepted as it is) with one limit passed at a time"""
    B.add(kind, "accept.limit_max", f"{bname}: every limit at its maximum", frame_of(root), True, True, base)
    hd = find(root, "preprepare.payload:.msg:.proposal.header")
    txs = find(root, "preprepare.payload:.msg:.proposal.transactions")
    extra, votes = hd.val[11], hd.val[12]
    assert (len(extra.val), len(votes.val), len(txs.val), len(txs.val[1].val[5].val)) == (32, 16, 2, 64)
    for what, n in (("extra of 33 bytes", extra), ("17 votes", votes), ("3 txs", txs), ("tx payload of 65 bytes", txs.val[1].val[5])):
        B.mutated(kind, "shape.limit_over", f"{bname}: {what}", root, [n],
                  lambda: setattr(n, "val", n.val + [copy.deepcopy(n.val[-1])]), False, False, base)


@functools.lru_cache(maxsize=None)
def catalogue():
    """-> dict(cfg, secrets, bases: [case index of every base frame], signer: {base index: validator}, cases: [dict(kind,
    cls, name, frame, accept, observe, base)]); a base frame is the case at its own `base` index"""
    cfg, sec, bases = _signed_bases()
    B = _Builder()
    seal = WS.decode(bases[1][2])["commit_seal"]
    base_ix, signer = [], {}
    for kind, name, fr, v in bases:
        ix = len(B.cases)
        base_ix.append(ix)
        if v is not None:
            signer[ix] = v
        B.add(kind, "base", name, fr, True, True, ix)
        root = tree_of(kind, fr)
        if name == "full preprepare":
            _limit_cases(B, kind, name, root, ix)
            continue
        _structure_cases(B, kind, name, root, ix)
        _field_cases(B, kind, name, root, ix, seal)
        _header_short(B, kind, name, root, ix)
        if kind == "subject":
            _span_cases(B, kind, name, root, ix)
        if name == "three blocks":
            blocks = find(root, "blocks.payload:")
            B.mutated(kind, "shape.limit_over", f"{name}: {MAX_PER_FRAME + 1} blocks", root, [blocks],
                      lambda: setattr(blocks, "val", blocks.val + [copy.deepcopy(blocks.val[-1])]), False, None, ix)
            B.add(kind, "accept.limit_max", f"{name}: {MAX_PER_FRAME} blocks", fr, True, None, ix)
    return dict(cfg=cfg, secrets=sec, bases=base_ix, signer=signer, cases=B.cases)


# ---- the strict reference's verdicts
ENTRY = dict(subject=lambda f: WS.decode(f), preprepare=lambda f: WS.decode_preprepare(f),
             blocks=lambda f: WS.decode_blocks(f, MAX_PER_FRAME), sync=lambda f: WS.decode_sync(f))


@functools.lru_cache(maxsize=None)
def reference():
    """the strict reference on every case, computed once per session -> dict(subject, preprepare, blocks, sync: [the
    decoded value or None per case], observe: [observe_fields' dict or None per case])"""
    cs = catalogue()["cases"]
    out = {k: [ENTRY[k](c["frame"]) for c in cs] for k in KINDS}
    out["observe"] = [WS.observe_fields(c["frame"]) for c in cs]
    return out


def by_class() -> dict:
    out = {k: 0 for k in CLASSES}
    for c in catalogue()["cases"]:
        out[c["cls"]] += 1
    return out


def self_check():
    """the catalogue against the reference alone: every class is non-empty, every case gets its declared verdict at the
    entry point of its kind and at the observer, and none at any other entry point; a base frame is canonical"""
    cat, ref = catalogue(), reference()
    counts = by_class()
    assert all(counts[k] > 0 for k in CLASSES), counts
    for i, c in enumerate(cat["cases"]):
        for k in KINDS:
            want = c["accept"] if k == c["kind"] else False
            assert (ref[k][i] is not None) == want, (i, c["cls"], c["name"], k)
        assert (ref["observe"][i] is not None) == bool(c["observe"]), (i, c["cls"], c["name"], "observe")
        assert (c["cls"].split(".")[0] in ("base", "accept", "observer")) == c["accept"], (i, c["cls"])
        assert c["base"] in cat["bases"]
    return counts


@functools.lru_cache(maxsize=None)
def header_catalogue():
    """the classes that apply to a bare Header (the importer's input, SPEC.md §11d), over the sealed header of height 1
    of ledger_ref.reference("n4") -> dict(ref: that reference, cases); `accept`: it decodes (to the same fields)"""
    import ledger_ref as LR
    ref = LR.reference("n4")
    h = ref["ledger"][0][0]
    r = WS.Reader(h)
    root = parse(HEADER, r, "header")
    r.end()
    assert ser(root) == h
    B = _Builder(lambda root, tail=b"": ser(root) + tail)
    B.add("header", "base", "sealed header", h, True, None, 0)
    _structure_cases(B, "header", "sealed header", root, 0)
    _header_short(B, "header", "sealed header", root, 0)
    return dict(ref=ref, cases=B.cases)


def commit_variants(frames) -> list:
    """five canonical Commit frames -> the same five, each in another accept-class encoding (signed as they were)"""
    assert len(frames) == 5
    out = []
    for k, fr in enumerate(frames):
        root = tree_of("subject", fr)
        g, peer = find(root, "subject.payload:"), find(root, "subject.header.peer_id")
        msg = find(root, "subject.payload:.msg")
        if k == 0:                                              # every integer outside the byte arrays as 0xcf
            for n in walk(root):
                if n.kind == "int" and n.role != "byte":
                    n.form = "cf"
        elif k == 1:                                            # every array header as array32
            for n in walk(root):
                if n.kind in ("arr", "level"):
                    n.form = "dd"
        elif k == 2:                                            # every element of digest, signature and seal as 0xcd
            for n in walk(root):
                if n.kind == "int" and n.role == "byte":
                    n.form = "cd"
        elif k == 3:                                            # peer_id Some (34 bytes), the variant indices as 0xcc
            peer.kind, peer.role, peer.val = "arr", "bytes", _bytes_node(peer.name, bytes(range(34)), True).val
            for n in walk(root):
                if n.role == "idx":
                    n.form = "cc"
        else:                                                   # the bytes of msg as 0xce, the payload array as array16
            msg.elem = {i: ser_uint(b, "ce") for i, b in enumerate(ser(msg.val))}
            find(root, "subject.payload").form = "dc"
            g.form = "dc"
        out.append(frame_of(root))
        assert out[-1] != fr and WS.decode(out[-1]) == dict(WS.decode(fr), peer_id=bytes(range(34)) if k == 3 else None)
    return out


@functools.lru_cache(maxsize=None)
def observer_stream():
    """what the observer and its continuations are given: instance 0 the whole catalogue; instance 1 the minimal
    Preprepare and five canonical Commits for its block (validators 0..4: a quorum of N = 7); instance 2 the same with
    each Commit in another accept-class encoding -> dict(cfg, stream, off, f0, heights, genesis)"""
    import accuse_ref as XR
    import audit_ref as AR
    import trace_ref as TR
    cat = catalogue()
    cfg, sec = cat["cfg"], cat["secrets"]
    pp = next(c["frame"] for c in cat["cases"] if c["cls"] == "base" and c["kind"] == "preprepare")
    p = WS.observe_parse(pp)
    commits = AR.commit_frames(sec, p["height"], p["digest"], range(5), p["round"])
    stream, off, f0 = XR.stream_of([[c["frame"] for c in cat["cases"]], [pp] + commits, [pp] + commit_variants(commits)])
    return dict(cfg=cfg, stream=stream, off=off, f0=f0, heights=6, genesis=TR.genesis_hash(cfg))


def stream_of(frames):
    import numpy as np
    off = np.zeros(len(frames) + 1, np.int64)
    off[1:] = np.cumsum([len(f) for f in frames])
    return b"".join(frames), off


if __name__ == "__main__":
    import time
    t0 = time.perf_counter()
    n = len(catalogue()["cases"])
    t1 = time.perf_counter()
    counts = self_check()
    t2 = time.perf_counter()
    for k, v in counts.items():
        print(f"{k:28s} {v}")
    print(f"{n} cases, {sum(len(c['frame']) for c in catalogue()['cases'])} bytes; built in {t1 - t0:.1f} s, "
          f"decoded and checked by the strict reference in {t2 - t1:.1f} s")
