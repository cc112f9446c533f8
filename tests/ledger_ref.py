"""CPU reference of the importer (SPEC.md §11d), test infrastructure only and independent of the code under test: a
strict reader of the SPEC.md §7 Header, the canonical re-encoding by the msgpack package, Keccak-256 and the
recoveries by the C oracle, and verify_header + verify_seal (src/consensus/backend.rs:319-367) in Python. Also builds
sealed ledgers from an oracle run: headers by orc_encode_header over oracle_lib.run, seals signed with
tests/sig_lib.sign by a chosen voter set."""
from __future__ import annotations

import functools

import msgpack
import numpy as np

import crypto_ref as C          # first: it puts oracle/ on the path
import oracle_lib as O
import sig_lib
import trace_ref as TR
import wire_strict as WS

(OK, ABSENT, UNDECODABLE, BAD_HEIGHT, NO_PARENT, BAD_PARENT, BAD_TIME, LACK_VOTES, BAD_VOTE, BAD_PROPOSER) = range(10)
MAX_EXTRA, MAX_VOTES = 32, 256
ARRAYS = ("status", "block_hash", "voters", "n_votes", "verified_height")


_Bad, _Reader = WS.Bad, WS.Reader          # the strict MessagePack reader of SPEC.md §9's decoder grammar


def decode(b: bytes):
    """header bytes -> dict of its fields (votes: None or a list of 65-byte strings), or None when undecodable"""
    r = _Reader(bytes(b))
    try:
        d = WS.read_header(r, MAX_VOTES, MAX_EXTRA)
        r.end()
        return d
    except _Bad:
        return None


def encode(d: dict, votes="nil") -> bytes:
    """the canonical bytes of a decoded header; votes: 'nil', or 'own' for d's own votes"""
    v = None if votes == "nil" or d["votes"] is None else [list(s) for s in d["votes"]]
    return msgpack.packb([list(d["prev_hash"]), "0x" + d["proposer"].hex(), list(d["root"]), list(d["tx_hash"]),
                          list(d["receipt_hash"]), d["bloom"], d["difficulty"], d["height"], d["gas_limit"], d["gas_used"],
                          d["time"], None if d["extra"] is None else list(d["extra"]), v])


def block_hash(d: dict) -> bytes:
    return O.keccak256(encode(d, "nil"))


def seal_digest(bh: bytes) -> bytes:
    return O.keccak256(b"\x03" + bh)


def with_votes(header_nil: bytes, votes) -> bytes:
    """a canonical header ending in `votes: nil` -> the same with Some(votes)"""
    assert header_nil[-1] == 0xc0
    return header_nil[:-1] + msgpack.packb([list(v) for v in votes])


def unpack(hdr, hdr_len, slot_bytes: int):
    hdr = np.asarray(hdr, np.uint8).reshape(-1)
    return [None if int(k) > slot_bytes else bytes(hdr[i * slot_bytes:i * slot_bytes + int(k)]) for i, k in enumerate(hdr_len)]


def verify(hdr, hdr_len, slot_bytes: int, heights: int, cfg, genesis_hash: bytes) -> dict:
    """the verdict on a ledger in bftsim_export_ledger's layout, shaped as tests/ledger_lib.verify shapes it"""
    H = heights
    lens = np.asarray(hdr_len, np.uint32).reshape(-1)
    n_inst = len(lens) // H
    slots = n_inst * H
    raw = unpack(hdr, lens[:slots], slot_bytes)
    decs = [None if (b is None or len(b) == 0) else decode(b) for b in raw]
    hashes = [block_hash(d) if d is not None else bytes(32) for d in decs]
    # the recoveries, batched through the C oracle
    digs, sigs, owner = [], [], []
    for i, d in enumerate(decs):
        if d is not None and d["votes"] is not None:
            sd = seal_digest(hashes[i])
            for s in d["votes"]:
                digs.append(sd), sigs.append(s), owner.append(i)
    index = {bytes(a): v for v, a in enumerate(cfg.addresses)}
    who = []
    if digs:
        pubs, ok = O.secp_recover_batch(np.frombuffer(b"".join(digs), np.uint8).reshape(-1, 32),
                                        np.frombuffer(b"".join(sigs), np.uint8).reshape(-1, 65), threads=8)
        who = [index.get(O.keccak256(pubs[k].tobytes())[12:], -1) if ok[k] else -1 for k in range(len(digs))]
    per = [[] for _ in range(slots)]
    for k, i in enumerate(owner):
        per[i].append(who[k])
    quorum = (2 * cfg.n) // 3
    status = np.zeros(slots, np.uint8)
    voters = np.zeros((slots, 4), np.uint64)
    n_votes = np.zeros(slots, np.uint16)
    dups = 0
    for i in range(slots):
        x = i % H + 1
        d = decs[i]
        seen = set()
        for v in per[i]:
            if v >= 0:
                dups += v in seen
                seen.add(v)
        for v in seen:
            voters[i, v >> 6] |= np.uint64(1 << (v & 63))
        if d is not None and d["votes"] is not None:
            n_votes[i] = len(d["votes"])

        def st():
            if raw[i] is not None and len(raw[i]) == 0:
                return ABSENT
            if d is None:
                return UNDECODABLE
            if d["height"] == 0 or d["height"] != x:
                return BAD_HEIGHT
            if x == 1:
                phash, ptime = genesis_hash, cfg.genesis_time
            else:
                p = decs[i - 1]
                if p is None:
                    return NO_PARENT
                phash, ptime = hashes[i - 1], p["time"]
            if d["prev_hash"] != phash:
                return BAD_PARENT
            if ptime + cfg.block_period >= 1 << 64 or d["time"] < ptime + cfg.block_period:
                return BAD_TIME
            if d["votes"] is None:
                return LACK_VOTES
            if any(v < 0 for v in per[i]):
                return BAD_VOTE
            if len(seen) <= quorum:
                return LACK_VOTES
            if d["proposer"] not in index:
                return BAD_PROPOSER
            return OK
        status[i] = st()
    status = status.reshape(n_inst, H)
    vh = np.zeros(n_inst, np.uint64)
    whole = 0
    for i in range(n_inst):
        x = 0
        while x < H and status[i, x] == OK:
            x += 1
        vh[i] = x
        whole += bool((status[i, x:] == ABSENT).all())
    report = dict(headers=int((status != ABSENT).sum()), by_status=[int((status == s).sum()) for s in range(10)],
                  votes=len(digs), recoveries=len(digs), duplicate_votes=int(dups), verified_instances=whole)
    return dict(status=status, block_hash=np.frombuffer(b"".join(hashes), np.uint8).reshape(n_inst, H, 32).copy()
                if slots else np.zeros((0, H, 32), np.uint8), voters=voters.reshape(n_inst, H, 4),
                n_votes=n_votes.reshape(n_inst, H), verified_height=vh, report=report)


def assert_same(got, want):
    """got: a bftsim.ledger.Verdict or a dict of its arrays; want: verify()'s dict"""
    g = got if isinstance(got, dict) else dict({k: getattr(got, k) for k in ARRAYS}, report=got.report)
    for k in ARRAYS:
        assert np.array_equal(np.asarray(g[k]), want[k]), (k, np.asarray(g[k]).tolist()[:4], want[k].tolist()[:4])
    assert g["report"] == want["report"], (g["report"], want["report"])


# ---- sealed ledgers built from an oracle run
def keyed(cfg, seed: int):
    """(config whose validator set is derived from synthetic secrets, the secrets in validator order)"""
    from bftsim.crypto import synthetic_secrets, keyed_config
    sec = synthetic_secrets(cfg.n, seed)
    return keyed_config(cfg, sec, [O.keccak256(O.secp_pubkey(k))[12:] for k in sec])


def seal(secret: bytes, bh: bytes) -> bytes:
    return sig_lib.sign(secret, seal_digest(bh))


def build(cfg, secrets, first: int, n: int, voters):
    """-> (ledger: per instance the list of sealed header byte strings of heights 1..committed, res: the oracle's run,
    nil: the same headers with votes nil); voters(i, x) = the validator indices whose seals height x carries"""
    res = O.run(cfg, first, n)
    genesis = TR.genesis_hash(cfg)
    ledger, nil = [], []
    for i in range(n):
        prev, row, row0 = genesis, [], []
        for x in range(1, int(res["committed_height"][i]) + 1):
            h0 = C._header(cfg, first + i, x, int(res["proposer"][i, x - 1]), int(res["variant"][i, x - 1]),
                           int(res["time_tick"][i, x - 1]), prev)
            bh = O.keccak256(h0)
            assert bh == bytes(res["block_hash"][i, x - 1])
            row.append(with_votes(h0, [seal(secrets[v], bh) for v in voters(i, x)]))
            row0.append(h0)
            prev = bh
        ledger.append(row)
        nil.append(row0)
    return ledger, res, nil


@functools.lru_cache(maxsize=None)
def reference(case: str):
    """the built ledgers the CPU and the GPU tests share, each computed once per session:
    'cfg1'  N = 5, 6 heights, instance 0, sealed by the 4 running validators (the reference keys of examples/*.toml)
    'n4'    N = 4, 6 heights, instances 3..4, sealed by validators 0..2 (Q + 1 = 3)
    'n100_67' / 'n100_68'  N = 100, 2 heights, 67 / 68 seals;  'n256_170' / 'n256_171'  N = 256, 2 heights
    -> dict(cfg, secrets, first, n, ledger, res, nil, genesis)"""
    from bftsim.configs import BftConfig, cfg1
    if case == "cfg1":
        keys = TR._reference_keys()
        cfg = cfg1(True, heights=6)
        secrets, first, n, vs = [keys[a] for a in cfg.addresses], 0, 1, [0, 1, 2, 3]
    elif case == "n4":
        cfg, secrets = keyed(BftConfig(n=4, heights=6, seed=21), 7)
        first, n, vs = 3, 2, [0, 1, 2]
    elif case.startswith("n100_") or case.startswith("n256_"):
        big, k = int(case[1:4]), int(case[5:])
        cfg, secrets = keyed(BftConfig(n=big, heights=2, seed=5), 11)
        first, n, vs = 0, 1, list(range(big - k, big))           # the highest k validators: every voter word
    else:
        raise KeyError(case)
    ledger, res, nil = build(cfg, secrets, first, n, lambda i, x: vs)
    return dict(cfg=cfg, secrets=secrets, first=first, n=n, ledger=ledger, res=res, nil=nil, genesis=TR.genesis_hash(cfg),
                voters=vs)


def replace_field(header: bytes, **fields) -> bytes:
    """a decodable header re-encoded (canonically, with its own votes) after changing fields"""
    d = decode(header)
    d.update(fields)
    return encode(d, "own")


def reseal(header: bytes, secrets, voters) -> bytes:
    """the header with fresh seals of `voters` over its own block hash"""
    d = decode(header)
    bh = block_hash(d)
    return with_votes(encode(d, "nil"), [seal(secrets[v], bh) for v in voters])


def tamper_cases():
    """the tampered ledgers the CPU and the GPU tests share: [(name, reference, ledger, heights, {(i, x): status})]"""
    c1, n4 = reference("cfg1"), reference("n4")
    L, sec = c1["ledger"][0], c1["secrets"]
    h4, sec4 = n4["ledger"][0][0], n4["secrets"]
    d4 = decode(h4)
    nil4 = encode(d4, "nil")
    rs = lambda h, **f: reseal(replace_field(h, **f), sec, [0, 1, 2, 3])
    flipped = bytearray(d4["votes"][1])
    flipped[40] ^= 0x01
    outsider = seal(O.keccak256(b"not a validator"), block_hash(d4))
    swapped = list(L)
    swapped[1], swapped[2] = swapped[2], swapped[1]
    # forged seals (tests/sig_cases.py): r + n = the first x of the curve above n, recovery id 2, which recovers over
    # any digest, to a key outside the set; and one that recovers to the point at infinity over this very digest
    import sig_cases as SC
    high_x = SC.sig_of(0x5ea1 << 200, SC.high_x_points(1)[0][0])
    to_inf = SC.forge_infinity(seal_digest(block_hash(d4)), 0xfeed << 190)
    assert high_x[64] == 2 and O.secp_recover(seal_digest(block_hash(d4)), high_x) is not None
    assert to_inf[64] < 2 and O.secp_recover(seal_digest(block_hash(d4)), to_inf) is None
    out = [("absent", c1, [L[:3]], 6, {(0, 4): ABSENT}),
           ("truncated", c1, [L[:2] + [L[2][:-5]] + L[3:]], 6, {(0, 3): UNDECODABLE, (0, 4): NO_PARENT}),
           ("height", c1, [L[:2] + [rs(L[2], height=7)] + L[3:]], 6, {(0, 3): BAD_HEIGHT}),
           ("height 0", c1, [[rs(L[0], height=0)]], 6, {(0, 1): BAD_HEIGHT}),
           ("hole", c1, [L[:2] + [b""] + L[3:]], 6, {(0, 3): ABSENT, (0, 4): NO_PARENT}),
           ("parent", c1, [L[:2] + [rs(L[2], prev_hash=bytes(32))] + L[3:]], 6, {(0, 3): BAD_PARENT}),
           ("time", c1, [L[:2] + [rs(L[2], time=decode(L[1])["time"] + c1["cfg"].block_period - 1)] + L[3:]], 6,
            {(0, 3): BAD_TIME}),
           ("no votes", c1, [L[:2] + [encode(decode(L[2]), "nil")] + L[3:]], 6, {(0, 3): LACK_VOTES, (0, 4): OK}),
           ("stranger", c1, [L[:2] + [reseal(L[2], [O.keccak256(b"stranger")] * 5, [0, 1, 2, 4])] + L[3:]], 6, {(0, 3): BAD_VOTE}),
           ("proposer", c1, [L[:2] + [rs(L[2], proposer=bytes(range(20)))] + L[3:]], 6, {(0, 3): BAD_PROPOSER}),
           ("tx_hash", c1, [L[:2] + [replace_field(L[2], tx_hash=O.keccak256(b"another body"))] + L[3:]], 6,
            {(0, 2): OK, (0, 3): BAD_VOTE, (0, 4): BAD_PARENT, (0, 5): OK}),
           ("swapped", c1, [swapped], 6, {(0, 1): OK, (0, 2): BAD_HEIGHT, (0, 3): BAD_HEIGHT, (0, 4): BAD_PARENT}),
           ("Q voters", n4, [[reseal(h4, sec4, [0, 1])]], 6, {(0, 1): LACK_VOTES}),
           ("Q + 1 voters", n4, [[reseal(h4, sec4, [0, 1, 3])]], 6, {(0, 1): OK}),
           ("duplicate", n4, [[reseal(h4, sec4, [0, 1, 1])]], 6, {(0, 1): LACK_VOTES}),
           ("flipped seal", n4, [[with_votes(nil4, [d4["votes"][0], bytes(flipped), d4["votes"][2]])]], 6, {(0, 1): BAD_VOTE}),
           ("outsider", n4, [[with_votes(nil4, list(d4["votes"]) + [outsider])]], 6, {(0, 1): BAD_VOTE}),
           ("outsider alone", n4, [[with_votes(nil4, [outsider])]], 6, {(0, 1): BAD_VOTE}),
           ("unrecoverable", n4, [[with_votes(nil4, [bytes(65)] * 3)]], 6, {(0, 1): BAD_VOTE}),
           ("forged high-x seal", n4, [[with_votes(nil4, list(d4["votes"]) + [high_x])]], 6, {(0, 1): BAD_VOTE}),
           ("seal to infinity", n4, [[with_votes(nil4, list(d4["votes"]) + [to_inf])]], 6, {(0, 1): BAD_VOTE}),
           ("trailing", n4, [[h4 + b"\x00"], [with_votes(nil4, [d4["votes"][0][:64]])],
                             [nil4[:-1] + msgpack.packb([list(d4["votes"][0])] * 257)],
                             [with_votes(nil4, [d4["votes"][0]] * 256)]], 1,
            {(0, 1): UNDECODABLE, (1, 1): UNDECODABLE, (2, 1): UNDECODABLE, (3, 1): LACK_VOTES})]
    return out
