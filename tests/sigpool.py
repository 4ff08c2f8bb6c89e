"""Test helpers for block signatures: ECDSA P-256 sign / verify in pure
Python (Go ecdsa.Verify semantics, crypto/utils.go:43-51) and the
generator's private keys (dag_gen.c:311-331)."""
import hashlib

import numpy as np

P = 0xFFFFFFFF00000001000000000000000000000000FFFFFFFFFFFFFFFFFFFFFFFF
Q = 0xFFFFFFFF00000000FFFFFFFFFFFFFFFFBCE6FAADA7179E84F3B9CAC2FC632551
B = 0x5AC635D8AA3A93E7B3EBBD55769886BC651D06B0CC53B0F63BCE3C3E27D2604B
G = (0x6B17D1F2E12C4247F8BCE6E563A440F277037D812DEB33A0F4A13945D898C296,
     0x4FE342E2FE1A7F9B8EE7EB4A7C0F9E162BCE33576B315ECECBB6406837BF51F5)


def on_curve(pt):
    x, y = pt
    return 0 <= x < P and 0 <= y < P and (y * y - (x * x * x - 3 * x + B)) % P == 0


# Jacobian points (X, Y, Z); Z == 0 is the point at infinity
def _jdbl(p):
    X, Y, Z = p
    if Z == 0 or Y == 0:
        return (1, 1, 0)
    yy = Y * Y % P
    s = 4 * X * yy % P
    m = 3 * (X - Z * Z) * (X + Z * Z) % P
    x3 = (m * m - 2 * s) % P
    return (x3, (m * (s - x3) - 8 * yy * yy) % P, 2 * Y * Z % P)


def _jadd_affine(p, a):
    """p (Jacobian) + a (affine, or None for infinity)."""
    if a is None:
        return p
    X, Y, Z = p
    if Z == 0:
        return (a[0], a[1], 1)
    zz = Z * Z % P
    u2 = a[0] * zz % P
    s2 = a[1] * zz * Z % P
    h = (u2 - X) % P
    r = (s2 - Y) % P
    if h == 0:
        return _jdbl(p) if r == 0 else (1, 1, 0)
    hh = h * h % P
    hhh = hh * h % P
    v = X * hh % P
    x3 = (r * r - hhh - 2 * v) % P
    return (x3, (r * (v - x3) - Y * hhh) % P, Z * h % P)


def _affine(p):
    X, Y, Z = p
    if Z == 0:
        return None
    zi = pow(Z, -1, P)
    return (X * zi * zi % P, Y * zi * zi * zi % P)


def mul(k, pt):
    """k * pt for an affine point (None: infinity); double-and-add."""
    k %= Q
    acc = (1, 1, 0)
    if pt is None:
        return None
    for b in range(k.bit_length() - 1, -1, -1):
        acc = _jdbl(acc)
        if (k >> b) & 1:
            acc = _jadd_affine(acc, pt)
    return _affine(acc)


def add(a, b):
    if a is None:
        return b
    return _affine(_jadd_affine((a[0], a[1], 1), b))


_GTAB = None


def _gtab():
    """d * 16^j * G for j < 64, d in [1, 15] (affine): k G is 64 mixed additions."""
    global _GTAB
    if _GTAB is None:
        tab, base = [], G
        for _ in range(64):
            row, acc = [None], (base[0], base[1], 1)
            row.append(base)
            for _d in range(2, 16):
                acc = _jadd_affine(acc, base)
                row.append(_affine(acc))
            tab.append(row)
            base = _affine(_jadd_affine((row[15][0], row[15][1], 1), base))
        _GTAB = tab
    return _GTAB


def mul_g(k):
    k %= Q
    tab, acc = _gtab(), (1, 1, 0)
    for j in range(64):
        acc = _jadd_affine(acc, tab[j][(k >> (4 * j)) & 15])
    return _affine(acc)


def sign(d, digest, k=None):
    """(r, s) of the 32-byte digest under private key d.  The nonce is
    derived from (d, digest) unless given; any nonce makes a valid signature."""
    e = int.from_bytes(digest, "big")
    ctr = 0
    while True:
        kk = k if k is not None else int.from_bytes(
            hashlib.sha256(b"nonce" + d.to_bytes(32, "big") + digest + ctr.to_bytes(4, "big")).digest(), "big") % Q
        ctr += 1
        if kk == 0:
            continue
        r = mul_g(kk)[0] % Q
        s = pow(kk, -1, Q) * (e + r * d) % Q
        if r and s:
            return r, s
        if k is not None:
            raise ValueError("nonce gives r == 0 or s == 0")


def verify(pub, digest, r, s):
    """Go ecdsa.Verify: pub an affine point, r / s integers (any size)."""
    if not (0 < r < Q and 0 < s < Q):
        return False
    e = int.from_bytes(digest, "big")
    w = pow(s, -1, Q)
    pt = add(mul_g(e * w % Q), mul(r * w % Q, pub))
    return pt is not None and pt[0] % Q == r


def generator_keys(seed, n):
    """The generator's private keys in its own key order, with their public
    points: key_i = SHA-256("babble-hip" || seed u64 LE || i i32 LE) mod q,
    0 -> 1 (dag_gen.c:311-321)."""
    out = []
    for i in range(n):
        h = hashlib.sha256(b"babble-hip" + int(seed).to_bytes(8, "little") + i.to_bytes(4, "little")).digest()
        d = int.from_bytes(h, "big") % Q or 1
        out.append((d, mul_g(d)))
    return out


def slot_keys(dag, seed):
    """Private key of each participant slot of a generated DAG, matched by
    public key (the generator sorts slots by participant ID, dag_gen.c:322-331)."""
    by_pub = {pt[0].to_bytes(32, "big") + pt[1].to_bytes(32, "big"): d for d, pt in generator_keys(seed, dag.n)}
    return [by_pub[dag.pubkeys[s, 1:65].tobytes()] for s in range(dag.n)]


def be32(x):
    return np.frombuffer(int(x).to_bytes(32, "big"), np.uint8)


def pub_bytes(pt):
    return np.frombuffer(pt[0].to_bytes(32, "big") + pt[1].to_bytes(32, "big"), np.uint8)


# ---- BlockBody.Marshal (block.go:13-29) ----
def _b64(b):
    import base64
    return base64.b64encode(b).decode()


def block_body_json(index, round_received, state_hash, frame_hash, transactions):
    """Go encoding/json of BlockBody{Index, RoundReceived, StateHash,
    FrameHash, Transactions} with the Encoder's newline; []byte as base64, a
    nil slice as null."""
    def bs(x):
        return "null" if x is None else '"' + _b64(x) + '"'
    txs = "null" if transactions is None else "[" + ",".join('"' + _b64(t) + '"' for t in transactions) + "]"
    return ('{"Index":%d,"RoundReceived":%d,"StateHash":%s,"FrameHash":%s,"Transactions":%s}\n'
            % (index, round_received, bs(state_hash), bs(frame_hash), txs)).encode()


def parse_block_body(body):
    """(index, round_received, state_hash, frame_hash, transactions) of a body's JSON."""
    import base64
    import json
    o = json.loads(body)
    dec = lambda x: None if x is None else base64.b64decode(x)  # noqa: E731
    txs = o["Transactions"]
    return (o["Index"], o["RoundReceived"], dec(o["StateHash"]), dec(o["FrameHash"]),
            None if txs is None else [base64.b64decode(t) for t in txs])


def sign_hash(body):
    return hashlib.sha256(body).digest()


# ---- ProcessSigPool / SetSignature / AnchorBlock, restated sequentially ----
class PoolModel:
    """hashgraph.go:1236-1300 line by line.  Validators are participant slots
    (-1: a key outside the participant set); blocks maps a held block's Index
    to its current sign hash (Store.GetBlock + Body.Hash())."""

    def __init__(self, pubs):
        self.pubs = list(pubs)
        self.trust = -(-len(self.pubs) // 3)  # ceil(n / 3), hashgraph.go:55
        self.blocks = {}      # Index -> sign hash (32 bytes)
        self.sigs = {}        # Index -> {slot: (r, s)}
        self.pool = []        # [(slot, Index, r, s)]
        self.anchor = None
        self._memo = {}

    def set_block(self, index, shash):
        self.blocks[index] = bytes(shash)
        self.sigs.setdefault(index, {})

    def add(self, slot, index, r, s):  # InsertEvent, hashgraph.go:758
        self.pool.append((slot, index, r, s))

    def set_signature(self, index, slot, r, s):  # Block.SetSignature
        self.sigs[index][slot] = (r, s)

    def _verify(self, slot, shash, r, s):
        k = (slot, shash, r, s)
        if k not in self._memo:
            self._memo[k] = verify(self.pubs[slot], shash, r, s)
        return self._memo[k]

    def process(self):
        processed = set()
        for i, (slot, index, r, s) in enumerate(self.pool):
            if slot < 0:                      # unknown validator
                continue
            if index not in self.blocks:      # Store.GetBlock fails
                continue
            if not self._verify(slot, self.blocks[index], r, s):
                continue
            self.set_signature(index, slot, r, s)
            if len(self.sigs[index]) > self.trust and (self.anchor is None or index > self.anchor):
                self.anchor = index
            processed.add(i)
        self.pool = [e for i, e in enumerate(self.pool) if i not in processed]
        return len(processed)

    def forget(self):  # bh_reset_consensus
        self.blocks, self.sigs, self.pool, self.anchor = {}, {}, [], None


def pool_as_bytes(pool):
    return [(v, b, int(r).to_bytes(32, "big"), int(s).to_bytes(32, "big")) for v, b, r, s in pool]


def assert_state(hg, model, first_block=0, where=""):
    """Counts, stored (r, s), survivors in order and anchor of the engine against the model."""
    assert hg.sig_pool() == pool_as_bytes(model.pool), where
    assert hg.anchor_block == model.anchor, (where, hg.anchor_block, model.anchor)
    counts = hg.block_signature_counts()
    for k, c in enumerate(counts):
        b = first_block + k
        want = model.sigs.get(b, {})
        assert c == len(want), (where, b, c, len(want))
        got = hg.block_signatures(b)
        assert got == {v: (r.to_bytes(32, "big"), s.to_bytes(32, "big")) for v, (r, s) in want.items()}, (where, b)
