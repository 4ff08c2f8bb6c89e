"""The pure-Python ECDSA P-256 helpers of tests/sigpool.py (the expected
values of tests/test_gpu_sigpool.py) against each other, against a known
P-256 point and against the generator's keys and event signatures."""
import hashlib

import numpy as np

import sigpool as sp


def test_curve_arithmetic():
    assert sp.on_curve(sp.G)
    # 2 G (a published P-256 multiple)
    g2 = (0x7CF27B188D034F7E8A52380304B51AC3C08969E277F21B35A60B48FC47669978,
          0x07775510DB8ED040293D9AC69F7430DBBA7DADE63CE982299E04B79D227873D1)
    assert sp.mul(2, sp.G) == g2 and sp.mul_g(2) == g2 and sp.add(sp.G, sp.G) == g2
    assert sp.mul_g(sp.Q - 1) == (sp.G[0], sp.P - sp.G[1])
    assert sp.add(sp.mul_g(sp.Q - 1), sp.G) is None
    assert sp.mul(sp.Q, sp.G) is None
    for k in (1, 15, 16, 17, 2 ** 128 + 12345, sp.Q - 2):
        assert sp.mul_g(k) == sp.mul(k, sp.G), k
        assert sp.on_curve(sp.mul_g(k))


def test_sign_verify_round_trip():
    d = int.from_bytes(hashlib.sha256(b"key").digest(), "big") % sp.Q
    pub = sp.mul_g(d)
    for m in (b"", b"a", b"block 7"):
        digest = hashlib.sha256(m).digest()
        r, s = sp.sign(d, digest)
        assert sp.verify(pub, digest, r, s)
        assert not sp.verify(pub, hashlib.sha256(m + b"x").digest(), r, s)
        assert not sp.verify(pub, digest, r, (s + 1) % sp.Q)
        assert not sp.verify(sp.mul_g(d + 1), digest, r, s)
        assert not sp.verify(pub, digest, 0, s) and not sp.verify(pub, digest, r, 0)
        assert not sp.verify(pub, digest, r + sp.Q, s) and not sp.verify(pub, digest, r, s + sp.Q)


def test_generator_keys_and_signatures():
    """The private keys rebuilt from the seed give the DAG's public keys, and
    the generator's event signatures (libcrypto) verify under the helper."""
    from babble_amd.dag import Dag
    d = Dag(5, 40, 77, sig_mode=1)
    keys = sp.slot_keys(d, d.seed)
    for s in range(d.n):
        assert sp.pub_bytes(sp.mul_g(keys[s])).tobytes() == d.pubkeys[s, 1:65].tobytes()
    for e in (0, 7, 39):
        c = int(d.creator[e])
        pub = sp.mul_g(keys[c])
        r = int.from_bytes(d.sig_r[e].tobytes(), "big")
        s = int.from_bytes(d.sig_s[e].tobytes(), "big")
        assert sp.verify(pub, d.hash[e].tobytes(), r, s)
        assert not sp.verify(sp.mul_g(keys[(c + 1) % d.n]), d.hash[e].tobytes(), r, s)
    # and the other way: a helper signature has the shape the engine takes
    r, s = sp.sign(keys[2], d.hash[3].tobytes())
    assert sp.be32(r).shape == (32,) and np.array_equal(sp.be32(s), np.frombuffer(s.to_bytes(32, "big"), np.uint8))


def kat_scenario():
    """The transcribed scenario as (fixture, private keys by signer)."""
    import json
    import os
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sigpool_kat.json")) as f:
        kat = json.load(f)
    keys = {s: int.from_bytes(hashlib.sha256(b"kat signer %d" % s).digest(), "big") % sp.Q
            for s in (0, 1, 2, 666)}
    return kat, keys


def test_model_insert_events_with_block_signatures():
    """TestInsertEventsWithBlockSignatures on the sequential restatement:
    three valid signatures give 3 on the block and an empty pool, a signature
    for an unknown block stays pooled, a non-participant's never lands."""
    kat, keys = kat_scenario()
    m = sp.PoolModel([sp.mul_g(keys[s]) for s in range(kat["n"])])
    assert m.trust == 1
    hashes = {"block0": sp.sign_hash(sp.block_body_json(0, 1, None, b"framehash0", [b"tx"])),
              "block1": sp.sign_hash(sp.block_body_json(1, 2, None, b"framehash", []))}
    for b in kat["held_blocks"]:
        m.set_block(b, hashes["block%d" % b])
    for step in kat["steps"]:
        for a in step["add"]:
            r, s = sp.sign(keys[a["signer"]], hashes[a["over"]])
            m.add(a["validator"], a["block"], r, s)
        assert len(m.pool) == step["pool_before"], step["name"]
        m.process()
        assert len(m.sigs[0]) == step["signatures_block0"], step["name"]
        assert len(m.pool) == step["pool_after"], step["name"]
    assert m.anchor == 0  # 3 > trustCount
    assert [e[:2] for e in m.pool] == [(2, 1), (-1, 0)]


def test_model_duplicates_and_anchor():
    """A later valid entry for the same pair replaces the earlier one; an
    invalid entry stays; SetSignature alone does not move the anchor."""
    d = [int.from_bytes(hashlib.sha256(b"k%d" % i).digest(), "big") % sp.Q for i in range(4)]
    m = sp.PoolModel([sp.mul_g(x) for x in d])
    assert m.trust == 2
    h0, h1 = sp.sign_hash(b"a\n"), sp.sign_hash(b"b\n")
    m.set_block(0, h0)
    m.set_block(1, h1)
    s1, s2 = sp.sign(d[0], h0, k=12345), sp.sign(d[0], h0, k=54321)
    assert s1 != s2
    m.add(0, 0, *s1)
    m.add(0, 0, *s2)
    m.add(1, 0, *sp.sign(d[1], h1))  # wrong block: invalid, stays
    assert m.process() == 2 and m.sigs[0] == {0: s2} and len(m.pool) == 1 and m.anchor is None
    for v in (1, 2, 3):
        m.set_signature(1, v, *sp.sign(d[v], h1))
    assert m.anchor is None
    m.add(0, 1, *sp.sign(d[0], h1))
    m.process()
    assert m.anchor == 1 and len(m.sigs[1]) == 4


def test_block_body_json():
    body = sp.block_body_json(3, 7, None, b"\x01\x02", None)
    assert body == b'{"Index":3,"RoundReceived":7,"StateHash":null,"FrameHash":"AQI=","Transactions":null}\n'
    body = sp.block_body_json(3, 7, b"", b"\x01\x02", [b"a", b""])
    assert body == b'{"Index":3,"RoundReceived":7,"StateHash":"","FrameHash":"AQI=","Transactions":["YQ==",""]}\n'
    assert sp.block_body_json(*sp.parse_block_body(body)) == body
