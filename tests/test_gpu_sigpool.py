"""Block signatures against the fixed signer set (block.go:234-254):
bh_set_validators tabulates the participants' keys, bh_verify_fixed runs Go's
ecdsa.Verify through the tables.  Integer-exact: every verdict must equal the
generic kernel's (bh_verify_signatures) and the pure-Python verify's."""
import numpy as np
import pytest

import sigpool as sp

pytestmark = pytest.mark.gpu

Q_BYTES = bytes.fromhex("FFFFFFFF00000000FFFFFFFFFFFFFFFFBCE6FAADA7179E84F3B9CAC2FC632551")


def _hg(dag, window, monkeypatch, **kw):
    from babble_amd import Hashgraph
    monkeypatch.setenv("BH_SIG_WINDOW", str(window))
    hg = Hashgraph(dag.participant_ids, 64, **kw)
    return hg


def _variants(d):
    """(name, hashes, r, s, validators) batches: the true tuples, then the
    rotated-key, flipped-hash-bit, perturbed-s and out-of-range r / s
    variants of tests/test_gpu_sha.py."""
    keys = d.creator.astype(np.int32)
    yield "true", d.hash, d.sig_r, d.sig_s, keys
    yield "rotated key", d.hash, d.sig_r, d.sig_s, (keys + 1) % d.n
    h2 = d.hash.copy()
    h2[:, 31] ^= 1
    yield "flipped hash bit", h2, d.sig_r, d.sig_s, keys
    s2 = d.sig_s.copy()
    s2[:, 31] ^= 4
    yield "perturbed s", d.hash, d.sig_r, s2, keys
    edge = np.zeros((4, 32), np.uint8)
    edge[1] = np.frombuffer(Q_BYTES, np.uint8)  # = n
    edge[2, 31] = 1
    edge[3] = 0xFF
    for e in range(4):  # r or s in {0, n, 1 (wrong), 2^256-1}
        rr = np.repeat(edge[e:e + 1], 4, 0)
        yield f"r edge {e}", d.hash[:4], rr, d.sig_s[:4], keys[:4]
        yield f"s edge {e}", d.hash[:4], d.sig_r[:4], rr, keys[:4]


def _agree(hg, d):
    pub = np.ascontiguousarray(d.pubkeys[:, 1:65])
    for name, h, r, s, v in _variants(d):
        want = hg.verify_signatures(h, r, s, v, pub)
        got = hg.verify_fixed(h, r, s, v)
        assert np.array_equal(got, want), (name, np.nonzero(got != want)[0][:10])
        assert want.all() if name == "true" else not want.any(), name


@pytest.mark.parametrize("window", [4, 8])
def test_verify_fixed_matches_generic_kernel(window, monkeypatch):
    """2000 signatures: 15 full workgroups plus a part."""
    from babble_amd.dag import Dag
    d = Dag(8, 2000, 93, sig_mode=1)
    hg = _hg(d, window, monkeypatch)
    hg.set_validators(d.pubkeys)
    info = hg.verify_ms()
    assert info["window_bits"] == window
    assert info["table_bytes"] == 9 * (256 // window) * (2 ** window - 1) * 64
    _agree(hg, d)
    assert hg.verify_fixed(d.hash[:0], d.sig_r[:0], d.sig_s[:0], np.zeros(0, np.int32)).shape == (0,)


def test_verify_fixed_wide_validator_set():
    """200 validators: slots past 128, table offsets past 2^26 bytes."""
    from babble_amd import Hashgraph
    from babble_amd.dag import Dag
    d = Dag(200, 600, 94, sig_mode=1)
    assert d.creator.max() >= 128
    hg = Hashgraph(d.participant_ids, 64)
    hg.set_validators(d.pubkeys)
    _agree(hg, d)


def _crafted(d_priv):
    """(name, u1, u2) scalar pairs for the key d_priv; the signature is
    e = u1 s, r = u2 s for a chosen s."""
    rng = np.random.default_rng(7)

    def rnd():
        return int.from_bytes(rng.bytes(32), "big") % sp.Q

    def clear(x, lo_bit, nbits):
        return x & ~(((1 << nbits) - 1) << lo_bit)

    u = rnd()
    yield "u1 = 0", 0, rnd()
    yield "u2 top window zero", rnd(), clear(rnd(), 248, 8)
    yield "u2 middle windows zero", rnd(), clear(rnd(), 120, 16)
    yield "u2 bottom window zero", rnd(), clear(rnd(), 0, 8)
    yield "both bottom halves zero", clear(rnd(), 0, 128), clear(rnd(), 0, 136)
    yield "result at infinity", (-u * d_priv) % sp.Q, u
    # u2 one table entry of Q in the top window (at either width), u1 G the
    # same point: every window of u1 is added before Q's top window, so the
    # last addition is a doubling
    top = 9 << 252
    yield "doubling inside the last addition", top * d_priv % sp.Q, top
    yield "cancellation inside the last addition", (-top * d_priv) % sp.Q, top
    yield "single window each", 0x07 << 120, 0x0B << 40
    yield "single window, u1 = 0", 0, 0xA0 << 64


@pytest.mark.parametrize("window", [4, 8])
def test_verify_fixed_crafted_scalars(window, monkeypatch):
    """Scalars chosen to reach the mixed addition's infinity, P + P and
    P + (-P) cases and the zero-window skip.  Each (u1, u2) is run with a
    random s and with the s that makes it a valid signature
    (s = x(u1 G + u2 Q) / u2), when there is one."""
    from babble_amd.dag import Dag
    d = Dag(8, 64, 95, sig_mode=1)
    keys = sp.slot_keys(d, d.seed)
    hg = _hg(d, window, monkeypatch)
    hg.set_validators(d.pubkeys)
    pub = np.ascontiguousarray(d.pubkeys[:, 1:65])
    rng = np.random.default_rng(11)
    names, H, R, S, V, want = [], [], [], [], [], []
    for slot in (0, 5):
        dp = keys[slot]
        qpt = sp.mul_g(dp)
        assert sp.pub_bytes(qpt).tobytes() == pub[slot].tobytes()
        for name, u1, u2 in _crafted(dp):
            ss = [int.from_bytes(rng.bytes(32), "big") % sp.Q or 1]
            pt = sp.add(sp.mul_g(u1), sp.mul(u2, qpt))
            if pt is not None and u2:
                ss.append(pt[0] % sp.Q * pow(u2, -1, sp.Q) % sp.Q)
            for k, s in enumerate(ss):
                e, r = u1 * s % sp.Q, u2 * s % sp.Q
                names.append((slot, name, k))
                H.append(sp.be32(e)), R.append(sp.be32(r)), S.append(sp.be32(s)), V.append(slot)
                want.append(sp.verify(qpt, e.to_bytes(32, "big"), r, s))
                if k == 1:
                    assert want[-1], (slot, name)
    H, R, S = (np.ascontiguousarray(np.stack(a)) for a in (H, R, S))
    V, want = np.asarray(V, np.int32), np.asarray(want)
    assert want.sum() >= 14 and (~want).sum() >= 14  # both verdicts are exercised
    got = hg.verify_fixed(H, R, S, V)
    gen = hg.verify_signatures(H, R, S, V, pub)
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, [names[i] for i in bad]
    assert np.array_equal(gen, want), [names[i] for i in np.nonzero(gen != want)[0]]


def test_fixed_key_lifecycle_errors():
    from babble_amd import Hashgraph
    from babble_amd.hashgraph import HashgraphError
    from babble_amd.dag import Dag
    d = Dag(8, 64, 95, sig_mode=1)
    keys = d.creator.astype(np.int32)
    hg = Hashgraph(d.participant_ids, 64)
    with pytest.raises(HashgraphError) as e:
        hg.verify_fixed(d.hash, d.sig_r, d.sig_s, keys)
    assert e.value.kind == "State"
    bad = d.pubkeys[:, 1:65].copy()
    bad[3, 63] ^= 1  # off the curve
    with pytest.raises(HashgraphError) as e:
        hg.set_validators(bad)
    assert e.value.kind == "Invalid"
    with pytest.raises(HashgraphError) as e:  # the failed call left no validators
        hg.verify_fixed(d.hash, d.sig_r, d.sig_s, keys)
    assert e.value.kind == "State"
    hg.set_validators(d.pubkeys)
    assert hg.verify_fixed(d.hash, d.sig_r, d.sig_s, keys).all()
    with pytest.raises(HashgraphError) as e:
        hg.verify_fixed(d.hash[:1], d.sig_r[:1], d.sig_s[:1], np.asarray([8], np.int32))
    assert e.value.kind == "Invalid"
    # keys survive reset_consensus (they belong to the peer set, not to a pass)
    hg.reset_consensus()
    assert hg.verify_fixed(d.hash, d.sig_r, d.sig_s, keys).all()
    # a second set_validators replaces the tables: rotated keys reject everything
    hg.set_validators(np.roll(d.pubkeys, 1, axis=0))
    assert not hg.verify_fixed(d.hash, d.sig_r, d.sig_s, keys).any()
    assert hg.verify_fixed(d.hash, d.sig_r, d.sig_s, (keys + 1) % 8).all()
    grp = Hashgraph(d.participant_ids, 64, devices=[0, 0])
    with pytest.raises(HashgraphError) as e:
        grp.set_validators(d.pubkeys)
    assert e.value.kind == "State"
    with pytest.raises(HashgraphError) as e:
        grp.verify_fixed(d.hash, d.sig_r, d.sig_s, keys)
    assert e.value.kind == "State"
