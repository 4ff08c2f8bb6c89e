"""The block-signature pool on the device (ProcessSigPool,
hashgraph.go:1236-1300; SetSignature; AnchorBlock) against the sequential
restatement in tests/sigpool.py.  Integer-exact: counts, stored (r, s), the
survivors in order and the anchor equal the model after every call."""
import hashlib

import numpy as np
import pytest

import sigpool as sp
from frames import kat_event_bytes
from kat import KatDag
from test_gpu_frames import _gen, _wire
from test_gpu_parity import _insert_kat
from test_sigpool_model import kat_scenario

pytestmark = pytest.mark.gpu


class Pair:
    """An engine handle and the model, fed the same calls."""

    def __init__(self, hg, privs, first_block=0):
        self.hg, self.privs, self.first = hg, privs, first_block
        self.pubs = [sp.mul_g(k) for k in privs]
        self.m = sp.PoolModel(self.pubs)
        hg.set_validators(np.stack([sp.pub_bytes(p) for p in self.pubs]))

    def refresh(self):
        """Store.GetBlock of the model: the engine's blocks and their current sign hashes."""
        sign, ok = self.hg.block_sign_hashes()
        assert ok.all()
        for k, h in enumerate(sign):
            self.m.set_block(self.first + k, h.tobytes())
        return len(sign)

    def add(self, entries):
        for e in entries:
            self.m.add(*e)
        if entries:
            self.hg.add_block_signatures([e[0] for e in entries], [e[1] for e in entries],
                                         np.stack([sp.be32(e[2]) for e in entries]),
                                         np.stack([sp.be32(e[3]) for e in entries]))

    def set_signature(self, block, slot, r, s):
        self.m.set_signature(block, slot, r, s)
        self.hg.set_block_signature(block, slot, sp.be32(r), sp.be32(s))

    def process(self, where=""):
        acc, rem = self.hg.process_sig_pool()
        assert acc == self.m.process(), where
        assert rem == len(self.m.pool), where
        sp.assert_state(self.hg, self.m, self.first, where)
        return acc


def _kat_handle():
    from babble_amd import Hashgraph
    d = KatDag("kat_consensus")
    hg = Hashgraph(d.participant_ids, 64, frames=True)
    assert not np.asarray(_insert_kat(hg, d)).any()
    bodies, sigs = zip(*(kat_event_bytes(d, e) for e in range(len(d))))
    hg.set_event_bytes(0, bodies, sigs)
    hg.run_consensus()
    return d, hg


def test_kat_pool():
    """TestInsertEventsWithBlockSignatures on the engine's own block 0, then
    a duplicate valid signature by one validator."""
    kat, keys = kat_scenario()
    d, hg = _kat_handle()
    assert d.n >= 3
    privs = [keys[s] if s in keys else int.from_bytes(hashlib.sha256(b"kat %d" % s).digest(), "big") % sp.Q
             for s in range(d.n)]
    p = Pair(hg, privs)
    nb = p.refresh()
    body0 = hg.block_json(0, body_only=True)
    assert sp.block_body_json(*sp.parse_block_body(body0)) == body0
    sign, _ = hg.block_sign_hashes()
    assert sign[0].tobytes() == sp.sign_hash(body0)
    hashes = {"block0": sign[0].tobytes(), "block1": sp.sign_hash(sp.block_body_json(1, 2, None, b"framehash", []))}
    assert hg.anchor_block is None
    for step in kat["steps"]:
        ent = []
        for a in step["add"]:
            r, s = sp.sign(keys[a["signer"]], hashes[a["over"]])
            ent.append((a["validator"], 0 if a["block"] == 0 else nb, r, s))  # "block 1": the first block not cut
        p.add(ent)
        assert len(hg.sig_pool()) == step["pool_before"]
        p.process(step["name"])
        assert hg.block_signature_counts()[0] == step["signatures_block0"]
        assert len(hg.sig_pool()) == step["pool_after"]
    first = hg.block_signatures(0)[1]
    r, s = sp.sign(privs[1], hashes["block0"], k=987654321)
    assert (r.to_bytes(32, "big"), s.to_bytes(32, "big")) != first
    p.add([(1, 0, r, s)])
    assert p.process("duplicate") == 1
    assert hg.block_signature_counts()[0] == 3
    assert hg.block_signatures(0)[1] == (r.to_bytes(32, "big"), s.to_bytes(32, "big"))
    st = hg.sig_stats()
    assert st.trust_count == -(-d.n // 3) and st.pool == 2 and st.accepted == 1


def _batch_round(p, nb):
    """Every validator's signature on the first dozen blocks, plus wrong-key,
    wrong-block, unknown-validator and not-yet-cut entries and one duplicate,
    shuffled; then the two anchor cases on block 12."""
    n, privs, m = len(p.privs), p.privs, p.m
    rng = np.random.default_rng(9)
    ent = []
    for b in range(12):
        h = m.blocks[b]
        for v in range(n):
            ent.append((v, b, *sp.sign(privs[v], h)))
        ent.append((b % n, b, *sp.sign(privs[(b + 1) % n], h)))          # wrong key
        ent.append(((b + 2) % n, b + 1, *sp.sign(privs[(b + 2) % n], h)))  # valid for b, sent for b + 1
        ent.append((-1, b, *sp.sign(privs[0] + 77, h)))                    # not a participant
        ent.append((b % n, nb + 5 + b, *sp.sign(privs[b % n], h)))         # not cut yet
    ent.append((4, 7, *sp.sign(privs[4], m.blocks[7], k=1234567)))        # a second valid one for (7, 4)
    order = rng.permutation(len(ent))
    p.add([ent[i] for i in order])
    acc = p.process("batch")
    assert acc == 12 * n + 1 and p.hg.anchor_block == 11
    assert p.hg.sig_stats().verified == len(ent) - 24  # every entry with a participant and a held block
    assert p.process("batch again") == 0
    assert p.hg.sig_stats().verified == 0  # nothing changed: nothing verified again
    # block 12: over trustCount by SetSignature alone -- the anchor stays
    h = m.blocks[12]
    for v in range(m.trust + 1):
        p.set_signature(12, v, *sp.sign(privs[v], h))
    sp.assert_state(p.hg, m, 0, "set_block_signature")
    assert p.process("after set_block_signature") == 0 and p.hg.anchor_block == 11
    p.add([(n - 1, 12, *sp.sign(privs[n - 1], h))])  # the next pooled valid one moves it
    assert p.process("anchor 12") == 1 and p.hg.anchor_block == 12


def test_batch_and_reset_consensus():
    """n = 9 (trustCount 3), N = 6000; then reset_consensus forgets
    signatures, anchor and pool, and a rerun reproduces the same results."""
    from babble_amd import Hashgraph
    d, bodies, sigs = _gen(9, 6000, 82, 2)
    hg = Hashgraph(d.participant_ids, 6000, frames=True)
    assert not np.asarray(_wire(hg, d, 0, 6000)).any()
    hg.set_event_bytes(0, bodies, sigs)
    hg.run_consensus()
    p = Pair(hg, sp.slot_keys(d, d.seed))
    assert p.m.trust == 3
    nb = p.refresh()
    assert nb > 20
    _batch_round(p, nb)
    counts = hg.block_signature_counts().copy()
    stored = hg.block_signatures(7)
    hg.reset_consensus()
    assert hg.anchor_block is None and hg.sig_pool() == []
    hg.run_consensus()
    assert not hg.block_signature_counts().any() and hg.block_signatures(7) == {}
    p.m.forget()
    assert p.refresh() == nb
    _batch_round(p, nb)
    assert np.array_equal(hg.block_signature_counts(), counts) and hg.block_signatures(7) == stored


def test_per_sync_schedule():
    """n = 7, N = 5000, one lagging peer, steps of 450 events.  Validators
    sign the body with its StateHash; some signatures arrive before their
    block is cut, and StateHashes are set a call late, so entries that are
    invalid become valid after set_block_state_hashes."""
    from babble_amd import Hashgraph
    n, N, step, NB, SIGNERS = 7, 5000, 450, 40, 5
    d, bodies, sigs = _gen(n, N, 83, 1)
    full = Hashgraph(d.participant_ids, N, frames=True)  # the same schedule run ahead: every block's body as cut
    for lo in range(0, N, step):
        hi = min(N, lo + step)
        assert not np.asarray(_wire(full, d, lo, hi)).any()
        full.set_event_bytes(lo, bodies[lo:hi], sigs[lo:hi])
        full.run_consensus()
    assert full.stats().blocks >= NB
    state = [hashlib.sha256(b"state %d" % b).digest() for b in range(NB)]
    body = []
    for b in range(NB):
        f = list(sp.parse_block_body(full.block_json(b, body_only=True)))
        f[2] = state[b]
        body.append(sp.block_body_json(*f))
    privs = sp.slot_keys(d, d.seed)
    hg = Hashgraph(d.participant_ids, N, frames=True)
    p = Pair(hg, privs)
    signed = stated = 0
    early = late = 0
    for lo in range(0, N, step):
        hi = min(N, lo + step)
        assert not np.asarray(_wire(hg, d, lo, hi)).any()
        hg.set_event_bytes(lo, bodies[lo:hi], sigs[lo:hi])
        hg.run_consensus()
        nb = p.refresh()
        upto = min(NB, nb + 2)  # two blocks ahead of the cut
        early += max(0, upto - max(signed, nb))
        p.add([(v, b, *sp.sign(privs[v], sp.sign_hash(body[b]))) for b in range(signed, upto) for v in range(SIGNERS)])
        signed = max(signed, upto)
        p.process(f"events {hi}")
        assert p.process(f"events {hi} again") == 0 and hg.sig_stats().verified == 0
        upto = min(NB, nb - 1)  # StateHashes: all but the newest block
        if upto > stated:
            late += sum(1 for e in p.m.pool if stated <= e[1] < upto)
            hg.set_block_state_hashes(stated, state[stated:upto])
            stated = upto
            p.refresh()
            assert p.process(f"events {hi} with StateHashes") > 0
            assert hg.block_json(stated - 1, body_only=True) == body[stated - 1]
    assert early > 0 and late > 0 and stated >= NB - 2
    assert hg.anchor_block == stated - 1 and hg.block_signature_counts()[stated - 1] == SIGNERS


def test_reset_block_and_state_errors():
    """A Reset handle (built as tests/test_gpu_reset.py builds one): the anchor
    is nil, sign hashes follow Index() - first_block, and the Reset block
    accepts signatures only after set_reset_block_sign_hash."""
    from babble_amd import Hashgraph
    from babble_amd.dag import Dag
    from babble_amd.hashgraph import HashgraphError
    from oracle_py import Oracle
    from reset import DagArrays, ResetInputs
    from test_gpu_reset import _event_bytes
    from test_gpu_reset import _wire as _wire_ids
    g = Dag(4, 3000, 0xBA0)
    d = DagArrays(g)
    bodies, sigs = _event_bytes(g)
    cap = len(d.creator) + 64
    o = Oracle(d.n, d.participant_ids, capacity=cap)
    o.insert_dag(d.creator, d.index, d.sp, d.op, d.hashes, d.sig_r, d.ntx)
    for e in range(len(d.creator)):
        o.set_event_bytes(e, bodies[e], sigs[e])
    o.run_consensus()
    rs = ResetInputs(o, d, 3)
    pid = np.asarray(d.participant_ids, np.int64)
    hg = Hashgraph(pid, cap, frames=True)
    hg.reset(rs.round_received, rs.block_index, rs.next_round, rs.sp_index, rs.sp_lt, rs.sp_round,
             rs.oth_root, rs.oth_key, pid[np.asarray(rs.oth_creator, np.int64)] if rs.oth_creator else [],
             rs.oth_index, rs.oth_lt, rs.oth_round, rs.oth_hash, self_parent_hash=rs.sp_hash)
    at = 0
    for ids in (list(rs.frame), list(rs.diff)):  # Reset's frame events, then the gossip after it
        assert not np.asarray(_wire_ids(hg, d, ids)).any()
        hg.set_event_bytes(at, [bodies[e] for e in ids], [sigs[e] for e in ids])
        hg.run_consensus()
        at += len(ids)
    first = rs.block_index + 1
    assert hg.stats().first_block == first and hg.anchor_block is None
    privs = sp.slot_keys(g, g.seed)
    p = Pair(hg, privs, first_block=first)
    nb = p.refresh()
    assert nb >= 2
    sign, _ = hg.block_sign_hashes()
    for k in range(nb):  # numbered Index() - first_block
        body = hg.block_json(k, body_only=True)
        assert sp.parse_block_body(body)[0] == first + k and sign[k].tobytes() == sp.sign_hash(body)
    hg.set_block_state_hashes(1, [b"reset state"])
    p.refresh()
    assert b'"StateHash":"' in hg.block_json(1, body_only=True)
    rh = hashlib.sha256(b"the Reset block's body").digest()
    ent = [(v, rs.block_index, *sp.sign(privs[v], rh)) for v in (0, 2, 3)]
    ent.append((1, first + 1, *sp.sign(privs[1], p.m.blocks[first + 1])))
    ent.append((3, rs.block_index - 1, *sp.sign(privs[3], rh)))  # below the Reset block: never held
    p.add(ent)
    assert p.process("before the Reset block's sign hash") == 1
    assert hg.block_signatures(rs.block_index) == {}
    hg.set_reset_block_sign_hash(np.frombuffer(rh, np.uint8))
    p.m.set_block(rs.block_index, rh)
    assert p.process("with the Reset block's sign hash") == 3
    assert hg.block_signatures(rs.block_index) == {
        v: (r.to_bytes(32, "big"), s.to_bytes(32, "big")) for v, (r, s) in p.m.sigs[rs.block_index].items()}
    assert hg.anchor_block == p.m.anchor == rs.block_index  # 3 signatures > trustCount = ceil(4 / 3) = 2
    assert len(hg.sig_pool()) == 1
    # state errors
    plain = Hashgraph(pid, 64, frames=True)
    with pytest.raises(HashgraphError) as e:
        plain.set_reset_block_sign_hash(np.zeros(32, np.uint8))
    assert e.value.kind == "State"
    with pytest.raises(HashgraphError) as e:
        plain.process_sig_pool()  # before set_validators
    assert e.value.kind == "State"
    with pytest.raises(HashgraphError) as e:
        plain.set_block_signature(0, 0, np.zeros(32, np.uint8), np.zeros(32, np.uint8))
    assert e.value.kind == "KeyNotFound"
    for bad in (Hashgraph(pid, 64), Hashgraph(pid, 64, devices=[0, 0], frames=True)):
        for call in (bad.process_sig_pool, bad.sig_pool,
                     lambda: bad.add_block_signatures([0], [0], np.zeros((1, 32), np.uint8), np.zeros((1, 32), np.uint8))):
            with pytest.raises(HashgraphError) as e:
                call()
            assert e.value.kind == "State"
