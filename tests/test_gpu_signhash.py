"""What validators sign: BlockBody.Hash() (block.go:21-46, 215-254) of the
blocks the engine cuts, with the StateHash the app's CommitBlock gives
(node.go:619-626).  Byte-exact: the sign hash is hashlib's SHA-256 of the
body JSON, and the body JSON with a StateHash is the body as cut with
"StateHash":null replaced by Go's base64 string."""
import base64
import hashlib

import numpy as np
import pytest

import sigpool as sp
from frames import kat_event_bytes
from kat import KatDag
from test_gpu_frames import _gen, _wire
from test_gpu_parity import _insert_kat

pytestmark = pytest.mark.gpu

NULL = b'"StateHash":null'


def _sha(b):
    return np.frombuffer(hashlib.sha256(b).digest(), np.uint8)


def _with_state(body, sh):
    assert body.count(NULL) == 1
    return body.replace(NULL, b'"StateHash":"' + base64.b64encode(sh) + b'"')


def _check(hg, bodies0, state, where=""):
    """Sign hashes and both JSON forms of every block against the bodies as
    cut (bodies0) and the StateHashes set so far (state: block -> bytes)."""
    sign, ok = hg.block_sign_hashes()
    assert ok.all() and len(sign) == len(bodies0)
    for b, body0 in enumerate(bodies0):
        body = _with_state(body0, state[b]) if b in state else body0
        assert hg.block_json(b, body_only=True) == body, (where, b)
        assert hg.block_json(b) == b'{"Body":' + body[:-1] + b',"Signatures":{}}\n', (where, b)
        assert np.array_equal(sign[b], _sha(body)), (where, b)


def test_sign_hashes_kat():
    from babble_amd import Hashgraph
    d = KatDag("kat_consensus")
    hg = Hashgraph(d.participant_ids, 64, frames=True)
    assert not np.asarray(_insert_kat(hg, d)).any()
    bodies, sigs = zip(*(kat_event_bytes(d, e) for e in range(len(d))))
    hg.set_event_bytes(0, bodies, sigs)
    hg.run_consensus()
    nb = hg.stats().blocks
    assert nb >= 1
    bodies0 = [hg.block_json(b, body_only=True) for b in range(nb)]
    assert all(NULL in x and x.endswith(b"}\n") for x in bodies0)
    _check(hg, bodies0, {})
    hg.set_block_state_hashes(0, [b"\x01\x02\x03"])
    _check(hg, bodies0, {0: b"\x01\x02\x03"})


@pytest.mark.parametrize("site", ["device", "host"])
def test_state_hashes_batch(monkeypatch, site):
    """n = 9, N = 6000: StateHashes of every length class (0, 1, 2, 3, 32, 64
    bytes: each base64 padding) on a range of blocks, set twice; the block
    hash as cut never changes; the blocks outside the range keep theirs."""
    monkeypatch.setenv("BH_FRAME_HASH", site)
    from babble_amd import Hashgraph
    from babble_amd.hashgraph import HashgraphError
    d, bodies, sigs = _gen(9, 6000, 82, 2)
    hg = Hashgraph(d.participant_ids, 6000, frames=True)
    assert not np.asarray(_wire(hg, d, 0, 6000)).any()
    hg.set_event_bytes(0, bodies, sigs)
    hg.run_consensus()
    nb = hg.stats().blocks
    assert nb >= 20
    bodies0 = [hg.block_json(b, body_only=True) for b in range(nb)]
    _, bh0, ok0 = hg.block_hashes()
    for b in range(nb):
        assert np.array_equal(bh0[b], _sha(hg.block_json(b)))
    _check(hg, bodies0, {}, site)
    rng = np.random.default_rng(5)
    vals = [rng.bytes(k) for k in (0, 1, 2, 3, 32, 64, 31, 33)]
    state = {3 + i: v for i, v in enumerate(vals)}
    hg.set_block_state_hashes(3, vals)
    _check(hg, bodies0, state, site)
    state.update({nb - 1: b"last", 7: b"again" * 4})
    hg.set_block_state_hashes(nb - 1, [b"last"])
    hg.set_block_state_hashes(7, [b"again" * 4])
    hg.set_block_state_hashes(5, [])
    _check(hg, bodies0, state, site)
    _, bh1, _ = hg.block_hashes()
    assert np.array_equal(bh0, bh1)  # bh_get_block_hashes: the hash as cut
    with pytest.raises(HashgraphError) as e:
        hg.set_block_state_hashes(0, [b"x" * 65])
    assert e.value.kind == "Invalid"
    with pytest.raises(HashgraphError) as e:
        hg.set_block_state_hashes(nb - 1, [b"a", b"b"])
    assert e.value.kind == "Invalid"
    _check(hg, bodies0, state, site)  # the refused calls changed nothing
    # reset_consensus cuts the blocks again: no StateHash
    hg.reset_consensus()
    hg.run_consensus()
    _check(hg, bodies0, {}, site)


def test_state_hashes_per_sync_and_check_block():
    """n = 7, N = 5000 in steps of 450 events, one lagging peer.  StateHashes
    arrive a step late; blocks cut later do not disturb them.  Then
    CheckBlock on the device: every validator signs a block's sign hash, and
    verify_fixed with that one hash repeated accepts exactly the signatures
    made over the block's current body."""
    from babble_amd import Hashgraph
    n, N, step = 7, 5000, 450
    d, bodies, sigs = _gen(n, N, 83, 1)
    hg = Hashgraph(d.participant_ids, N, frames=True)
    state, bodies0, done = {}, [], 0
    for lo in range(0, N, step):
        hi = min(N, lo + step)
        assert not np.asarray(_wire(hg, d, lo, hi)).any()
        hg.set_event_bytes(lo, bodies[lo:hi], sigs[lo:hi])
        hg.run_consensus()
        nb = hg.stats().blocks
        bodies0 += [hg.block_json(b, body_only=True) for b in range(len(bodies0), nb)]
        late = list(range(done, max(done, nb - 2)))  # all but the newest two
        if late:
            vals = [hashlib.sha256(b"state %d" % b).digest() for b in late]
            hg.set_block_state_hashes(late[0], vals)
            state.update(zip(late, vals))
            done = late[-1] + 1
    assert len(state) >= 10 and len(bodies0) > len(state)
    _check(hg, bodies0, state)
    keys = sp.slot_keys(d, d.seed)
    hg.set_validators(d.pubkeys)
    sign, _ = hg.block_sign_hashes()
    b = 4
    rs = [sp.sign(k, sign[b].tobytes()) for k in keys]
    R = np.stack([sp.be32(r) for r, _ in rs])
    S = np.stack([sp.be32(s) for _, s in rs])
    slots = np.arange(n, dtype=np.int32)
    assert hg.verify_fixed(np.repeat(sign[b:b + 1], n, 0), R, S, slots).all()
    assert not hg.verify_fixed(np.repeat(sign[b + 1:b + 2], n, 0), R, S, slots).any()
    hg.set_block_state_hashes(b, [b"another state"])
    sign2, _ = hg.block_sign_hashes(b, 1)
    assert not np.array_equal(sign2[0], sign[b])
    assert not hg.verify_fixed(np.repeat(sign2, n, 0), R, S, slots).any()


def test_sign_hash_state_errors():
    from babble_amd import Hashgraph
    from babble_amd.hashgraph import HashgraphError
    d = KatDag("kat_consensus")
    hg = Hashgraph(d.participant_ids, 64)
    for call in (lambda: hg.block_sign_hashes(0, 0), lambda: hg.set_block_state_hashes(0, [])):
        with pytest.raises(HashgraphError) as e:
            call()
        assert e.value.kind == "State"
    grp = Hashgraph(d.participant_ids, 64, devices=[0, 0], frames=True)
    with pytest.raises(HashgraphError) as e:
        grp.set_block_state_hashes(0, [])
    assert e.value.kind == "State"


def test_missing_bytes_block_has_no_sign_hash():
    """A block whose frame has an event without bytes: valid = 0 and a zero
    sign hash, a StateHash for it changes nothing, and a pooled signature
    for it stays pooled (the block is not held)."""
    from babble_amd import Hashgraph
    n, N, hole = 5, 4000, 2000
    d, bodies, sigs = _gen(n, N, 85)
    hg = Hashgraph(d.participant_ids, N, frames=True)
    assert not np.asarray(_wire(hg, d, 0, N)).any()
    hg.set_event_bytes(0, bodies[:hole], sigs[:hole])
    hg.set_event_bytes(hole + 1, bodies[hole + 1:], sigs[hole + 1:])
    hg.run_consensus()
    sign, ok = hg.block_sign_hashes()
    bad = np.nonzero(~ok)[0]
    assert len(bad) >= 1 and ok.any()
    b = int(bad[0])
    assert not sign[b].any()
    hg.set_block_state_hashes(b - 1, [b"s0", b"s1", b"s2"])
    sign2, ok2 = hg.block_sign_hashes()
    assert np.array_equal(ok2, ok) and not sign2[b].any()
    for k in (b - 1, b + 1):
        assert np.array_equal(sign2[k], _sha(hg.block_json(k, body_only=True))) and not np.array_equal(sign2[k], sign[k])
    keys = sp.slot_keys(d, d.seed)
    hg.set_validators(d.pubkeys)
    r, s = sp.sign(keys[0], bytes(32))
    hg.add_block_signatures([0], [b], sp.be32(r)[None], sp.be32(s)[None])
    assert hg.process_sig_pool() == (0, 1) and hg.sig_stats().verified == 0
