"""Fixed-key against generic ECDSA P-256 verification on the device, in one
process on the same tuples: bh_verify_signatures (k_ecdsa_verify) and
bh_verify_fixed (k_verify_fixed, 8-bit and 4-bit table windows) on the event
signatures of a sig_mode=1 DAG (n = 128, 50,000 events), device-timed with
events around the kernel (bh_get_sig_stats), warmed, the three alternating,
median of --reps runs.  bh_set_validators (the table build) is timed once per
width.  A second batch of --block-sigs tuples (default 811,776 = the 6,342
blocks of a C3 pass x 128 validators) with random digests, r and s in range
times a whole pass's worth of block signatures: a verification does the same
work whether or not it ends in a match, and random tuples touch the tables
as unrelated signatures would.  bh_process_sig_pool is timed on a pool of
--pool entries against the blocks the engine cut from the same DAG
(pool_pass).  One JSON line.
usage: python tools/bench_sigpool.py [--sigs M] [--reps R] [--block-sigs B]"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def pool_pass(a, d):
    """bh_process_sig_pool on a pool of a.pool entries against the blocks the
    engine cut from the same DAG: random r and s in range for participant
    slots and held blocks, so every entry is verified against its block's
    sign hash (the work of a valid one), none is accepted and the stable
    compaction keeps them all; a second call verifies nothing."""
    from babble_amd import Hashgraph
    bodies, bo, sigs, so = d.event_bytes()
    hg = Hashgraph(np.asarray(d.participant_ids), d.N, frames=True)
    assert not np.asarray(hg.insert_dag(d)).any()
    hg._check(hg._L.bh_set_event_bytes(hg._h, 0, d.N, bodies.ctypes.data, bo.ctypes.data, sigs.ctypes.data,
                                       so.ctypes.data))
    hg.run_consensus()
    hg.set_validators(d.pubkeys)
    nb = int(hg.stats().blocks)
    rng = np.random.default_rng(4)
    r = rng.integers(0, 256, (a.pool, 32), dtype=np.uint8)
    s = rng.integers(0, 256, (a.pool, 32), dtype=np.uint8)
    r[:, 0] &= 0x7F
    s[:, 0] &= 0x7F
    hg.add_block_signatures(np.arange(a.pool) % d.n, np.arange(a.pool) // d.n % nb, r, s)
    acc, rem = hg.process_sig_pool()
    st = hg.sig_stats()
    first = {"ms": st.process_sig_pool_ms, "verified": int(st.verified), "accepted": acc, "remaining": rem}
    hg.set_block_state_hashes(0, [b"state"] * nb)  # every body changes: everything is verified again
    ms = []
    for k in range(a.reps):
        hg.set_block_state_hashes(0, [b"state %d" % k] * nb)
        hg.process_sig_pool()
        st = hg.sig_stats()
        assert st.verified == a.pool
        ms.append(st.process_sig_pool_ms)
    hg.process_sig_pool()
    st = hg.sig_stats()
    return {"entries": a.pool, "blocks": nb, "first_call": first, "kernels_ms_median": statistics.median(ms),
            "kernels_ms_min_max": [min(ms), max(ms)], "rate_per_s": a.pool / (statistics.median(ms) * 1e-3),
            "unchanged_call": {"ms": st.process_sig_pool_ms, "verified": int(st.verified)}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=128)
    ap.add_argument("--sigs", type=int, default=50_000)
    ap.add_argument("--reps", type=int, default=12)
    ap.add_argument("--block-sigs", type=int, default=6342 * 128)
    ap.add_argument("--pool", type=int, default=50_000, help="entries of the bh_process_sig_pool run (0: skip)")
    a = ap.parse_args()
    from babble_amd import Hashgraph
    from babble_amd.dag import Dag
    d = Dag(a.n, a.sigs, 0xBABB1E03, sig_mode=1)
    pub = np.ascontiguousarray(d.pubkeys[:, 1:65])
    keys = d.creator.astype(np.int32)
    hgs, tables = {}, {}
    for w in (8, 4):
        os.environ["BH_SIG_WINDOW"] = str(w)  # read by bh_set_validators
        hg = Hashgraph(np.asarray(d.participant_ids), 64)
        hg.set_validators(d.pubkeys)
        hgs[w], tables[w] = hg, hg.verify_ms()
    os.environ.pop("BH_SIG_WINDOW")

    def generic(h, r, s, v):
        ok = hgs[8].verify_signatures(h, r, s, v, pub)
        return ok, hgs[8].verify_ms()["verify_signatures_ms"]

    def fixed(w):
        def run(h, r, s, v):
            ok = hgs[w].verify_fixed(h, r, s, v)
            return ok, hgs[w].verify_ms()["verify_fixed_ms"]
        return run

    variants = {"generic": generic, "fixed8": fixed(8), "fixed4": fixed(4)}

    def measure(h, r, s, v, reps, names):
        ms, oks = {k: [] for k in names}, {}
        for it in range(reps + 2):  # two warm-up rounds
            for k in names:
                ok, t = variants[k](h, r, s, v)
                oks[k] = ok
                if it >= 2:
                    ms[k].append(t)
        return {k: statistics.median(x) for k, x in ms.items()}, {k: [min(x), max(x)] for k, x in ms.items()}, oks

    med, spread, oks = measure(d.hash, d.sig_r, d.sig_s, keys, a.reps, ("generic", "fixed8", "fixed4"))
    assert all(o.all() for o in oks.values())
    out = {"metric": "block signatures verified/sec against the handle's validators (ECDSA P-256, kernel time)",
           "n": a.n, "signatures": a.sigs, "reps": a.reps,
           "kernel_ms": med, "kernel_ms_min_max": spread,
           "rate_per_s": {k: a.sigs / (t * 1e-3) for k, t in med.items()},
           "speedup_fixed8": med["generic"] / med["fixed8"], "speedup_fixed4": med["generic"] / med["fixed4"],
           "set_validators_ms": {str(w): tables[w]["set_validators_ms"] for w in (8, 4)},
           "table_bytes": {str(w): tables[w]["table_bytes"] for w in (8, 4)}}
    if a.block_sigs > 0:
        rng = np.random.default_rng(3)
        B = a.block_sigs
        h = rng.integers(0, 256, (B, 32), dtype=np.uint8)
        r = rng.integers(0, 256, (B, 32), dtype=np.uint8)
        s = rng.integers(0, 256, (B, 32), dtype=np.uint8)
        r[:, 0] &= 0x7F  # in [1, n - 1]
        s[:, 0] &= 0x7F
        v = (np.arange(B) % a.n).astype(np.int32)  # every validator signs every block
        bmed, bspread, boks = measure(h, r, s, v, max(3, a.reps // 4), ("generic", "fixed8", "fixed4"))
        assert np.array_equal(boks["generic"], boks["fixed8"]) and np.array_equal(boks["generic"], boks["fixed4"])
        out["block_pass"] = {"signatures": B, "kernel_ms": bmed, "kernel_ms_min_max": bspread,
                             "rate_per_s": {k: B / (t * 1e-3) for k, t in bmed.items()}}
    if a.pool > 0:
        out["process_sig_pool"] = pool_pass(a, d)
    out["value"] = out["rate_per_s"]["fixed8"]
    out["unit"] = "signatures/s"
    print(json.dumps(out))


if __name__ == "__main__":
    main()
