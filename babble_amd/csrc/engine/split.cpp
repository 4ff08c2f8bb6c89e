// split.cpp -- the coordinate split (kernels_split.hip): shard 0 of
// a group runs the round loop, fame and order and computes no coordinates;
// shards 1 .. G-1 run the chain dataflow for a range of LA columns each
// (rank 1 also the Lamport timestamps) and ship every segment's rows of
// them to shard 0, packed as 16-bit offsets, over xGMI (peer copies in
// process, ncclSend / ncclRecv across processes)
#include <cstdlib>
#include <cstring>

#include "handle.h"
#include "sched_plan.h"

namespace {

// the LA columns of coordinate shard `rank` (>= 1) of a split group
inline void split_cols(const bh_handle *h, int32_t rank, int64_t *c0, int64_t *c1) {
  shard_range(h->d.n, h->world - 1, rank - 1, c0, c1);
}

// the split runs on the chain dataflows: n <= 128 (k_flow32 + k_round2p)
// and 128 < n <= 512 (k_floww2 on the coordinate shards; shard 0 transposes
// each segment for the 16-bit k_round_wide); every shard decides it alike
// from its (identical) host tables
bool split_active(const bh_handle *h) {
  const Dev &d = h->d;
  const bool narrow = bh::flow_eligible(d) && bh::flow32_eligible(d);
  const bool wide = !d.fd_cols && bh::floww_eligible(d) && bh::round_p16(d);
  return h->split && !h->reset_on && d.N > 0 && (narrow || wide) &&
         !(getenv("BH_SWEEP") && !strcmp(getenv("BH_SWEEP"), "chunk"));
}

}  // namespace

size_t SplitPlan::block_bytes(const bh_handle *h, int k, int32_t rank) const {
  int64_t c0, c1;
  split_cols(h, rank, &c0, &c1);
  return bh::split_layout((int)(c1 - c0), S[(size_t)k], NQ[(size_t)k], rank == 1, nullptr, nullptr);
}

bh::SplitBlock SplitPlan::block(const bh_handle *h, int k, int32_t rank, uint8_t *at) const {
  int64_t c0, c1;
  split_cols(h, rank, &c0, &c1);
  bh::SplitBlock b;
  bh::split_layout((int)(c1 - c0), S[(size_t)k], NQ[(size_t)k], rank == 1, &b, at);
  b.c0 = (int32_t)c0;
  // (test knobs, read per block: the tests switch them) BH_SPLIT_RANGE
  // lowers the 16-bit range so gossip DAGs fill the overflow slots, from
  // segment BH_SPLIT_RANGE_SEG on (0: every segment) -- a LATER segment's
  // overflow while earlier loops run
  const char *e = getenv("BH_SPLIT_RANGE");
  const char *es = getenv("BH_SPLIT_RANGE_SEG");
  b.range = e && k >= (es ? atoi(es) : 0) ? std::clamp(atoi(e), 0, 65535) : 65535;
  return b;
}

static SplitPlan split_plan(const bh_handle *h, int K, int64_t base) {
  const int n = h->d.n;
  const int64_t N = h->d.N;
  SplitPlan p;
  p.K = K;
  p.base = base;
  p.Ns.assign((size_t)K + 1, base);
  bh::segment_bounds(base, N, K, seg_ratio(h->d), p.Ns.data());
  p.tab.assign((size_t)K * 2 * n + (size_t)K * 2 * (n + 1), 0);
  p.S.assign((size_t)K, 0);
  p.NQ.assign((size_t)K, 0);
  for (int k = 0; k < K; ++k) {
    int32_t *lo = p.tab.data() + (size_t)k * 2 * n, *hi = lo + n;
    chain_lens_at(h, p.Ns[(size_t)k], lo);
    chain_lens_at(h, p.Ns[(size_t)k + 1], hi);
    int32_t *P = p.tab.data() + (size_t)K * 2 * n + (size_t)k * 2 * (n + 1), *Q = P + n + 1;
    P[0] = Q[0] = 0;
    for (int c = 0; c < n; ++c) {
      P[c + 1] = P[c] + (hi[c] - lo[c]);
      Q[c + 1] = Q[c] + (hi[c] - lo[c] + 63) / 64;
    }
    p.S[(size_t)k] = P[n];
    p.NQ[(size_t)k] = Q[n];
  }
  p.off.assign((size_t)K * h->world, 0);
  for (int k = 0; k < K; ++k)
    for (int r = 1; r < h->world; ++r) {
      p.off[(size_t)k * h->world + r] = p.total;
      p.total += p.block_bytes(h, k, r);
    }
  return p;
}

// the plan's tables on x's device (one upload), its segment events, and
// `bytes` of block buffer
int split_prepare(bh_handle *x, const SplitPlan &p, size_t bytes) {
  if (p.K > x->xseg_k) {
    if (x->xseg) (void)hipFree(x->xseg);
    x->xseg = nullptr;
    x->xseg_k = 0;
    HIPCHK(x, hipMalloc((void **)&x->xseg, p.tab.size() * 4));
    x->xseg_k = p.K;
  }
  HIPCHK(x, copy_sync(x->stream, x->xseg, p.tab.data(), p.tab.size() * 4, hipMemcpyHostToDevice));
  if (bytes > x->xcap) {
    HIPCHK(x, wait_stream(x->stream2));
    if (x->xbuf) (void)hipFree(x->xbuf);
    x->xbuf = nullptr;
    x->xcap = 0;
    const size_t cap = bytes + bytes / 4;
    HIPCHK(x, hipMalloc((void **)&x->xbuf, cap));
    x->xcap = cap;
  }
  int rc;
  if ((rc = ensure_events(x, x->seg_ev, (size_t)4 * p.K, hipEventDefault)) ||
      (rc = ensure_events(x, x->pack_ev, (size_t)p.K, hipEventDisableTiming)))
    return rc;
  if (!x->xprep) HIPCHK(x, hipEventCreateWithFlags(&x->xprep, hipEventDisableTiming));
  if (!x->stream3) {  // (the coordinate stream's priority: the loop stream keeps the higher one)
    int lo_pri = 0, hi_pri = 0;
    HIPCHK(x, hipDeviceGetStreamPriorityRange(&lo_pri, &hi_pri));
    HIPCHK(x, hipStreamCreateWithPriority(&x->stream3, hipStreamNonBlocking, lo_pri));
  }
  return BH_OK;
}

// a coordinate shard's part of the call, enqueued on its stream2: per
// segment the descriptors, k_flow32 over its columns (+ LT on rank 1) and
// the packed block (pack_ev[k]).  The narrow split all-gathers the blocks
// from the segment pipeline (every shard runs the loop); the wide split sends
// each to rank 0 here (ncclSend, or rank 0's peer copy waits for pack_ev)
static int split_coords(bh_handle *x, const SplitPlan &p) {
  Dev dv = x->d;
  int64_t c0, c1;
  split_cols(x, x->rank, &c0, &c1);
  dv.col0 = (int32_t)c0;
  dv.ncol = (int32_t)(c1 - c0);
  dv.flow_lt = x->rank == 1;
  const bool wide = !dv.fd_cols;  // 128 < n <= 512: k_floww2
  int rc;
  if ((rc = split_prepare(x, p, p.total))) return rc;
  hipStream_t sc = x->stream2;
  x->segments_used = p.K;
  if (p.base == 0) bh::launch_prep(dv, sc);
  else bh::launch_chain_scatter(dv, p.base, sc);
  HIPCHK(x, hipMemsetAsync(dv.state + bh::ST_FLOWOVF, 0, 4, sc));
  for (int k = 0; k < p.K; ++k) {
    Dev v = segment_view(x, dv, p.dview(x, k), p.Ns.data(), k);
    v.tile_list = nullptr;
    if (wide) {
      // k_floww2 over the shard's columns (its LT value as well: every
      // workgroup set carries one; only rank 1's travels)
      if (dv.ncol > 0) bh::launch_floww(v, sc);
    } else {
      bh::launch_flow_desc(v, sc);
      if (dv.ncol > 0 || dv.flow_lt) bh::launch_flow(v, sc);
    }
    uint8_t *at = x->xbuf + p.boff(x, k, x->rank);
    const bh::SplitBlock b = p.block(x, k, x->rank, at);
    bh::launch_split_pack(v, p.dpq(x, k), b, sc);
    HIPCHK(x, hipEventRecord(x->pack_ev[(size_t)k], sc));
    if (wide && x->xport && (rc = x->xport->send(x, at, p.block_bytes(x, k, x->rank), 0, sc))) return rc;
  }
  HIPCHK(x, hipGetLastError());
  // bookkeeping alike on every shard (the next call's base is rank 0's anyway)
  // valid unconditionally, while a coordinate shard of the
  // narrow split restarts its loop from r0 on incremental calls -- the fix
  // touches this call and SegmentPipeline::host_resume_round (rounds.cpp)
  commit_coords(x, dv.N, true);
  x->rows_stale = true;
  x->sweep_kernel = wide ? bh::floww_kernel(dv) : bh::flow_kernel(dv);
  return BH_OK;
}

// DivideRounds of a split group: this process's
// shards -- the whole group in process, or this rank -- each in its role.
// Rank 0 decides the call's base (its own resume state; broadcast across
// processes), so every shard cuts the same segments.  The narrow split
// (split_all): the coordinate shards' dataflow first (stream2), then every
// shard's pipeline, which all-gathers the blocks and runs the loop; the
// wide split: the same dataflow and sends, then shard 0's pipeline alone
int rounds_split_stage(bh_handle *h) {
  int rc;
  std::vector<bh_handle *> sh = local_shards(h);
  for (bh_handle *x : sh) {
    HIPCHK(x, hipSetDevice(x->device));
    x->d.N = (int64_t)x->h_creator.size();
    x->xchg_ms = 0;
    if ((rc = upload(x))) return rc;
    if ((rc = set_chain_tables(x))) return rc;
  }
  (void)hipSetDevice(h->device);
  const bool all = h->split_all();
  bh_handle *h0 = sh[0]->rank == 0 ? sh[0] : nullptr;  // the loop shard, if this process drives it
  const int64_t N = sh[0]->d.N;
  int64_t base = 0;
  if (h0) base = resume_base(h0, N);
  if (h->xport) {  // across processes: rank 0's base
    if (!h->xbase) HIPCHK(h, hipMalloc((void **)&h->xbase, 8));
    int64_t *pin = reinterpret_cast<int64_t *>(h->pinned_state + bh::ST_COUNT + 6);  // (8-B aligned pinned words)
    *pin = base;
    HIPCHK(h, hipMemcpyAsync(h->xbase, pin, 8, hipMemcpyHostToDevice, h->stream));
    if ((rc = h->xport->bcast(h, h->xbase, 8, 0, h->stream))) return rc;
    HIPCHK(h, copy_sync(h->stream, pin, h->xbase, 8, hipMemcpyDeviceToHost));
    base = *pin;
  }
  // the shards that run the loop, fame and order
  std::vector<bh_handle *> loopers;
  for (bh_handle *x : sh)
    if (all || x->rank == 0) loopers.push_back(x);
  auto on_loopers = [&](auto fn) -> int {  // (one host thread per shard in process: their host waits overlap)
    if (loopers.empty()) return BH_OK;
    if (loopers.size() == 1) {
      HIPCHK(loopers[0], hipSetDevice(loopers[0]->device));
      const int r = fn(loopers[0]);
      if (r && loopers[0] != h) h->err = "shard " + std::to_string(loopers[0]->rank) + ": " + loopers[0]->err;
      (void)hipSetDevice(h->device);
      return r;
    }
    return run_local(h, fn);
  };
  if (!split_active(sh[0])) {
    // n > 128 beyond the wide dataflow's limits, chains beyond k_flow32's,
    // a Reset hashgraph, or nothing inserted: the unsplit path on every
    // shard that runs the loop (no exchange); the others start over when
    // the split applies again
    for (bh_handle *x : sh)
      if (!all && x->rank > 0) x->inc_valid = false;
    return on_loopers([](bh_handle *x) {
      bool used = false;
      int r;
      if ((r = rounds_segmented(x, &used)) || used) return r;
      if ((r = rounds_coords(x))) return r;
      return rounds_loop(x);
    });
  }
  if (base == N) {  // nothing new to divide
    for (bh_handle *x : loopers) x->stage = std::max(x->stage, 1);
    return BH_OK;
  }
  // the wide split pipelines as well: k_floww2 runs on the coordinate
  // shards, so shard 0's loop over segment k no longer shares its compute
  // units with the dataflow of segment k + 1 (segments_for keeps the
  // unsplit wide path at one segment for that reason)
  int K = segments_for(sh[0]->d, N - base);
  if (!sh[0]->d.fd_cols && !getenv("BH_SEGMENTS")) K = N - base >= 1000000 ? 4 : 1;
  const SplitPlan plan = split_plan(sh[0], K, base);
  // the coordinate shards' dataflow first: the receives wait on it
  for (bh_handle *x : sh) {
    if (x->rank == 0) continue;
    HIPCHK(x, hipSetDevice(x->device));
    if ((rc = split_coords(x, plan))) {
      if (x != h) h->err = "shard " + std::to_string(x->rank) + ": " + x->err;
      (void)hipSetDevice(h->device);
      return rc;
    }
  }
  (void)hipSetDevice(h->device);
  const std::vector<bh_handle *> *grp = h->xport ? nullptr : &h->group;
  rc = on_loopers([&](bh_handle *x) {
    x->d.rows = x->layout_rows;
    x->d.e0 = 0;
    x->d.seg_lo = x->seg_zero;
    x->inc_calls += base > 0;
    return rounds_pipelined(x, plan.K, base, &plan, grp);
  });
  for (bh_handle *x : sh) {  // the sends / copies of this call are done
    if (x->rank == 0) continue;
    HIPCHK(x, hipSetDevice(x->device));
    HIPCHK(x, wait_stream(x->stream2));
    if (x->stream3) HIPCHK(x, wait_stream(x->stream3));
  }
  (void)hipSetDevice(h->device);
  return rc;
}
