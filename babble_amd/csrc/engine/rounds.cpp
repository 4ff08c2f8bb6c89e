// rounds.cpp -- host scheduling of DivideRounds: chain tables, coordinates,
// the round loop and the segment pipeline (stage_rounds is api.cpp's entry).
#include <cstdlib>
#include <cstring>

#include "handle.h"
#include "sched_plan.h"

// Chain-major layout: chain c's events occupy rows [chain_start[c],
// chain_start[c] + len_c) of a region of cap_c rows.  The regions are kept
// while every chain fits (appended events extend a region in place, so the
// rows already computed stay valid); when one outgrows its region they are
// laid out again with fresh slack (max(BH_LAYOUT_SLACK or 1024, len / 8)
// rows each, if the allocation has room; none otherwise) and layout_changed
// is set.  Rows past a chain's events are gaps (chain_ids -1).
int set_chain_tables(bh_handle *h, bool wait) {
  const int n = h->d.n;
  std::vector<int32_t> len((size_t)n);
  int32_t mx = 0;
  for (int c = 0; c < n; ++c) {
    len[(size_t)c] = (int32_t)h->chain[(size_t)c].size();
    mx = std::max(mx, len[(size_t)c]);
  }
  bool fits = (int)h->cap_h.size() == n;
  for (int c = 0; fits && c < n; ++c) fits = len[(size_t)c] <= h->cap_h[(size_t)c];
  h->layout_changed = !fits;
  if (!fits) {
    h->rows_built = false;  // (rows built for the old layout)
    const int64_t min_slack = getenv("BH_LAYOUT_SLACK") ? atoll(getenv("BH_LAYOUT_SLACK")) : 1024;
    const bool slack = h->d.la_rows > h->cap;  // the allocation reserved room for it
    int64_t need = 0;
    for (int c = 0; c < n; ++c) need += len[(size_t)c] + std::max<int64_t>(min_slack, len[(size_t)c] / 8);
    const bool use = slack && need <= h->d.la_rows;
    h->cap_h.resize((size_t)n);
    h->cstart_h.resize((size_t)n);
    int64_t acc = 0;
    for (int c = 0; c < n; ++c) {
      h->cstart_h[(size_t)c] = (int32_t)acc;
      h->cap_h[(size_t)c] = (int32_t)(len[(size_t)c] + (use ? std::max<int64_t>(min_slack, len[(size_t)c] / 8) : 0));
      acc += h->cap_h[(size_t)c];
    }
    h->layout_rows = acc;
    HIPCHK(h, hipMemcpyAsync(h->d.chain_start, h->cstart_h.data(), n * 4, hipMemcpyHostToDevice, h->stream));
  }
  h->d.max_chain_len = mx;
  h->lens_h = len;
  HIPCHK(h, hipMemcpyAsync(h->d.chain_len, h->lens_h.data(), n * 4, hipMemcpyHostToDevice, h->stream));
  // (!wait: the caller orders every later reader after h->stream -- the
  // segment pipeline's coordinate stream waits for an event recorded on it
  // -- and lens_h / cstart_h change only in the next call, after its
  // stages' synchronisations)
  if (wait) HIPCHK(h, wait_stream(h->stream));
  return BH_OK;
}

// the round loop's iterations as one graph of `iters` (even) launches for
// the view v, cached per slot (kernel arguments are captured by value)
static int build_graph(bh_handle *h, const Dev &v, hipGraphExec_t *graph, Dev *graph_dev, int iters) {
  if (*graph && memcmp(graph_dev, &v, sizeof(Dev)) == 0) return BH_OK;
  if (*graph) {
    (void)hipGraphExecDestroy(*graph);
    *graph = nullptr;
  }
  hipGraph_t g;
  HIPCHK(h, hipStreamBeginCapture(h->stream, hipStreamCaptureModeThreadLocal));
  for (int i = 0; i < iters; ++i) bh::launch_round_iteration(v, i & 1, h->stream);
  HIPCHK(h, hipStreamEndCapture(h->stream, &g));
  HIPCHK(h, hipGraphInstantiate(graph, g, nullptr, nullptr, 0));
  (void)hipGraphDestroy(g);
  *graph_dev = v;
  return BH_OK;
}

// the round loop on h->stream for view v, its inputs set up already:
// replays batches of iterations, checking completion one batch behind so
// the device never idles on the host round trip.  The first two batches
// are ITER_FIRST iterations (graph_s), the rest ITER_BATCH: a loop that ends
// within a few rounds -- an incremental call's -- runs 8 launches rather
// than 64, most of them no-ops behind the done flag.  Returns the loop state.
static int run_round_loop(bh_handle *h, const Dev &v, hipGraphExec_t *graph, Dev *graph_dev, hipGraphExec_t *graph_s,
                   Dev *graph_dev_s, int32_t *st) {
  int rc;
  hipStream_t s = h->stream;
  // BH_NO_GRAPH=1: launch the iterations directly instead of replaying a
  // captured graph (profiling / A-B; results are identical)
  const bool no_graph = getenv("BH_NO_GRAPH") && atoi(getenv("BH_NO_GRAPH"));
  const bool loop_timing = !(getenv("BH_LOOP_TIMING") && !atoi(getenv("BH_LOOP_TIMING")));
  if (bh::round_solo_eligible(v)) {  // one launch runs every round (k_round_solo)
    if (loop_timing) HIPCHK(h, hipEventRecord(h->ev_loop[0], s));
    bh::launch_round_solo(v, s);
    HIPCHK(h, hipGetLastError());
    if (loop_timing) HIPCHK(h, hipEventRecord(h->ev_loop[1], s));
    HIPCHK(h, copy_sync(s, st, v.state, bh::ST_COUNT * 4, hipMemcpyDeviceToHost));
    float lms = 0;
    if (loop_timing && hipEventElapsedTime(&lms, h->ev_loop[0], h->ev_loop[1]) == hipSuccess) h->loop_ms_acc += lms;
    if (!st[bh::ST_DONE]) return h->fail(BH_ERR_STATE, "round loop did not terminate");
    if (st[bh::ST_ERR]) return h->fail(BH_ERR_CAPACITY, "round table capacity exceeded");
    return BH_OK;
  }
  const bool pers = bh::round_persist_eligible(v), wpers = !pers && bh::round_wide_persist_eligible(v);
  if (pers || wpers) {  // one launch, a grid barrier per iteration (k_round2p / k_round_wide<..., true>)
    // the loop's inputs, kept: a barrier that gives up (ST_ERR = 3) leaves
    // them overwritten, and the per-iteration launches below start again
    // from them -- parity 0's boundaries and candidate rows (candfd, which
    // the wide loop's cand16 aliases; cand8 and its tags), the state block
    const int n = v.n;
    const size_t w8 = v.cand8 ? (size_t)n * ((v.npad + 15) / 16 * 16) : 0;
    struct Piece { void *dev; size_t bytes; } pieces[] = {
        {v.Bp, (size_t)n * 4}, {v.candfd, (size_t)n * v.npad * 4}, {v.state, bh::ST_COUNT * 4},
        {v.cand8, wpers ? w8 : 0}, {v.c8tag, wpers && v.c8tag ? (size_t)n * 4 : 0}};
    auto snapshot = [&](bool restore) -> int {
      char *sp = reinterpret_cast<char *>(v.psnap);
      for (const Piece &pc : pieces) {
        if (!pc.bytes) continue;
        HIPCHK(h, hipMemcpyAsync(restore ? pc.dev : sp, restore ? sp : pc.dev, pc.bytes, hipMemcpyDeviceToDevice, s));
        sp += (pc.bytes + 15) & ~(size_t)15;
      }
      return BH_OK;
    };
    if ((rc = snapshot(false))) return rc;
    if (loop_timing) HIPCHK(h, hipEventRecord(h->ev_loop[0], s));
    ++h->persist_loops;
    if (pers) bh::launch_round_persist(v, s);
    else bh::launch_round_wide_persist(v, s);
    HIPCHK(h, hipGetLastError());
    if (loop_timing) HIPCHK(h, hipEventRecord(h->ev_loop[1], s));
    HIPCHK(h, copy_sync(s, st, v.state, bh::ST_COUNT * 4, hipMemcpyDeviceToHost));
    float lms = 0;
    if (loop_timing && hipEventElapsedTime(&lms, h->ev_loop[0], h->ev_loop[1]) == hipSuccess) h->loop_ms_acc += lms;
    if (st[bh::ST_DONE] && st[bh::ST_ERR] != 3) {
      if (st[bh::ST_ERR]) return h->fail(BH_ERR_CAPACITY, "round table capacity exceeded");
      return BH_OK;
    }
    // the grid barrier gave up (some workgroup was never placed): restore and
    // take the per-iteration launches (counted in stats.persist_fallbacks)
    ++h->persist_fallbacks;
    if ((rc = snapshot(true))) return rc;
    if (pers && bh::cand_fe(v)) bh::launch_cand_defe(v, s);  // (k_round2 reads plain entries)
  }
  if (!no_graph && (rc = build_graph(h, v, graph, graph_dev, ITER_BATCH))) return rc;
  if (!no_graph && (rc = build_graph(h, v, graph_s, graph_dev_s, ITER_FIRST))) return rc;
  hipEvent_t done_ev[2];
  HIPCHK(h, hipEventCreateWithFlags(&done_ev[0], hipEventDisableTiming));
  HIPCHK(h, hipEventCreateWithFlags(&done_ev[1], hipEventDisableTiming));
  // the round kernels store 1 into the mapped word pin[0] when the loop ends
  volatile int32_t *pin = h->pinned_state;
  pin[0] = 0;
  bool done = false;
  // the loop's own device time (bh_get_stage_ms entry 7; BH_LOOP_TIMING=0: off, A/B)
  if (loop_timing) HIPCHK(h, hipEventRecord(h->ev_loop[0], s));  // (after any wait queued on s: loop time only)
  const int64_t max_batches = (int64_t)v.R_cap / ITER_BATCH + 4;
  for (int64_t b = 0; b < max_batches && !done; ++b) {
    const bool first = b < 2;
    if (no_graph) {
      for (int i = 0; i < (first ? ITER_FIRST : ITER_BATCH); ++i) bh::launch_round_iteration(v, i & 1, s);
      HIPCHK(h, hipGetLastError());
    } else {
      HIPCHK(h, hipGraphLaunch(first ? *graph_s : *graph, s));
    }
    HIPCHK(h, hipEventRecord(done_ev[b & 1], s));
    if (b > 0) {
      HIPCHK(h, hipEventSynchronize(done_ev[(b - 1) & 1]));
      if (pin[0]) done = true;
    }
  }
  if (loop_timing) HIPCHK(h, hipEventRecord(h->ev_loop[1], s));
  HIPCHK(h, copy_sync(s, st, v.state, bh::ST_COUNT * 4, hipMemcpyDeviceToHost));  // (one synchronisation)
  float lms = 0;
  if (loop_timing && hipEventElapsedTime(&lms, h->ev_loop[0], h->ev_loop[1]) == hipSuccess) h->loop_ms_acc += lms;
  (void)hipEventDestroy(done_ev[0]);
  (void)hipEventDestroy(done_ev[1]);
  if (!st[bh::ST_DONE]) return h->fail(BH_ERR_STATE, "round loop did not terminate");
  if (st[bh::ST_ERR]) return h->fail(BH_ERR_CAPACITY, "round table capacity exceeded");
  return BH_OK;
}

// the chain dataflow sweep where eligible; BH_SWEEP=chunk forces the chunked
// sweep (A/B and parity of both paths)
bool use_flow(const Dev &d) {
  const char *e = getenv("BH_SWEEP");
  return bh::flow_eligible(d) && !(e && !strcmp(e, "chunk"));
}

// the 32-bit chain-major FD rows (n > 128), allocated the first time a path
// that writes them runs (d.fd_rows): the default wide path never does
int ensure_fd(bh_handle *h) {
  Dev &d = h->d;
  if (d.fd_cols || !d.fd_rows || d.fd) return BH_OK;
  HIPCHK(h, hipMalloc((void **)&d.fd, (size_t)(d.la_rows + 64) * d.npad * 4));
  return BH_OK;
}


int ensure_events(bh_handle *h, std::vector<hipEvent_t> &v, size_t count, unsigned flags) {
  while (v.size() < count) {
    hipEvent_t e;
    HIPCHK(h, hipEventCreateWithFlags(&e, flags));
    v.push_back(e);
  }
  return BH_OK;
}

// ---------------------------------------------------------------------------
// stage 1: coordinates, Lamport timestamps, rounds, witnesses

// the chunked sweep (the fallback of the chain dataflows), e0 / e1 recorded
// around k_la_sweep alone
constexpr const char *CHUNKED_SWEEP = "k_la_sweep";
static int launch_chunked_sweep(bh_handle *h, hipStream_t s, hipEvent_t e0 = nullptr, hipEvent_t e1 = nullptr) {
  bh::launch_chunk_depth(h->d, s);
  if (e0) HIPCHK(h, hipEventRecord(e0, s));
  bh::launch_la_sweep(h->d, s);
  if (e1) HIPCHK(h, hipEventRecord(e1, s));
  bh::launch_permute(h->d, s);
  return BH_OK;
}

// a Reset hashgraph's rounds below r0, event by event (k_fiat_ls, the fiat
// region only), which also derives B[r0]
static int launch_fiat_pass(bh_handle *h, const Dev &v, hipStream_t s) {
  HIPCHK(h, hipMemsetAsync(v.rexists, 0, (size_t)v.R_cap + 1, s));
  HIPCHK(h, hipMemsetAsync(v.fw, 0xFF, (size_t)(v.r0 - v.rlo) * v.n * 4, s));
  HIPCHK(h, hipMemsetAsync(v.state + bh::ST_FIATMAX, 0xFF, 4, s));
  bh::launch_fiat(v, s);
  return BH_OK;
}

// A Reset hashgraph's coordinates (kernels_reset.hip): the events [0, E0)
// -- every event whose other-parent only Root.Others knows lies in it --
// one at a time, then the chain dataflow resumes every chain after them as
// a segment does (Root LamportTimestamps seed the chains, lt_seed); each
// part is transposed and walked for firstDescendants like a segment
int reset_coords(bh_handle *h, hipStream_t s) {
  Dev &d = h->d;
  const int n = d.n;
  if (!(bh::flow32_eligible(d) && use_flow(d)) && !bh::floww_eligible(d))
    return h->fail(BH_ERR_STATE, "Reset hashgraphs need the chain dataflow (n <= 512, chains within its limits)");
  const int64_t N = d.N, E0 = std::min<int64_t>(h->E0, N);
  int32_t *stg = h->seg_stage;  // [lo, len] of part A, then of part B
  for (int c = 0; c < n; ++c) {
    const auto &ch = h->chain[(size_t)c];
    const int32_t a = (int32_t)(std::lower_bound(ch.begin(), ch.end(), (int32_t)E0) - ch.begin());
    stg[c] = 0;
    stg[n + c] = a;
    stg[2 * n + c] = a;
    stg[3 * n + c] = (int32_t)ch.size();
  }
  HIPCHK(h, hipMemcpyAsync(h->segbuf, stg, (size_t)4 * n * 4, hipMemcpyHostToDevice, s));
  Dev va = d, vb = d;
  va.seg_lo = h->segbuf;
  va.chain_len = h->segbuf + n;
  va.N = E0;
  va.e0 = 0;
  va.tile_list = nullptr;
  vb.seg_lo = h->segbuf + 2 * n;
  vb.chain_len = h->segbuf + 3 * n;
  vb.e0 = E0;
  vb.tile_list = nullptr;
  if (E0 > 0) {
    bh::launch_reset_coords(va, s);
    bh::launch_flow_transpose(va, s);
    bh::launch_fd_idle(va, s);
  }
  HIPCHK(h, hipMemsetAsync(d.state + bh::ST_FLOWOVF, 0, 4, s));
  if (N > E0) {
    if (bh::flow32_eligible(d) && use_flow(d)) {
      bh::launch_flow_desc(vb, s);
      bh::launch_flow(vb, s);
      h->sweep_kernel = bh::flow_kernel(d);
    } else {
      bh::launch_floww(vb, s);
      h->sweep_kernel = bh::floww_kernel(d);
    }
    bh::launch_flow_transpose(vb, s);
    bh::launch_fd_idle(vb, s);
  }
  HIPCHK(h, hipGetLastError());
  return BH_OK;
}

// The segments left only the column-major LA (SegmentPipeline, n <= 128):
// the row-major LA and the complete FDT of the layout's rows up to the
// chain lengths `upto` -- a query's, or an eager call resuming a prefix --
// as the segment pipeline's eager transpose builds them: only the tiles of
// rows past the ones an earlier build covered (their FD entries of older
// rows are completed by the new rows' walk and k_fd_idle), or every row the
// first time and after a relayout.  Synchronous (its staging is reused).
int build_rows(bh_handle *h, const std::vector<int32_t> &upto, hipStream_t s) {
  const int n = h->d.n;
  Dev v = h->d;
  v.e0 = 0;
  v.rows = h->layout_rows;
  v.col0 = 0;
  v.ncol = n;
  v.xpose_fd = 1;
  const bool inc = h->rows_built && (int)h->rows_lens.size() == n;
  int32_t *stg = h->seg_stage;  // [lo | len] per chain
  for (int c = 0; c < n; ++c) {
    stg[c] = inc ? std::min(h->rows_lens[(size_t)c], upto[(size_t)c]) : 0;
    stg[n + c] = upto[(size_t)c];
  }
  HIPCHK(h, hipMemcpyAsync(h->segbuf, stg, (size_t)2 * n * 4, hipMemcpyHostToDevice, s));
  v.seg_lo = h->segbuf;
  v.chain_len = h->segbuf + n;
  v.tile_list = nullptr;
  v.ntiles = 0;
  if (inc) {  // the 64-row tiles holding the new rows, shared boundary tiles once
    int32_t *tl = h->tlist_stage;
    const int64_t nt = bh::tile_list(n, h->cstart_h.data(), stg, stg + n, tl);
    if (nt) HIPCHK(h, hipMemcpyAsync(h->tlist, tl, (size_t)nt * 4, hipMemcpyHostToDevice, s));
    v.tile_list = h->tlist;
    v.ntiles = nt;
  }
  if (!inc || v.ntiles > 0) bh::launch_flow_transpose(v, s);
  bh::launch_fd_idle(v, s);
  HIPCHK(h, hipGetLastError());
  HIPCHK(h, wait_stream(s));
  h->rows_lens = upto;
  h->rows_built = true;
  h->rows_stale = false;
  return BH_OK;
}

// coordinates up to the dataflow kernel (this shard's LA columns when split)
int rounds_coords(bh_handle *h) {
  int rc;
  if ((rc = upload(h))) return rc;
  Dev &d = h->d;
  d.N = (int64_t)h->h_creator.size();
  d.e0 = 0;
  d.seg_lo = h->seg_zero;
  h->xchg_ms = 0;
  h->segments_used = 1;
  h->inc_valid = false;
  h->fdt_lost = false;
  h->rows_stale = false;  // (rounds_loop transposes)
  h->rows_built = false;
  if ((rc = set_chain_tables(h))) return rc;
  d.rows = h->layout_rows;
  hipStream_t s = h->stream;
  HIPCHK(h, hipEventRecord(h->ev[0], s));
  bh::launch_prep(d, s);
  if (h->reset_on) {
    if ((rc = reset_coords(h, s))) return rc;
  } else if (use_flow(d)) {
    bh::launch_flow_desc(d, s);
    HIPCHK(h, hipEventRecord(h->ev_sweep[0], s));
    bh::launch_flow(d, s);
    HIPCHK(h, hipEventRecord(h->ev_sweep[1], s));
    h->sweep_kernel = bh::flow_kernel(d);
  } else if (bh::floww_eligible(d)) {
    HIPCHK(h, hipEventRecord(h->ev_sweep[0], s));
    bh::launch_floww(d, s);
    HIPCHK(h, hipEventRecord(h->ev_sweep[1], s));
    h->sweep_kernel = bh::floww_kernel(d);
  } else {
    if ((rc = launch_chunked_sweep(h, s, h->ev_sweep[0], h->ev_sweep[1]))) return rc;
    h->sweep_kernel = CHUNKED_SWEEP;
  }
  HIPCHK(h, hipGetLastError());
  return BH_OK;
}

static int rounds_tail(bh_handle *h, const int32_t *st, int64_t e_begin, bool tables_done = false);

// the rest: LA rows + firstDescendants, the round loop, witness tables
int rounds_loop(bh_handle *h) {
  int rc;
  Dev &d = h->d;
  hipStream_t s = h->stream;
  const bool walked = use_flow(d);
  bool wide_flow = bh::floww_eligible(d);
  if (wide_flow) {  // k_floww's watchdog (ST_FLOWOVF = 2): the chunked sweep instead
    int32_t ovf = 0;
    HIPCHK(h, hipMemcpyAsync(&ovf, d.state + bh::ST_FLOWOVF, 4, hipMemcpyDeviceToHost, s));
    HIPCHK(h, wait_stream(s));
    if (ovf == 2 && h->reset_on) {
      // the watchdog counts stalled headers, not a proven deadlock (other
      // work sharing the compute units can starve a wave): the Reset
      // coordinates have no sweep fallback (it knows no Root seeds), so the
      // dataflow runs once more before the call fails
      HIPCHK(h, hipMemsetAsync(d.state + bh::ST_FLOWOVF, 0, 4, s));
      if ((rc = reset_coords(h, s))) return rc;
      HIPCHK(h, hipMemcpyAsync(&ovf, d.state + bh::ST_FLOWOVF, 4, hipMemcpyDeviceToHost, s));
      HIPCHK(h, wait_stream(s));
    }
    if (ovf && h->reset_on)
      return h->fail(BH_ERR_CAPACITY, ovf == 2 ? "the wide dataflow gave up twice on a Reset hashgraph"
                                               : "Lamport timestamps beyond the wide dataflow's range after Reset");
    if (ovf == 2) {
      HIPCHK(h, hipMemsetAsync(d.state + bh::ST_FLOWOVF, 0, 4, s));
      if ((rc = launch_chunked_sweep(h, s))) return rc;
      h->sweep_kernel = CHUNKED_SWEEP;
      wide_flow = false;
    }
  }
  // LA rows and the firstDescendants walk (FDT) from the dataflow's
  // column-major LA; n > 128 then transposes FDT into chain-major FD rows
  if ((walked || wide_flow) && !h->reset_on) bh::launch_flow_transpose(d, s);  // (reset_coords transposed already)
  d.fd_rows = !((walked || wide_flow) && bh::round_p16(d));  // 32-bit fd rows only where read
  if ((rc = ensure_fd(h))) return rc;
  bh::launch_first_descendants(d, s, walked || wide_flow);
  HIPCHK(h, hipGetLastError());
  HIPCHK(h, hipEventRecord(h->ev[1], s));
  h->coords_for = (int)d.N;
  if (d.N == 0) {
    HIPCHK(h, hipEventRecord(h->ev[2], s));
    h->R = 0;
    h->n_div = 0;
    h->wofs_h.assign(1, 0);
    h->stage = 1;
    return BH_OK;
  }
  int32_t st[bh::ST_COUNT];
  d.wide_cols = 0;  // (the wide loop over FDT: rows were transposed above)
  d.use_cla = d.fd_cols && !bh::round_solo_eligible(d);
  if (h->reset_on) {
    // rounds below r0 event by event, then the loop from B[r0]
    if ((rc = launch_fiat_pass(h, d, s))) return rc;
    bh::launch_round_resume(d, s);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipMemcpyAsync(&h->fiat_max, d.state + bh::ST_FIATMAX, 4, hipMemcpyDeviceToHost, s));
    if (getenv("BH_FIAT_DEBUG")) {
      int32_t fs[4] = {0, 0, 0, 0};
      HIPCHK(h, hipMemcpyAsync(fs, d.state + bh::ST_FIATMAX, 16, hipMemcpyDeviceToHost, s));
      HIPCHK(h, wait_stream(s));
      fprintf(stderr, "[k_fiat] max round %d, chains done %d of %d, events visited %d, chunks %d (r0 %d)\n", fs[0], fs[1],
              d.n, fs[2], fs[3], d.r0);
      if (d.diag) {
        unsigned long long g[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        HIPCHK(h, copy_sync(s, g, d.diag + 24, sizeof g, hipMemcpyDeviceToHost));
        const double e = (double)(g[4] ? g[4] : 1);
        fprintf(stderr, "[k_fiat] cycles per event (BH_FIAT=serial: finalize + pr, witness rows, counts) or per step "
                "(level-synchronous: parents, counts, rounds): %.0f, %.0f, %.0f (%llu); round stagings %llu\n",
                g[0] / e, g[1] / e, g[2] / e, g[4], g[7]);
        HIPCHK(h, hipMemsetAsync(d.diag + 24, 0, sizeof g, s));
      }
    }
  } else {
    bh::launch_round_init(d, s);
  }
  if ((rc = run_round_loop(h, d, &h->graph, &h->graph_dev, &h->graph_s, &h->graph_dev_s, st))) return rc;
  bh::launch_resume_point(d, st[bh::ST_ROUNDS], nullptr, s);  // each chain's resume round (rq) for the next call
  if ((rc = rounds_tail(h, st, 0))) return rc;
  if (h->reset_on && !h->fdt_lost) {
    // a Reset hashgraph's later calls resume from here (rounds_segmented):
    // the chain dataflow left every LA row and a complete FDT
    commit_coords(h, d.N, true);
  }
  return BH_OK;
}

// after the loop: witness tables, per-event rounds, PendingRounds.  Rounds
// and witness flags of events [0, e_begin) are unchanged (an incremental
// call appended events only)
static int rounds_tail(bh_handle *h, const int32_t *st, int64_t e_begin, bool tables_done) {
  Dev &d = h->d;
  hipStream_t s = h->stream;
  h->R = st[bh::ST_ROUNDS];
  h->iters = st[bh::ST_ITERS];
  // a Reset hashgraph with no event at round r0 yet: the last round is the fiat pass's
  if (h->reset_on && h->R <= d.r0) h->R = h->fiat_max + 1;
  if (h->reset_on && st[bh::ST_FLOWOVF])  // the fallbacks know no Root LamportTimestamps
    return h->fail(BH_ERR_CAPACITY, "Lamport timestamps beyond the dataflow kernel's range after Reset");
  if (st[bh::ST_FLOWOVF]) {  // LT reached the one-dword limit; LT only feeds the frame order
    if (bh::floww_eligible(d)) {  // the chunked sweep recomputes LA (same values) and LT
      int rc;
      if ((rc = launch_chunked_sweep(h, s))) return rc;
      // its slabs share FDT's memory: the next query recomputes the
      // coordinates, the next pass starts from scratch
      h->coords_for = -1;
      h->fdt_lost = true;
      h->rows_built = false;
    } else {
      bh::launch_flow_lt_fallback(d, s);
    }
  }
  // (tables_done: SegmentPipeline::finish_async launched them from the device's round
  // count, ahead of its synchronisation)
  if (!tables_done) bh::launch_witness_tables(d, h->R, s);
  bh::launch_assign_rounds(d, e_begin, h->n_div, h->P, s);
  HIPCHK(h, hipGetLastError());
  HIPCHK(h, hipEventRecord(h->ev[2], s));
  if (!(h->fuse_fame && h->world == 1)) {
    // the witness offsets (the split's fame exchange reads them), behind the
    // stage's synchronisation.  bh_run_consensus on one shard goes on to
    // DecideFame at once instead: its scatter reads the bounds on the device
    h->wofs_h.resize((size_t)h->R + 1);
    int rc;
    if ((rc = rd_async(h, s, h->wofs_h.data(), d.wofs, ((size_t)h->R + 1) * 4)) || (rc = rd_wait(h, s))) return rc;
  }
  h->n_div = d.N;
  // rounds new to this call join PendingRounds undecided (hashgraph.go:809-815;
  // every round >= LastConsensusRound is queued when it first appears)
  h->pend_dec.resize((size_t)h->R, 0);
  h->stage = 1;
  return BH_OK;
}

// Coordinates and rounds as a pipeline over K insertion-order prefixes
// (segments): the coordinate kernels of prefix s + 1 run on stream2 while
// the round loop runs prefix s on `stream`, resuming at the last round the
// previous prefix fixed (k_resume_point).  Chain dataflow paths only:
// n <= 128 (k_flow32 + k_round2) and 128 < n <= 512 (k_floww2 + the 16-bit
// k_round_wide over the complete FDT); every shard of a group whose
// coordinates are replicated (the default) runs it on its own device.
static bool segments_eligible(const bh_handle *h) {
  const Dev &d = h->d;
  if (h->shard_cols) return false;
  if (d.fd_cols) return use_flow(d) && bh::flow32_eligible(d);
  return bh::floww_eligible(d) && bh::round_p16(d);
}

// segments for `events` new events: measured at C3 (10M events): 4
// segments 73.4 ms, 8 segments 72.4 ms, one 84.3 ms (profiles/r2_segments.log).
// The wide path (n > 128) takes one: k_floww2 (145 KiB of LDS) and the
// wide transpose leave no compute unit room for a k_round_wide workgroup,
// so its segments run one after the other and only cost more (C4: 284 ->
// 316 ms with 8, profiles/r3_c4_segments.log); its incremental calls still
// run as one more segment of the same machinery
int segments_for(const Dev &d, int64_t events) {
  // (round 3: C5, 2M events, 79.0M events/s at 4 segments, 87.0M at 8,
  // 88.1M at 12; C2, 1M events, 48.6M at 4, 48.3M at 8; C3 equal at 8 and 12)
  // (round 4, persistent loop, C3: with each segment's LT after the next
  // one's columns, 8 segments 188.8M events/s, 16 187.6M, 24 184.1M)
  // (round 5, C3 10M events, segment k holding a 1.38^k share: 38.1-38.4 ms
  // per step at 10-14 segments against 40.1 at 8 segments of 1.5^k)
  // (round 6: at n <= 96 the dataflow and the loop take about as long, so
  // more, flatter segments shorten the loop left after the dataflow's end;
  // at n = 128 the lean loop is only ~1.14x the dataflow: 16 of 1.15x)
  int K = !d.fd_cols ? 1
          : d.n <= 96 ? (events >= 1000000 ? 12 : 1)
                      : (events >= 4000000 ? 16 : events >= 1500000 ? 8 : events >= 1000000 ? 4 : 1);
  if (const char *e = getenv("BH_SEGMENTS")) K = atoi(e);
  return (int)std::max<int64_t>(1, std::min<int64_t>({K, events / 4096 + 1, 64}));
}

// The growth ratio: segment k + 1's dataflow runs beside segment k's loop,
// so it can grow by (loop time / dataflow time) per event and still be ready
// when the loop reaches it; grown faster, the loop waits for it between
// segments.  That ratio depends on n: at C3 (n = 128) the loop is ~1.14x
// the dataflow (29.4 against 25.9 ms per step with k_round_lean; 1.32 with
// k_round2p left 3.35 ms of waits between the loop's launches,
// profiles/r6_seg_sweep_lean.txt: 34.5 -> 32.0 ms at 1.15 x 16 segments);
// at C5 (n = 64) and C2 (n = 32) the two take about the same time, where
// growing segments only leave a long last loop after the dataflow's end:
// equal segments.  BH_SEG_RATIO overrides it (A/B)
// (round 6, profiles/r6_seg_sweep.txt, r6_seg_sweep_lean.txt: C5 16.89 ->
// 14.3 ms with 12 equal segments, C2 11.63 -> 9.6 ms with 12 equal segments)
constexpr double SEG_RATIO_WIDE = 1.15, SEG_RATIO_NARROW = 1.0;
double seg_ratio(const Dev &d) {
  if (const char *e = getenv("BH_SEG_RATIO")) return std::max(1.0, atof(e));
  return d.n > 96 ? SEG_RATIO_WIDE : SEG_RATIO_NARROW;
}

// per-chain prefix lengths at an insertion-order boundary (ids of a chain
// ascend with its index); bounds at or below the events inserted so far
// are kept (lens_memo)
void chain_lens_at(const bh_handle *h, int64_t bound, int32_t *out) {
  const int n = h->d.n;
  const bool keep = bound <= (int64_t)h->h_creator.size();
  if (keep) {
    const auto it = h->lens_memo.find(bound);
    if (it != h->lens_memo.end() && (int)it->second.size() == n) {
      std::copy(it->second.begin(), it->second.end(), out);
      return;
    }
  }
  for (int c = 0; c < n; ++c) {
    const auto &ch = h->chain[(size_t)c];
    out[c] = (int32_t)(std::lower_bound(ch.begin(), ch.end(), (int32_t)std::min<int64_t>(bound, INT32_MAX)) - ch.begin());
  }
  if (keep) {
    if (h->lens_memo.size() >= 1024) h->lens_memo.clear();
    h->lens_memo[bound].assign(out, out + n);
  }
}

// ---------------------------------------------------------------------------
// the segment pipeline

namespace {

// the events a call creates for itself, released on every return path
struct CallEvents {
  hipEvent_t sr_mark = nullptr;             // the loop stream's progress, for segbuf reuse by stream2
  hipEvent_t lt0 = nullptr, lt1 = nullptr;  // BH_SEG_DEBUG: around a segment's loop
  CallEvents() = default;
  CallEvents(const CallEvents &) = delete;
  CallEvents &operator=(const CallEvents &) = delete;
  ~CallEvents() {
    for (hipEvent_t e : {sr_mark, lt0, lt1})
      if (e) (void)hipEventDestroy(e);
  }
};

// a call's switches
struct PipelineModes {
  bool cshard;  // (split_all: a coordinate shard that runs the loop too)
  bool wide;    // k_floww2 + k_round_wide (cand16 from FDT)
  bool eager;   // the segments build the row-major LA and FDT
  bool dbg;     // BH_SEG_DEBUG: per-segment timings to stderr
  bool async, lt_combined, loop_timing;
  int npar;
};

// ... read once where the call starts (the tests switch the BH_* knobs
// between calls of one process); sets the loop's switches in h->d
PipelineModes pipeline_modes(bh_handle *h, const SplitPlan *sp) {
  Dev &d = h->d;
  PipelineModes m;
  m.cshard = sp && h->rank > 0;
  m.wide = !d.fd_cols;
  if (m.wide) d.fd_rows = 0;
  // n <= 128: k_round2 and fame read only the dataflow's column-major LA, so
  // the segments skip the row-major LA and FDT (the transpose; 21 GB of the
  // C3 step's HBM traffic) -- queries build them on demand (ensure_coords).
  // A Reset hashgraph's fiat pass and the resident loop (BH_ROUND_SOLO) read
  // them; BH_EAGER_ROWS=1 builds them anyway (A/B)
  // 128 < n <= 512: the 16-bit wide loop reads la_col as well (window,
  // candidates' FD rows, fame's LA rows; k_round_wide<*, true, true>) --
  // BH_WIDE_ROWS=1 keeps the FDT / row-major LA loop (A/B)
  const bool eager_env = getenv("BH_EAGER_ROWS") && atoi(getenv("BH_EAGER_ROWS"));
  const bool wide_rows_env = !getenv("BH_WIDE_COLS") || !atoi(getenv("BH_WIDE_COLS")) ||
                             (getenv("BH_WIDE_ROWS") && atoi(getenv("BH_WIDE_ROWS")));  // (off until verified)
  d.wide_cols = m.wide && !sp && !h->reset_on && !wide_rows_env && !eager_env && bh::round_p16(d) && d.cla && d.n <= 512;
  // BH_WIDE_COLS=2 (A/B): the window from the transposed row-major LA, the hand-off from la_col
  if (d.wide_cols && atoi(getenv("BH_WIDE_COLS")) == 2) d.wide_cols = 2;
  // (the wide split: shard 0 transposes each received segment for the
  // row-major loop)
  m.eager = sp ? m.wide
               : ((m.wide && d.wide_cols != 1) || h->reset_on || eager_env || bh::round_solo_eligible(d) ||
                  d.round_src_rows);
  d.use_cla = (d.fd_cols || d.wide_cols) && !bh::round_solo_eligible(d);
  if (sp) d.round_src_rows = 0;  // the split ships the column-major LA only
  // segment lengths on the device: three buffers round robin, so that
  // segment k + 1's dataflow waits only for loop k - 2 (long finished) and
  // runs beside loop k - 1 -- with two, its launches (the lengths' copy,
  // k_flow_desc32x2) waited for loop k - 1 and landed on the compute units
  // in the gap between two loops, beside k_seg_resume (15 -> 35 us, C3).
  // The eager rows' tile lists keep two
  m.npar = sp || m.eager ? 2 : 3;
  // where a segment's Lamport timestamps run: k_flow32x2 (the default)
  // carries them in its first workgroup, (n + 1) / 2 workgroups in all.  The
  // one-value k_flow32 (chains past X2_MAXLEN; BH_FLOW1) needs a workgroup of
  // its own for them: inside the column launch while 2n + 1 workgroups fit
  // the compute units beside the loop's n (C5: 82 -> 101M events/s in round
  // 4), else after the next segment's columns on the coordinate stream (at
  // n = 128 a 129th column workgroup would share a unit with a loop
  // workgroup, which every barrier then waits for; profiles/r4_ab_lt.txt)
  m.lt_combined = m.wide || bh::flow32x2_eligible(d) || 2 * d.n + 1 <= h->ncu;
  // n <= 128 with the persistent loop: every segment's loop is enqueued
  // without a host round trip (each used to wait for its loop's state: ~0.2
  // ms of idle device per segment at C3, profiles/r5_gaps_c3.txt).  The
  // resume point reads the round count on the device, a failed loop makes
  // the later ones leave at once (ST_PFAIL), and the host reads the state
  // once, after the last loop.  Other loops (wide, one launch per round,
  // BH_SEG_DEBUG) wait for each segment as before
  m.dbg = getenv("BH_SEG_DEBUG") && atoi(getenv("BH_SEG_DEBUG"));
  m.async = !m.wide && !m.eager && !m.dbg && bh::round_persist_eligible(d);
  m.loop_timing = !(getenv("BH_LOOP_TIMING") && !atoi(getenv("BH_LOOP_TIMING")));
  return m;
}

std::vector<int64_t> pipeline_bounds(const Dev &d, int K, int64_t base) {
  std::vector<int64_t> Ns((size_t)K + 1, base);
  bh::segment_bounds(base, d.N, K, seg_ratio(d), Ns.data());
  return Ns;
}

// One call of the pipeline.  base > 0: an incremental call -- events
// [0, base) hold coordinates and the round loop left its resume point
// (ST_RESUME) for that prefix.  sp: the coordinate split -- the segments'
// columns arrive from the coordinate shards (grp: the in-process group, else
// over h->xport) instead of being computed here; on a coordinate shard of
// the narrow split (split_all) its own columns come from its dataflow
// (split_coords, stream2) and the others' arrive beside it
struct SegmentPipeline {
  bh_handle *const h;
  Dev &d;  // the whole prefix: every segment's view derives from it
  const int n, K;
  const int64_t base, N;
  const SplitPlan *const sp;
  const std::vector<bh_handle *> *const grp;
  const bool cshard, wide, eager, dbg, async, lt_combined, loop_timing;
  const int npar;
  // the loop's stream, the coordinates', and the split's receives and
  // unpacks: a stream of their own, beside a coordinate shard's dataflow
  const hipStream_t sr, sc, sx;
  const std::vector<int64_t> Ns;  // segment k: events [Ns[k], Ns[k + 1])
  // A blocking transport (the host transport's receives and broadcasts wait
  // on the host) takes segment k + 1 after loop k is enqueued, so loop k runs
  // while the host waits for segment k + 1; stream-ordered
  // exchanges go first, as the dataflow's launches do
  const bool late;
  // the witness tables from the device's round count, launched behind the
  // state's read-back so that they run while the host wakes up (the host
  // checks the state before anything reads them: a failed loop's fallback
  // builds them again)
  const bool tables_early;
  int32_t host_resume;
  int32_t st[bh::ST_COUNT] = {};
  bool wd_fired = false;
  CallEvents ev;

  SegmentPipeline(bh_handle *h, int K, int64_t base, const SplitPlan *sp, const std::vector<bh_handle *> *grp,
                  const PipelineModes &m)
      : h(h), d(h->d), n(h->d.n), K(K), base(base), N(h->d.N), sp(sp), grp(grp), cshard(m.cshard), wide(m.wide),
        eager(m.eager), dbg(m.dbg), async(m.async), lt_combined(m.lt_combined), loop_timing(m.loop_timing),
        npar(m.npar), sr(h->stream), sc(h->stream2), sx(sp ? h->stream3 : h->stream2),
        Ns(pipeline_bounds(h->d, K, base)), late(sp && h->xport && h->xport->blocking()),
        tables_early(m.async && !h->reset_on), host_resume(h->d.r0) {}

  Dev view(int k) const {
    return segment_view(h, d, sp ? sp->dview(h, k) : h->segbuf + (size_t)(k % npar) * 2 * n, Ns.data(), k);
  }
  Dev loop_view(int k) const {  // the loop's view: only the prefix lengths differ from d
    Dev rv = d;
    rv.chain_len = view(k).chain_len;
    return rv;
  }

  // an incremental call resumes at the last round whose boundaries lie
  // inside the previous prefix on every chain this call extends
  // (k_resume_point left each chain's first outside round in rq)
  // a coordinate shard of the narrow split finds no grown
  // chain here (split_coords committed this call's lengths already) and
  // restarts from r0 -- the fix touches this and split_coords' commit_coords
  int host_resume_round() {
    if (base == 0) return BH_OK;
    std::vector<int32_t> rq((size_t)n);
    HIPCHK(h, copy_sync(sr, rq.data(), d.rq, (size_t)n * 4, hipMemcpyDeviceToHost));
    host_resume = bh::resume_round(n, rq.data(), h->lens_coord.data(), h->lens_h.data(), d.r0);
    return BH_OK;
  }

  // before the first segment: events, the resume round, the chain tables
  int prepare() {
    int rc;
    h->segments_used = K;
    h->fdt_lost = false;
    if ((rc = ensure_events(h, h->seg_ev, (size_t)4 * K, hipEventDefault)) || (rc = host_resume_round())) return rc;
    // the coordinate stream starts after everything queued on the main one
    HIPCHK(h, hipEventRecord(h->ev[0], sr));
    HIPCHK(h, hipStreamWaitEvent(sc, h->ev[0], 0));
    if (!cshard) {  // (a coordinate shard's split_coords queued them ahead of its dataflow)
      if (base == 0) {
        bh::launch_prep(d, sc);
      } else {  // only the new events' chain-table entries; loop state kept
        bh::launch_chain_scatter(d, base, sc);
      }
      HIPCHK(h, hipMemsetAsync(d.state + bh::ST_FLOWOVF, 0, 4, sc));
    }
    if (sp && !cshard) {  // the unpacks wait for the chain tables and the cleared flag
      HIPCHK(h, hipEventRecord(h->xprep, sc));
      HIPCHK(h, hipStreamWaitEvent(sx, h->xprep, 0));
    }
    HIPCHK(h, hipMemsetAsync(d.state + bh::ST_PFAIL, 0, 4, sr));
    if (async && (rc = ensure_events(h, h->loop_evs, (size_t)2 * K, hipEventDefault))) return rc;
    return BH_OK;
  }

  // the 64-row tiles holding segment k's rows (the transpose's work list):
  // each chain's run [start + lo, start + hi), in layout order, shared
  // boundary tiles once (eager runs wait for each loop: the staging's two
  // halves cannot be overtaken)
  int tile_list(int k, const int32_t *lo, const int32_t *hi, Dev &v, hipStream_t ts) {
    int32_t *tl = h->tlist_stage + (size_t)(k & 1) * h->tlist_cap;
    const int64_t nt = bh::tile_list(n, h->cstart_h.data(), lo, hi, tl);
    int32_t *dtl = h->tlist + (size_t)(k & 1) * h->tlist_cap;
    if (nt) HIPCHK(h, hipMemcpyAsync(dtl, tl, (size_t)nt * 4, hipMemcpyHostToDevice, ts));
    v.tile_list = dtl;
    v.ntiles = nt;
    return BH_OK;
  }

  // the split: segment k's columns from the coordinate shards (every other
  // one: a coordinate shard of the narrow split computed its own), into the
  // common block layout -- the narrow split all-gathers them (a broadcast
  // per coordinate rank, in place; in process, peer copies), the wide one
  // receives them on shard 0 only
  int receive(int k) {
    int rc;
    Dev v = view(k);
    HIPCHK(h, hipEventRecord(h->seg_ev[(size_t)3 * K + k], sx));
    if (cshard) HIPCHK(h, hipStreamWaitEvent(sx, h->pack_ev[(size_t)k], 0));  // its own block (its dataflow) done
    if (grp) {
      for (int r = 1; r < h->world; ++r)
        if (r != h->rank) HIPCHK(h, hipStreamWaitEvent(sx, (*grp)[(size_t)r]->pack_ev[(size_t)k], 0));
    }
    HIPCHK(h, hipEventRecord(h->seg_ev[(size_t)3 * k + 1], sx));
    std::vector<bh::SplitBlock> blk((size_t)h->world);
    for (int r = 1; r < h->world; ++r) blk[(size_t)r] = sp->block(h, k, r, h->xbuf + sp->boff(h, k, r));
    if (grp) {  // peer copies (xGMI between devices, a device copy on a shared one)
      for (int r = 1; r < h->world; ++r) {
        if (r == h->rank) continue;
        const bh_handle *x = (*grp)[(size_t)r];
        const size_t o = sp->boff(h, k, r);
        HIPCHK(h, hipMemcpyPeerAsync(h->xbuf + o, h->device, x->xbuf + o, x->device, sp->block_bytes(h, k, r), sx));
      }
    } else {
      if ((rc = h->xport->group_start(h))) return rc;
      for (int r = 1; r < h->world; ++r) {
        uint8_t *at = h->xbuf + sp->boff(h, k, r);
        const size_t bb = sp->block_bytes(h, k, r);
        rc = h->split_all() ? h->xport->bcast(h, at, bb, r, sx) : h->xport->recv(h, at, bb, r, sx);
        if (rc) {
          (void)h->xport->group_end(h);
          return rc;
        }
      }
      if ((rc = h->xport->group_end(h))) return rc;
    }
    HIPCHK(h, hipEventRecord(h->seg_ev[(size_t)3 * k + 2], sx));
    for (int r = 1; r < h->world; ++r)
      if (r != h->rank) bh::launch_split_unpack(v, sp->dpq(h, k), blk[(size_t)r], sx);
    bh::launch_lt_rows(v, sx);
    if (eager) {
      // the wide loop reads the row-major LA and FDT: the segment's rows
      // transposed here, from the columns just unpacked
      const int32_t *lo = sp->tab.data() + (size_t)k * 2 * n;
      if ((rc = tile_list(k, lo, lo + n, v, sx))) return rc;
      bh::launch_flow_transpose(v, sx);
      bh::launch_fd_idle(v, sx);
    }
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipEventRecord(h->seg_ev[(size_t)3 * k], sx));
    if (k == K - 1) HIPCHK(h, hipEventRecord(h->ev[1], sx));
    return BH_OK;
  }

  // (!lt_combined) segment kk's LT workgroup and per-event LT, on the coordinate stream
  void lamport_after(int kk) {
    const Dev vk = view(kk);
    Dev vl = vk;
    vl.ncol = 0;
    vl.flow_lt = 1;
    bh::launch_flow(vl, sc);
    bh::launch_lt_rows(vk, sc);
  }

  // segment k's coordinates on the coordinate stream (the split: received)
  int coords(int k) {
    if (sp) return receive(k);
    int rc;
    Dev v = view(k);
    // pinned staging of its own per segment: with the loops enqueued without
    // host waits (async) the host runs ahead of these copies
    int32_t *stg = h->seg_stage + (size_t)k * 2 * n;
    chain_lens_at(h, Ns[(size_t)k], stg);
    chain_lens_at(h, Ns[(size_t)k + 1], stg + n);
    HIPCHK(h, hipMemcpyAsync(v.seg_lo, stg, (size_t)2 * n * 4, hipMemcpyHostToDevice, sc));
    HIPCHK(h, hipEventRecord(h->seg_ev[(size_t)3 * K + k], sc));  // the segment's lengths are on the device
    if (eager) {
      if ((rc = tile_list(k, stg, stg + n, v, sc))) return rc;
    } else {
      v.tile_list = nullptr;
      v.ntiles = 0;
    }
    // a whole-DAG wide run takes the whole-layout transpose (32-row tiles,
    // several workgroups per compute unit) instead of 64-row tile lists
    if (wide && K == 1 && base == 0) v.tile_list = nullptr;
    if (wide) {
      HIPCHK(h, hipEventRecord(h->seg_ev[(size_t)3 * k + 1], sc));
      bh::launch_floww(v, sc);  // the segment's descriptors, then k_floww2
    } else {
      bh::launch_flow_desc(v, sc);
      HIPCHK(h, hipEventRecord(h->seg_ev[(size_t)3 * k + 1], sc));
      // the LA columns only: n workgroups.  With the Lamport timestamps'
      // workgroup beside them (n + 1 = 129 at n = 128) one compute unit of
      // the 256 hosts a column workgroup and a round-loop workgroup at once,
      // and every loop iteration waits for that slower one (C3: 10.8 against
      // 9.7 us per iteration); LT, which the loop does not read, follows
      // once the segment's columns are handed to the loop
      Dev vc = v;
      vc.flow_lt = lt_combined ? 1 : 0;
      bh::launch_flow(vc, sc);
    }
    HIPCHK(h, hipEventRecord(h->seg_ev[(size_t)3 * k + 2], sc));
    if (eager) {
      // (wide_cols 2: the loop's windows need the row-major LA, its hand-off
      // no FDT -- the transpose writes LA rows only)
      Dev vt = v;
      vt.xpose_fd = d.wide_cols == 2 ? 0 : 1;
      bh::launch_flow_transpose(vt, sc);  // (its LT copy is redone by k_lt_rows below)
      if (vt.xpose_fd) bh::launch_fd_idle(v, sc);
    }
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipEventRecord(h->seg_ev[(size_t)3 * k], sc));  // the segment's LA is ready for the loop
    if (!wide && lt_combined) {
      bh::launch_lt_rows(v, sc);
    } else if (!wide) {
      // the Lamport timestamps of the segment before this one, after this
      // segment's columns: the loop's next segment waits only for columns
      // (the last segment's follow its own columns)
      if (k > 0) lamport_after(k - 1);
      if (k == K - 1) lamport_after(k);
    } else if (!eager) {  // wide: k_floww2 wrote lt_row; per-event LT (the transpose copies it otherwise)
      bh::launch_lt_rows(v, sc);
      HIPCHK(h, hipGetLastError());
    }
    if (k == K - 1) HIPCHK(h, hipEventRecord(h->ev[1], sc));  // the coordinate pipeline's end
    return BH_OK;
  }

  // segment k + 1's coordinates (or receive), once its buffers are free
  int coords_next(int k) {
    if (k + 1 >= K) return BH_OK;
    // segment k + 1 reuses the segbuf (and tile-list) slot of k + 1 - npar,
    // last read by its loop (async: the loop's own stop event -- no marker
    // packet on the loop stream) or its resume point
    if (async && npar == 3) {
      if (k >= 2) HIPCHK(h, hipStreamWaitEvent(sx, h->loop_evs[(size_t)2 * (k - 2) + 1], 0));
    } else if (async && k > 0) {
      HIPCHK(h, hipStreamWaitEvent(sx, h->loop_evs[(size_t)2 * k - 1], 0));
    } else {
      HIPCHK(h, hipEventRecord(ev.sr_mark, sr));
      HIPCHK(h, hipStreamWaitEvent(sx, ev.sr_mark, 0));
    }
    return coords(k + 1);
  }

  // k_floww2's watchdog (ST_FLOWOVF = 2; the split: a block that ran out of
  // overflow slots) is read before a loop runs on the segment: a loop over
  // unfinished coordinates could fail ("did not terminate", capacity) before
  // finish_watchdog's fallback is reached.  One host synchronisation per
  // segment; a wide batch runs one segment.  (The persistent n <= 128 loop
  // leaves at once on the flag itself.)  Every segment's receive is still
  // posted, so no coordinate rank's send is left unmatched
  int read_watchdog() {
    if (!(wide || sp) || async) return BH_OK;
    int32_t *ovf = h->pinned_state + bh::ST_COUNT + 4;
    HIPCHK(h, hipMemcpyAsync(ovf, d.state + bh::ST_FLOWOVF, 4, hipMemcpyDeviceToHost, sr));
    HIPCHK(h, wait_stream(sr));
    if (*ovf == 2) wd_fired = true;
    return BH_OK;
  }

  // the loop's inputs for segment k: the first rounds, or where the
  // previous prefix's loop stopped
  int start_loop(int k) {
    int rc;
    const Dev rv = loop_view(k);
    if (dbg) HIPCHK(h, hipEventRecord(ev.lt0, sr));
    if (k == 0 && base == 0) {
      bh::launch_round_init(rv, sr);
    } else if (async && k > 0) {
      // the previous loop's resume point and this segment's first
      // candidates in one launch (k_seg_resume: k_resume_point +
      // k_round_resume + k_cand_rows)
      Dev rs = rv;
      rs.seg_lo = view(k).seg_lo;  // (the previous prefix's lengths)
      bh::launch_seg_resume(rs, sr);
    } else {
      if (k == 0) {
        if (h->reset_on) {  // a Reset hashgraph: the rounds below r0 again
          if ((rc = launch_fiat_pass(h, rv, sr))) return rc;
          HIPCHK(h, hipGetLastError());
          HIPCHK(h, hipMemcpyAsync(h->pinned_state + bh::ST_COUNT + 2, d.state + bh::ST_FIATMAX, 4,
                                   hipMemcpyDeviceToHost, sr));
        }
        h->pinned_state[bh::ST_COUNT + 1] = host_resume;
        HIPCHK(h, hipMemcpyAsync(d.state + bh::ST_RESUME, h->pinned_state + bh::ST_COUNT + 1, 4, hipMemcpyHostToDevice, sr));
      }
      bh::launch_round_resume(rv, sr);
    }
    return BH_OK;
  }

  int launch_loop(int k) {
    const Dev rv = loop_view(k);
    if (!async)
      return run_round_loop(h, rv, &h->seg_graph[k & 1], &h->seg_graph_dev[k & 1], &h->seg_graph_s[k & 1],
                            &h->seg_graph_dev_s[k & 1], st);
    ++h->persist_loops;
    bh::launch_round_persist(rv, sr, h->loop_evs[(size_t)2 * k], h->loop_evs[(size_t)2 * k + 1]);
    HIPCHK(h, hipGetLastError());
    return BH_OK;
  }

  // where the next segment -- or the next call's new events -- resume
  int resume_point(int k) {
    const Dev rv = loop_view(k);
    const int32_t *next_len = nullptr;
    if (k + 1 < K) {
      // (async: the next iteration's wait for segment k + 1's columns, recorded
      // after its lengths on the same stream, covers k_seg_resume -- one
      // barrier packet less between two loops)
      if (!async) HIPCHK(h, hipStreamWaitEvent(sr, h->seg_ev[(size_t)3 * K + k + 1], 0));
      next_len = view(k + 1).chain_len;
    }
    // (async: the next segment's k_seg_resume finds it)
    if (!(async && k + 1 < K)) bh::launch_resume_point(rv, async ? -1 : st[bh::ST_ROUNDS], next_len, sr);
    if (!dbg) return BH_OK;
    HIPCHK(h, hipEventRecord(ev.lt1, sr));
    HIPCHK(h, wait_stream(sr));
    float lms = 0, cms = 0, fms = 0;
    (void)hipEventElapsedTime(&lms, ev.lt0, ev.lt1);
    (void)hipEventElapsedTime(&fms, h->seg_ev[(size_t)3 * k + 1], h->seg_ev[(size_t)3 * k + 2]);
    (void)hipEventElapsedTime(&cms, h->seg_ev[(size_t)3 * k + 1], h->seg_ev[(size_t)3 * k]);
    int32_t r0 = 0;
    (void)copy_sync(sr, &r0, rv.state + bh::ST_RESUME, 4, hipMemcpyDeviceToHost);
    fprintf(stderr, "[seg %d] coords %.2f ms (%s %.2f) | loop %.2f ms, rounds %d, iters %d, next resume at %d\n", k,
            cms, wide ? "k_floww2" : bh::flow_kernel(d), fms, lms, st[bh::ST_ROUNDS], st[bh::ST_ITERS], r0);
    return BH_OK;
  }

  // the whole call again through the unpipelined passes on this shard
  // (drop_persist: one loop launch per iteration)
  int rerun_unpipelined(bool drop_persist) {
    h->inc_valid = false;
    h->segments_used = 1;
    HIPCHK(h, wait_stream(sc));
    HIPCHK(h, wait_stream(sx));
    const int32_t keep = d.round_persist;
    if (drop_persist) d.round_persist = 0;
    int rc = rounds_coords(h);
    if (!rc) rc = rounds_loop(h);
    d.round_persist = keep;
    return rc;
  }

  // async: every loop's end, one host synchronisation for the call
  int finish_async(bool *rerun) {
    int rc;
    if ((rc = rd_async(h, sr, st, d.state, bh::ST_COUNT * 4))) return rc;
    if (tables_early) {
      HIPCHK(h, hipEventRecord(h->ev_st, sr));
      bh::launch_witness_tables(d, -1, sr);
      if ((rc = rd_wait_event(h, h->ev_st))) return rc;
    } else if ((rc = rd_wait(h, sr))) {
      return rc;
    }
    const int32_t fail = std::max(st[bh::ST_PFAIL], st[bh::ST_ERR]);
    if (fail == 1 || (fail == 0 && st[bh::ST_FLOWOVF] != 2 && !st[bh::ST_DONE]))
      return h->fail(fail == 1 ? BH_ERR_CAPACITY : BH_ERR_STATE,
                     fail == 1 ? "round table capacity exceeded" : "round loop did not terminate");
    if (fail == 3) {
      // a grid barrier gave up (some workgroup was never placed): one loop
      // launch per iteration (counted in persist_fallbacks)
      ++h->persist_fallbacks;
      *rerun = true;
      return rerun_unpipelined(true);
    }
    return BH_OK;
  }

  // k_floww2's watchdog left a segment's coordinates unfinished (or a split
  // block could not carry its columns): the unpipelined passes fall back to
  // the chunked sweep
  int finish_watchdog(bool *rerun) {
    if (!((wide || sp) && (wd_fired || st[bh::ST_FLOWOVF] == 2))) return BH_OK;
    *rerun = true;
    return rerun_unpipelined(false);
  }

  int commit() {
    int rc;
    // the last segment's Lamport timestamps run after its LA columns were
    // handed to the loop (coords): the passes after DivideRounds (the frame
    // order reads LT) wait for the coordinate stream's end
    HIPCHK(h, hipStreamWaitEvent(sr, h->ev[1], 0));
    h->coords_for = (int)N;
    h->rows_stale = !eager || d.wide_cols == 2;  // (wide_cols 2 built no FDT)
    if (!h->rows_stale) {  // (the segments' eager transposes built every row so far)
      h->rows_lens = h->lens_h;
      h->rows_built = true;
    }
    h->sweep_kernel = wide ? bh::floww_kernel(d) : bh::flow_kernel(d);
    if (h->reset_on && base > 0) h->fiat_max = h->pinned_state[bh::ST_COUNT + 2];
    if ((rc = rounds_tail(h, st, base, tables_early))) return rc;
    // the timings: every event completed before rounds_tail's synchronisation.
    // Read when asked (settle_timings): ~2K event queries here would hold the
    // device idle between DivideRounds and DecideFame
    h->tm_seg_K = K;
    h->tm_seg_loops = async && loop_timing;
    h->tm_seg_sp = sp != nullptr;
    h->tm_seg = true;
    if (sp) settle_timings(h);  // (the exchange time feeds the split's stage table now)
    commit_coords(h, N, !h->fdt_lost);
    return BH_OK;
  }

  int run() {
    int rc;
    if ((rc = prepare()) || (rc = coords(0))) return rc;
    HIPCHK(h, hipEventCreateWithFlags(&ev.sr_mark, hipEventDisableTiming));
    if (dbg) {
      HIPCHK(h, hipEventCreate(&ev.lt0));
      HIPCHK(h, hipEventCreate(&ev.lt1));
    }
    for (int k = 0; k < K; ++k) {
      HIPCHK(h, hipStreamWaitEvent(sr, h->seg_ev[(size_t)3 * k], 0));
      if ((rc = read_watchdog())) return rc;
      if (!late && (rc = coords_next(k))) return rc;
      if (!wd_fired && ((rc = start_loop(k)) || (rc = launch_loop(k)))) return rc;
      if (late && (rc = coords_next(k))) return rc;  // (wd_fired: every segment's receive is still posted)
      if (!wd_fired && (rc = resume_point(k))) return rc;
    }
    bool rerun = false;
    if (async && (rc = finish_async(&rerun))) return rc;
    if (!rerun && (rc = finish_watchdog(&rerun))) return rc;
    return rerun ? BH_OK : commit();
  }
};

}  // namespace

int rounds_pipelined(bh_handle *h, int K, int64_t base, const SplitPlan *sp, const std::vector<bh_handle *> *grp) {
  int rc;
  const PipelineModes m = pipeline_modes(h, sp);
  if (base > 0 && m.eager && h->rows_stale) {
    // the previous call left the prefix's rows unbuilt (a lazy-rows path)
    // and this one resumes on a path that reads them: build them first
    if ((rc = build_rows(h, h->lens_coord, h->stream))) return rc;
  }
  // (a coordinate shard's split_coords prepared the plan already)
  if (sp && !m.cshard && (rc = split_prepare(h, *sp, sp->total))) return rc;
  return SegmentPipeline(h, K, base, sp, grp, m).run();
}

// DivideRounds of one shard through the segment pipeline where it applies
// (*used = false otherwise, with nothing launched).  A call that only
// appended events resumes from the last one (the cost
// follows the new events)
int rounds_segmented(bh_handle *h, bool *used) {
  int rc;
  *used = false;
  Dev &d = h->d;
  d.N = (int64_t)h->h_creator.size();
  if (d.N == 0) return BH_OK;
  if ((rc = upload(h))) return rc;
  if ((rc = set_chain_tables(h, false))) return rc;
  const bool eligible = segments_eligible(h);
  const int64_t base = resume_base(h, d.N);
  if (getenv("BH_SEG_DEBUG") && atoi(getenv("BH_SEG_DEBUG")))
    fprintf(stderr, "[segments] N %lld eligible %d layout_changed %d inc_valid %d n_coord %lld reset %d E0 %lld\n",
            (long long)d.N, (int)eligible, (int)h->layout_changed, (int)h->inc_valid, (long long)h->n_coord,
            (int)h->reset_on, (long long)h->E0);
  if (!eligible) return BH_OK;
  // a Reset hashgraph's first call (and any call that brings events whose
  // other-parent only Root.Others knows) computes the whole DAG
  // (rounds_coords / rounds_loop: k_reset_coords, the fiat pass); the calls
  // after it append a segment like any other handle
  if (h->reset_on && (base == 0 || h->E0 > base)) return BH_OK;
  *used = true;
  d.rows = h->layout_rows;
  d.e0 = 0;
  d.seg_lo = h->seg_zero;
  if (base == d.N) {  // nothing new to divide: DivideRounds changes nothing
    h->stage = std::max(h->stage, 1);
    return BH_OK;
  }
  h->inc_calls += base > 0;
  return rounds_pipelined(h, h->reset_on ? 1 : segments_for(d, d.N - base), base);
}

int stage_rounds(bh_handle *h) {
  int rc;
  h->xchg_ms = 0;
  for (bh_handle *x : local_shards(h)) {
    x->loop_ms_acc = 0;
    x->tm_seg = x->tm_stages = false;  // (the last run's events are about to be reused: unread timings go)
  }
  if (h->split) return rounds_split_stage(h);
  if (!h->shard_cols) {
    // every shard holds the whole DAG and computes the same coordinates and
    // rounds: each runs the segment pipeline on its own device (one host
    // thread per shard of an in-process group), so a group is never slower
    // than one shard
    int nused = 0;
    std::vector<bh_handle *> sh = local_shards(h);
    std::vector<char> used(sh.size(), 0);
    rc = run_local(h, [&](bh_handle *x) {
      bool u = false;
      const int r = rounds_segmented(x, &u);
      for (size_t i = 0; i < sh.size(); ++i)
        if (sh[i] == x) used[i] = u;
      return r;
    });
    if (rc) return rc;
    for (char u : used) nused += u;
    if (nused == (int)sh.size()) return BH_OK;
    if (nused) return h->fail(BH_ERR_STATE, "shards disagree on the segment pipeline");
  }
  if ((rc = run_local(h, rounds_coords))) return rc;
  if (h->world > 1 && h->shard_cols && use_flow(h->d)) {
    // LA columns: shard r computed columns [col0, col0 + ncol), each a
    // contiguous (la_rows + 64)-int32 run of la_col
    const size_t colb = (size_t)(h->d.la_rows + 64) * 4;
    std::vector<size_t> off = range_bytes(h, h->d.n, colb, false), len = range_bytes(h, h->d.n, colb, true);
    if ((rc = exchange(h, [](bh_handle *x) -> void * { return x->d.la_col; }, off, len))) return rc;
  }
  return run_local(h, rounds_loop);
}
