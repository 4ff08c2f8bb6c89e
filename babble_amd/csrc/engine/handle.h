// handle.h -- host state of a libbabble_hip handle (internal; shared by
// api.cpp, the C ABI, passes and queries; rounds.cpp and split.cpp,
// DivideRounds' scheduling; frames.cpp, the block projection; sigpool.cpp).
#pragma once
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <chrono>
#include <cstdarg>
#include <cstdio>
#include <string>
#include <thread>
#include <unordered_map>
#include <vector>

#include "babble_hip.h"
#include "engine.h"

using bh::Dev;

namespace bh {

constexpr int ITER_BATCH = 32;  // round-loop iterations per graph replay
constexpr int ITER_FIRST = 4;   // ... for the first two replays of a loop (an incremental call needs a few rounds)
constexpr int NSTAGE = 5;

struct Block {
  int32_t rr;
  int64_t first, count, ntx;
};

// a multi-process group's exchange (comm.cpp): RCCL or the caller's host
// transport; device buffers, ordered on stream s
struct Comm {
  virtual ~Comm() = default;
  virtual int bcast(bh_handle *h, void *buf, size_t bytes, int32_t root, hipStream_t s) = 0;
  virtual int send(bh_handle *h, const void *buf, size_t bytes, int32_t peer, hipStream_t s) = 0;
  virtual int recv(bh_handle *h, void *buf, size_t bytes, int32_t peer, hipStream_t s) = 0;
  virtual int group_start(bh_handle *) { return 0; }  // (RCCL: receives from several peers at once)
  virtual int group_end(bh_handle *) { return 0; }
  // true: the calls wait on the host (the host transport); false: they are
  // enqueued on s and return (RCCL)
  virtual bool blocking() const { return false; }
};
Comm *make_rccl_comm(bh_handle *h, int32_t rank, int32_t world, const uint8_t *id);  // nullptr on failure (h->err)
Comm *make_host_comm(const bh_transport &t, int32_t rank);

}  // namespace bh

using bh::Block;
using bh::ITER_BATCH;
using bh::ITER_FIRST;
using bh::NSTAGE;

struct bh_handle {
  Dev d{};
  int device = 0;
  hipStream_t stream = nullptr;
  std::string err;
  int64_t cap = 0;
  // host mirrors (insert bookkeeping: ParticipantEventsCache + checks)
  std::vector<int64_t> pids;
  // participant ID -> slot: open addressing, power-of-two table >= 4n,
  // linear probing (one or two probes per lookup on the insert loop)
  std::vector<int64_t> slot_key;
  std::vector<int32_t> slot_val;
  uint64_t slot_mask = 0;
  int32_t slot_find(int64_t id) const {
    for (uint64_t i = ((uint64_t)id * 0x9E3779B97F4A7C15ull) >> 32 & slot_mask;; i = (i + 1) & slot_mask) {
      if (slot_val[i] < 0) return -1;
      if (slot_key[i] == id) return slot_val[i];
    }
  }
  std::vector<std::vector<int32_t>> chain;  // ids by creator, by index
  // per-chain prefix lengths at an insertion-order bound (chain_lens_at):
  // chains only grow by appends, so a bound's lengths never change once
  // every event below it is inserted -- kept, since each is n binary searches
  // over cold multi-MB id vectors (~250 us at C3 before the first loop)
  mutable std::unordered_map<int64_t, std::vector<int32_t>> lens_memo;
  std::vector<int32_t> h_creator, h_index, h_sp, h_op, h_ntx;
  std::vector<uint8_t> h_coin;
  std::vector<uint32_t> h_sigw;
  int64_t uploaded = 0;  // events already on the device
  int64_t loaded_total = 0;
  // The Go Hashgraph's state persists across calls: InsertEvent appends to
  // UndeterminedEvents and changes nothing else; each pass updates its own
  // part (hashgraph.go:714-1122).  The engine keeps the same split.
  //   n_div   events covered by the last DivideRounds (round / witness / LT)
  //   n_rr    events covered by the last DecideRoundReceived
  //   R       rounds (Store.LastRound() + 1)
  //   P       processed prefix: LastConsensusRound + 1
  //   pend_dec  PendingRounds' decided flags for rounds [P, R): sticky, as
  //             updatePendingRounds only ever sets them (hashgraph.go:689-695)
  int stage = 0;  // last pass run: 0 none, 1 rounds, 2 fame, 3 rr, 4 processed
  int coords_for = -1;  // N the device coordinates were computed for
  int64_t n_div = 0, n_rr = 0;
  int32_t R = 0, P = 0;
  std::vector<int8_t> pend_dec;     // indexed by round, meaningful for [P, R)
  std::vector<int8_t> decided_h;    // last fame pass: round r's witnesses all decided
  int64_t nundet = 0;               // undetermined among [0, n_rr) after the last rr pass
  int32_t R_rr = 0;                 // R at the last rr pass (frame_cnt covers [0, R_rr))
  int64_t ncons = 0, cons_txs = 0, cons_loaded = 0;
  std::vector<Block> blocks;
  // round-loop graph
  hipGraphExec_t graph = nullptr, graph_s = nullptr;  // ITER_BATCH / ITER_FIRST iterations
  Dev graph_dev{}, graph_dev_s{};
  int32_t *pinned_state = nullptr;
  // pinned staging for a pass's device-to-host reads (rd_async / rd_wait):
  // a pageable destination makes every hipMemcpyAsync a blocking staged copy
  uint8_t *pin_rd = nullptr;
  size_t pin_rd_cap = 0, pin_rd_used = 0;
  struct PinRead {
    void *dst;
    size_t off, bytes;
  };
  std::vector<PinRead> pin_rd_list;
  uint8_t *sha_buf = nullptr;  // bh_hash_bodies scratch
  uint8_t *q_buf = nullptr;    // bh_query_events scratch
  int32_t *pack_buf = nullptr;  // order_finish's read-back (k_pack_frames)
  size_t pack_cap = 0;          // (int32 words)
  size_t q_cap = 0;
  size_t sha_cap = 0;
  // fixed-key signature verification (bh_set_validators; sigpool.cpp)
  uint32_t *sig_tab = nullptr;  // windowed tables of the validators' keys and of G (kernels_sigpool.hip)
  int sig_window = 0;           // their window width in bits; 0 = no validators set
  uint8_t *sig_buf = nullptr;   // bh_verify_fixed scratch
  size_t sig_cap = 0;
  hipEvent_t ev_sig[2]{};       // around the last verify / table / pool kernels (bh_get_sig_stats)
  float verify_ms = 0, verify_fixed_ms = 0, tables_ms = 0, pool_ms = 0;
  // the block-signature pool (sigpool.cpp), allocated by its first use
  bh::SigPool sp{};
  bool sp_on = false;
  int64_t pool_count = 0, pool_cap = 0;
  int32_t *sp_blk_rr = nullptr;  // [sp_blk_cap] frame of each held block; sp_blk_up uploaded
  int64_t sp_blk_cap = 0, sp_blk_up = 0;
  uint8_t *sp_reset_shash = nullptr;  // [32 + 64] the Reset block's sign hash, bh_set_block_signature staging
  int32_t sp_reset_ver = -1;
  int64_t sig_verified = 0, sig_accepted = 0, sig_verified_total = 0, sig_anchor = -1;
  hipEvent_t ev[NSTAGE + 1]{};
  hipEvent_t ev_sweep[2]{};  // around k_la_sweep alone (roofline timing)
  hipEvent_t ev_loop[2]{};   // around each round loop (run_round_loop): its device time, summed per run
  hipEvent_t ev_st = nullptr;  // behind the loop state's read-back (SegmentPipeline: the witness tables run after it)
  bool fuse_fame = false;      // bh_run_consensus: DecideFame follows DivideRounds at once (rounds_tail)
  float loop_ms = 0, loop_ms_acc = 0;
  float sweep_ms = 0;
  const char *sweep_kernel = "";
  float stage_ms[NSTAGE]{};
  // timings of the last run not yet read from its events (settle_timings)
  bool tm_seg = false, tm_stages = false, tm_seg_loops = false, tm_seg_sp = false;
  int tm_seg_K = 0;
  int64_t iters = 0;
  int64_t *d_counters_host = nullptr;
  // segment pipeline: coordinates of prefix s + 1 on
  // stream2 while the round loop runs prefix s on `stream`
  hipStream_t stream2 = nullptr;
  std::vector<hipEvent_t> loop_evs;            // around each segment's loop launch (rounds_pipelined, async)
  int ncu = 256;                               // compute units of the device
  int32_t *seg_zero = nullptr;   // [n] zeros: seg_lo of a one-segment view
  int32_t *segbuf = nullptr;     // [2 parities][lo, len][n]
  int32_t *seg_stage = nullptr;  // pinned staging of the segments' [lo, len] rows, one per segment (<= 64)
  hipGraphExec_t seg_graph[2] = {nullptr, nullptr}, seg_graph_s[2] = {nullptr, nullptr};
  Dev seg_graph_dev[2]{}, seg_graph_dev_s[2]{};
  std::vector<hipEvent_t> seg_ev;  // per segment: coordinates done, k_flow32 start / end
  int32_t segments_used = 1;
  int32_t *tlist = nullptr, *tlist_stage = nullptr;  // [2 parities][tlist_cap] segment tile lists
  int64_t tlist_cap = 0;
  std::vector<int32_t> cstart_h;  // chain_start as uploaded
  std::vector<int32_t> cap_h;     // rows of each chain's region
  std::vector<int32_t> lens_h;    // chain lengths as uploaded
  int64_t layout_rows = 0;        // rows of the layout (regions included)
  bool layout_changed = true;
  // incremental calls (a call that only appended events runs them as one
  // more segment): coordinates and round loop hold the first n_coord events
  // of the current layout; lens_coord their chain lengths
  bool inc_valid = false;
  bool fdt_lost = false;  // the wide LT fallback's sweep overwrote FDT (no resume from it)
  bool rows_stale = false;  // n <= 128 segments built la_col only: row-major LA / FDT wait for a query
  // the row-major LA / FDT built (build_rows) for these chain lengths of the
  // current layout: a later build transposes only the rows past them
  bool rows_built = false;
  std::vector<int32_t> rows_lens;
  int64_t n_coord = 0;
  int64_t inc_calls = 0;  // DivideRounds calls that resumed (statistics)
  int64_t persist_loops = 0, persist_fallbacks = 0;  // k_round2p loops run / given up (bh_get_loop_stats)
  std::vector<int32_t> lens_coord;
  // sharding
  int32_t rank = 0, world = 1;
  std::vector<bh_handle *> group;  // in-process group: every shard (group[rank] == this); empty otherwise
  bh::Comm *xport = nullptr;       // multi-process group (bh_comm_init / bh_comm_init_transport)
  bool shard_cols = false;         // split the coordinate dataflow's LA columns (else every shard computes all)
  // the coordinate split (kernels_split.hip): shards
  // 1 .. G-1 run the dataflow for a range of LA columns each and ship every
  // segment's rows of them.  n <= 128 (split_all): the blocks are
  // all-gathered and EVERY shard runs the round loop on the full columns, so
  // fame rounds and frame sorts split between all shards as in the
  // replicated mode; 128 < n <= 512 (the wide split): shard 0 alone receives
  // them and runs the loop, fame and order
  bool split = false;
  bool split_all() const { return split && d.fd_cols; }
  uint8_t *xbuf = nullptr;        // every segment's blocks of every coordinate shard, at SplitPlan::boff
  size_t xcap = 0;
  int32_t *xseg = nullptr;        // [K][lo, hi][n] segment views, then [K][P, Q][n + 1] packing tables
  int32_t xseg_k = 0;             // segments xseg has room for
  std::vector<hipEvent_t> pack_ev;  // coordinate shard: segment k's own block packed (stream2)
  hipStream_t stream3 = nullptr;    // the split's receives and unpacks, beside the dataflow (stream2)
  hipEvent_t xprep = nullptr;       // the call's chain tables prepared (stream2), before any unpack
  int32_t *xbase = nullptr;       // multi-process: rank 0's base for the call (broadcast)
  float xchg_ms = 0;               // exchange time of the last pass sequence (host wall, incl. waits)
  std::vector<int32_t> wofs_h;     // [R + 1] witness offsets (fame exchange ranges; launch size)
  std::vector<int32_t> fofs_h;     // [P + 1] frame offsets (order exchange ranges)
  // block projection (bh_config.frames; frames.cpp)
  bool frames_on = false;
  bh::Frames fr{};
  std::vector<uint8_t> h_hash;     // hashes of events inserted but not yet uploaded
  int64_t arena_cap = 0, arena_len = 0;
  int64_t others_total = 0;        // Others of the processed frames (oofs[P * n])
  size_t json_cap = 0, bjson_cap = 0;
  uint8_t *host_json = nullptr;  // pinned host copy of the JSON a call hashes on the host (frames.cpp)
  size_t host_json_cap = 0;
  int64_t hash_host_frames = 0;  // frames whose FrameHash the host computed (statistics)
  hipEvent_t ev_fr[2]{};           // around the last projection
  float frames_ms = 0;

  // Reset / FastSync roots (bh_reset; hashgraph.go:1324-1369).  Chains
  // start at base_h[c] = Root.SelfParent.Index + 1; Root.Others entries are
  // found by (root slot, key hash) and by (root slot, creator slot, Index)
  bool reset_on = false;
  int32_t reset_lcr = -1;      // block.RoundReceived(): LastConsensusRound after Reset
  int64_t reset_block = -1;    // block.Index(): LastBlockIndex after Reset
  int32_t reset_F = -1;        // highest NextRound / SelfParent.Round of a root
  std::vector<int32_t> base_h, next_h, sp_round_h, sp_lt_h;
  struct Other {
    int32_t root, creator, index, lt, round;
    uint8_t key[32], hash[32];
  };
  std::vector<Other> others;
  std::unordered_map<std::string, int32_t> oth_by_key;  // root slot bytes + key hash -> entry
  std::unordered_map<uint64_t, int32_t> oth_by_index;   // (root slot, creator slot, Index) -> entry
  std::vector<uint8_t> h_hashes;                        // every event's hash (Others matching)
  std::vector<int8_t> h_rflag;                          // Dev::rflag
  std::vector<int32_t> h_ext_lt;                        // Dev::ext_lt
  std::vector<int32_t> h_oth;                           // Frames::oth_of (frames on)
  int64_t E0 = 0;  // events [0, E0) hold every other-parent only Root.Others knows
  int32_t fiat_max = -1;

  // test hook: BH_TEST_FAIL_ALLOC=k makes the k-th device allocation of a
  // bh_reset call fail (tests check that a failed call leaves the handle as
  // it was); -1 otherwise
  int fail_alloc_in = -1;

  // a coordinate rank of a multi-process WIDE split group: it ran no
  // consensus pass, so it holds no results (rank 0 does)
  bool no_results() const { return split && !split_all() && rank > 0 && xport != nullptr; }
  int fail(int code, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    err = buf;
    return code;
  }
};

#define HIPCHK(h, call)                                                              \
  do {                                                                               \
    hipError_t e_ = (call);                                                          \
    if (e_ != hipSuccess)                                                            \
      return (h)->fail(BH_ERR_DEVICE, "%s: %s (%s:%d)", #call, hipGetErrorString(e_), \
                       __FILE__, __LINE__);                                          \
  } while (0)

template <class T>
inline int dalloc(bh_handle *h, T **p, size_t count) {
  if (h->fail_alloc_in >= 0 && h->fail_alloc_in-- == 0) {  // test hook (bh_reset, BH_TEST_FAIL_ALLOC)
    *p = nullptr;
    return h->fail(BH_ERR_DEVICE, "injected allocation failure");
  }
  HIPCHK(h, hipMalloc((void **)p, std::max<size_t>(count, 1) * sizeof(T)));
  return BH_OK;
}

// sigpool.cpp
void sig_free(bh_handle *h);
void sig_pool_forget(bh_handle *h);  // bh_reset_consensus: signatures, anchor and pool go with the blocks
int sig_events(bh_handle *h);  // creates ev_sig on first use

// frames.cpp
int frames_alloc(bh_handle *h);
void frames_free(bh_handle *h);
// the projection's device tables for R1 rounds into fr (with a Reset's K
// installed Others entries: reset); frames_init gives them their initial
// contents once they are the handle's
int frames_alloc_tables(bh_handle *h, bh::Frames &fr, int64_t R1, int64_t K, bool reset);
void frames_free_tables(bh::Frames &fr);
int frames_init(bh_handle *h);
int frames_prepare(bh_handle *h, bh::Frames &fr, int64_t R1, size_t *json_cap, size_t *bjson_cap);
void frames_reset(bh_handle *h);
// roots, FrameHash and block hashes of the frames [P0, P1) just processed
// (consensus positions [i0, i1))
int frames_project(bh_handle *h, int32_t P0, int32_t P1, int64_t i0, int64_t i1);

// api.cpp: host helpers the passes share
int upload(bh_handle *h);  // events inserted since the last upload
hipError_t wait_stream(hipStream_t s);
hipError_t copy_sync(hipStream_t s, void *dst, const void *src, size_t bytes, hipMemcpyKind kind);
int rd_async(bh_handle *h, hipStream_t s, void *dst, const void *src, size_t bytes);
int rd_wait(bh_handle *h, hipStream_t s);
int rd_wait_event(bh_handle *h, hipEvent_t e);
void settle_timings(bh_handle *h);
std::vector<size_t> range_bytes(const bh_handle *h, int64_t items, size_t esz, bool lengths,
                                const std::vector<int32_t> *ofs = nullptr, int64_t base = 0);

// shards: ranges, local execution, exchanges

// [lo, hi) of `items` owned by shard `rank` of `world`: contiguous, sizes
// differ by at most one (bh_shard_range exposes it to the tests)
inline void shard_range(int64_t items, int32_t world, int32_t rank, int64_t *lo, int64_t *hi) {
  *lo = items * rank / world;
  *hi = items * (rank + 1) / world;
}

// the shards this process drives for handle h
inline std::vector<bh_handle *> local_shards(bh_handle *h) {
  return h->group.empty() ? std::vector<bh_handle *>{h} : h->group;
}

// run fn on every local shard: one host thread per shard of an in-process
// group (each on its own device and stream; the round loop polls its device
// from the host), inline otherwise.  The first failure is reported on h.
template <class F>
int run_local(bh_handle *h, F fn) {
  if (h->group.size() <= 1) return fn(h);
  const size_t G = h->group.size();
  std::vector<int> rc(G, BH_OK);
  std::vector<std::thread> th;
  for (size_t i = 0; i < G; ++i)
    th.emplace_back([&, i] {
      bh_handle *s = h->group[i];
      if (hipSetDevice(s->device) != hipSuccess) { rc[i] = s->fail(BH_ERR_DEVICE, "hipSetDevice"); return; }
      rc[i] = fn(s);
    });
  for (auto &t : th) t.join();
  for (size_t i = 0; i < G; ++i)
    if (rc[i] != BH_OK) {
      if (h->group[i] != h) h->err = "shard " + std::to_string(i) + ": " + h->group[i]->err;
      (void)hipSetDevice(h->device);
      return rc[i];
    }
  (void)hipSetDevice(h->device);
  return BH_OK;
}

// All-gather of per-shard byte ranges of one device buffer (same layout on
// every shard): shard r owns [off[r], off[r] + len[r]) of the buffer `sel`
// selects; afterwards every shard holds every range.  In-process: each
// shard's stream waits for the owner's work, then peer-copies the range
// (xGMI between devices, a device copy on a shared one).  Across processes:
// one ncclBroadcast per owner, in place, grouped.
template <class Sel>
int exchange(bh_handle *h, Sel sel, const std::vector<size_t> &off, const std::vector<size_t> &len) {
  if (h->world <= 1) return BH_OK;
  const auto t0 = std::chrono::steady_clock::now();
  if (h->xport) {
    uint8_t *base = reinterpret_cast<uint8_t *>(sel(h));
    int rc;
    if ((rc = h->xport->group_start(h))) return rc;
    for (int r = 0; r < h->world; ++r)
      if (len[r] && (rc = h->xport->bcast(h, base + off[r], len[r], r, h->stream))) {
        (void)h->xport->group_end(h);
        return rc;
      }
    if ((rc = h->xport->group_end(h))) return rc;
    HIPCHK(h, wait_stream(h->stream));
  } else {
    const size_t G = h->group.size();
    std::vector<hipEvent_t> ready(G);
    for (size_t r = 0; r < G; ++r) {
      bh_handle *o = h->group[r];
      HIPCHK(h, hipSetDevice(o->device));
      HIPCHK(h, hipEventCreateWithFlags(&ready[r], hipEventDisableTiming));
      HIPCHK(h, hipEventRecord(ready[r], o->stream));
    }
    for (size_t t = 0; t < G; ++t) {
      bh_handle *dst = h->group[t];
      HIPCHK(h, hipSetDevice(dst->device));
      uint8_t *db = reinterpret_cast<uint8_t *>(sel(dst));
      for (size_t r = 0; r < G; ++r) {
        if (r == t || !len[r]) continue;
        bh_handle *src = h->group[r];
        HIPCHK(h, hipStreamWaitEvent(dst->stream, ready[r], 0));
        HIPCHK(h, hipMemcpyPeerAsync(db + off[r], dst->device, reinterpret_cast<uint8_t *>(sel(src)) + off[r],
                                     src->device, len[r], dst->stream));
      }
    }
    for (size_t t = 0; t < G; ++t) {
      HIPCHK(h, hipSetDevice(h->group[t]->device));
      HIPCHK(h, wait_stream(h->group[t]->stream));
      (void)hipEventDestroy(ready[t]);
    }
    HIPCHK(h, hipSetDevice(h->device));
  }
  h->xchg_ms += std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
  return BH_OK;
}

// rounds.cpp: DivideRounds' host scheduling
int stage_rounds(bh_handle *h);
int set_chain_tables(bh_handle *h, bool wait = true);
bool use_flow(const Dev &d);
int ensure_fd(bh_handle *h);
int reset_coords(bh_handle *h, hipStream_t s);
int build_rows(bh_handle *h, const std::vector<int32_t> &upto, hipStream_t s);
int rounds_coords(bh_handle *h);
int rounds_loop(bh_handle *h);
int rounds_segmented(bh_handle *h, bool *used);
int segments_for(const Dev &d, int64_t events);
double seg_ratio(const Dev &d);
void chain_lens_at(const bh_handle *h, int64_t bound, int32_t *out);
// events of the current layout an incremental call keeps (0: a full call)
inline int64_t resume_base(const bh_handle *h, int64_t N) {
  return (!h->layout_changed && h->inc_valid && N >= h->n_coord) ? h->n_coord : 0;
}
// the resume bookkeeping after a call's coordinates: the device holds those
// of the first N events of the current layout (lens_h their chain lengths);
// valid: the next call may resume from them (else rounds_tail's LT fallback
// overwrote FDT and dropped coords_for)
inline void commit_coords(bh_handle *h, int64_t N, bool valid) {
  if (valid) h->coords_for = (int)N;
  h->n_coord = N;
  h->lens_coord = h->lens_h;
  h->inc_valid = valid;
}
// segment k of a call cut at Ns: events [Ns[k], Ns[k + 1]), its chain ranges
// [lo | len][n] at lens (device)
inline Dev segment_view(const bh_handle *h, const Dev &d, int32_t *lens, const int64_t *Ns, int k) {
  Dev v = d;
  v.seg_lo = lens;
  v.chain_len = lens + d.n;
  v.N = Ns[k + 1];
  v.e0 = Ns[k];
  v.rows = h->layout_rows;
  return v;
}
int ensure_events(bh_handle *h, std::vector<hipEvent_t> &v, size_t count, unsigned flags);  // grow v to count events

// split.cpp: the coordinate split.  One call's segments, alike on every
// shard: boundaries, each segment's chain ranges [lo, hi) and packing tables
// P (rows before chain c) and Q (64-row chunks before chain c), the blocks'
// sizes
struct SplitPlan {
  int K = 0;
  int64_t base = 0;
  std::vector<int64_t> Ns, S, NQ;
  std::vector<int32_t> tab;  // [K][lo, hi][n], then [K][P, Q][n + 1]
  // block (k, r) at byte offset off[k * world + r] of every shard's xbuf
  // (segment-major, then coordinate rank): one layout everywhere, so a
  // block is broadcast in place and peer-copied offset to offset
  std::vector<size_t> off;
  size_t total = 0;
  size_t boff(const bh_handle *h, int k, int32_t rank) const { return off[(size_t)k * h->world + rank]; }
  int32_t *dview(const bh_handle *h, int k) const { return h->xseg + (size_t)k * 2 * h->d.n; }
  const int32_t *dpq(const bh_handle *h, int k) const {
    return h->xseg + (size_t)K * 2 * h->d.n + (size_t)k * 2 * (h->d.n + 1);
  }
  size_t block_bytes(const bh_handle *h, int k, int32_t rank) const;
  bh::SplitBlock block(const bh_handle *h, int k, int32_t rank, uint8_t *at) const;
};
int split_prepare(bh_handle *x, const SplitPlan &p, size_t bytes);
int rounds_split_stage(bh_handle *h);
// the segment pipeline (rounds.cpp) over K segments from base; sp / grp: the
// split's plan and in-process group
int rounds_pipelined(bh_handle *h, int K, int64_t base, const SplitPlan *sp = nullptr,
                     const std::vector<bh_handle *> *grp = nullptr);
