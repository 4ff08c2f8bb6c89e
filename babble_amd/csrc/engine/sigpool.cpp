// sigpool.cpp -- block-signature verification against the handle's
// validators (host side; the kernels are in kernels_sigpool.hip).
//
// Reference: Block.Verify (block.go:234-254) as ProcessSigPool
// (hashgraph.go:1236-1300) and CheckBlock (hashgraph.go:1483-1497) call it for
// signatures of participants.  bh_set_validators tabulates the participants'
// public keys once; bh_verify_fixed then runs ecdsa.Verify through the tables.
#include <openssl/bn.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "babble_hip.h"
#include "engine.h"
#include "handle.h"

void sig_free(bh_handle *h) {
  if (h->sig_tab) (void)hipFree(h->sig_tab);
  if (h->sig_buf) (void)hipFree(h->sig_buf);
  for (auto &e : h->ev_sig)
    if (e) (void)hipEventDestroy(e);
  h->sig_tab = nullptr;
  h->sig_buf = nullptr;
  h->sig_cap = 0;
  h->sig_window = 0;
  bh::SigPool &sp = h->sp;
  void *ptrs[] = {sp.set, sp.rs, sp.cnt, sp.winner, sp.misc, sp.val, sp.val2, sp.blk, sp.blk2, sp.prs, sp.prs2,
                  sp.seen, sp.seen2, sp.row, sp.stat, h->sp_blk_rr, h->sp_reset_shash};
  for (void *p : ptrs)
    if (p) (void)hipFree(p);
  sp = bh::SigPool{};
  h->sp_blk_rr = nullptr;
  h->sp_reset_shash = nullptr;
  h->sp_on = false;
  h->pool_count = h->pool_cap = h->sp_blk_cap = h->sp_blk_up = 0;
}

// bh_reset_consensus: the blocks are cut again, so their signatures, the
// anchor and the pool go (the caller adds the signatures again); the Reset
// block and its sign hash belong to bh_reset and stay
void sig_pool_forget(bh_handle *h) {
  h->pool_count = 0;
  h->sp_blk_up = 0;
  h->sig_anchor = -1;
  h->sig_verified = h->sig_accepted = 0;
  if (!h->sp_on) return;
  bh::SigPool &sp = h->sp;
  const size_t rows = (size_t)sp.R1 + 1;
  (void)hipMemsetAsync(sp.set, 0, rows * sp.n, h->stream);
  (void)hipMemsetAsync(sp.cnt, 0, rows * 4, h->stream);
  (void)hipMemsetAsync(sp.misc, 0, 4 * 8, h->stream);
}

int sig_events(bh_handle *h) {
  for (auto &e : h->ev_sig)
    if (!e) HIPCHK(h, hipEventCreate(&e));
  return BH_OK;
}

namespace {

// y^2 == x^3 - 3 x + b (mod p) with x, y < p, for each of the n points; the
// index of the first point that fails, -1 if none (-2: out of memory)
int first_off_curve(const uint8_t *pub, int32_t n) {
  static const char *P_HEX = "FFFFFFFF00000001000000000000000000000000FFFFFFFFFFFFFFFFFFFFFFFF";
  static const char *B_HEX = "5AC635D8AA3A93E7B3EBBD55769886BC651D06B0CC53B0F63BCE3C3E27D2604B";
  BN_CTX *ctx = BN_CTX_new();
  BIGNUM *p = nullptr, *b = nullptr;
  BIGNUM *x = BN_new(), *y = BN_new(), *l = BN_new(), *r = BN_new(), *t = BN_new();
  int bad = -1;
  if (!ctx || !x || !y || !l || !r || !t || !BN_hex2bn(&p, P_HEX) || !BN_hex2bn(&b, B_HEX)) bad = -2;
  for (int32_t i = 0; i < n && bad == -1; ++i) {
    const uint8_t *k = pub + 64 * (size_t)i;
    if (!BN_bin2bn(k, 32, x) || !BN_bin2bn(k + 32, 32, y)) {
      bad = -2;
    } else if (BN_cmp(x, p) >= 0 || BN_cmp(y, p) >= 0) {
      bad = i;
    } else if (!BN_mod_sqr(l, y, p, ctx) || !BN_mod_sqr(r, x, p, ctx) || !BN_mod_mul(r, r, x, p, ctx) ||
               !BN_mod_add(t, x, x, p, ctx) || !BN_mod_add(t, t, x, p, ctx) || !BN_mod_sub(r, r, t, p, ctx) ||
               !BN_mod_add(r, r, b, p, ctx)) {
      bad = -2;
    } else if (BN_cmp(l, r) != 0) {
      bad = i;
    }
  }
  BN_free(x), BN_free(y), BN_free(l), BN_free(r), BN_free(t), BN_free(p), BN_free(b);
  BN_CTX_free(ctx);
  return bad;
}

bool sharded(const bh_handle *h) { return !h->group.empty() || h->world > 1; }

}  // namespace

extern "C" {

int bh_set_validators(bh_handle *h, const uint8_t *pubkeys) {
  if (!h) return BH_ERR_INVALID;
  if (!pubkeys) return h->fail(BH_ERR_INVALID, "bh_set_validators: null pubkeys");
  if (sharded(h)) return h->fail(BH_ERR_STATE, "bh_set_validators: one shard (block signatures are not sharded)");
  const int32_t n = h->d.n;
  const int bad = first_off_curve(pubkeys, n);
  if (bad == -2) return h->fail(BH_ERR_INVALID, "bh_set_validators: out of memory");
  if (bad >= 0) return h->fail(BH_ERR_INVALID, "bh_set_validators: key %d is not a point of P-256", bad);
  // BH_SIG_WINDOW: 4 or 8 bits per table window (measurement; read per call)
  int window = 8;
  if (const char *e = getenv("BH_SIG_WINDOW")) window = atoi(e);
  if (window != 4 && window != 8) return h->fail(BH_ERR_INVALID, "BH_SIG_WINDOW must be 4 or 8");
  (void)hipSetDevice(h->device);
  HIPCHK(h, hipStreamSynchronize(h->stream));
  if (h->sig_tab) (void)hipFree(h->sig_tab);
  h->sig_tab = nullptr;
  h->sig_window = 0;
  if (int rc = sig_events(h)) return rc;
  uint8_t *dpub = nullptr;
  HIPCHK(h, hipMalloc((void **)&h->sig_tab, bh::fixed_table_bytes(n, window)));
  if (hipMalloc((void **)&dpub, (size_t)n * 64) != hipSuccess) {
    (void)hipFree(h->sig_tab);
    h->sig_tab = nullptr;
    return h->fail(BH_ERR_DEVICE, "bh_set_validators: allocation failed");
  }
  hipError_t e = hipMemcpyAsync(dpub, pubkeys, (size_t)n * 64, hipMemcpyHostToDevice, h->stream);
  if (e == hipSuccess) e = hipEventRecord(h->ev_sig[0], h->stream);
  if (e == hipSuccess) {
    bh::launch_fixed_tables(dpub, n, window, h->sig_tab, h->stream);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipEventRecord(h->ev_sig[1], h->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
  if (e == hipSuccess) e = hipEventElapsedTime(&h->tables_ms, h->ev_sig[0], h->ev_sig[1]);
  (void)hipFree(dpub);
  if (e != hipSuccess) {
    (void)hipFree(h->sig_tab);
    h->sig_tab = nullptr;
    return h->fail(BH_ERR_DEVICE, "bh_set_validators: %s", hipGetErrorString(e));
  }
  h->sig_window = window;
  return BH_OK;
}

int bh_verify_fixed(bh_handle *h, const uint8_t *hashes, const uint8_t *sig_r, const uint8_t *sig_s,
                    const int32_t *validator, int64_t count, uint8_t *ok) {
  if (!h) return BH_ERR_INVALID;
  if (sharded(h)) return h->fail(BH_ERR_STATE, "bh_verify_fixed: one shard (block signatures are not sharded)");
  if (!h->sig_window) return h->fail(BH_ERR_STATE, "bh_verify_fixed before bh_set_validators");
  if (count < 0 || (count > 0 && (!hashes || !sig_r || !sig_s || !validator || !ok)))
    return h->fail(BH_ERR_INVALID, "bh_verify_fixed: null buffer or bad count");
  if (count == 0) return BH_OK;
  const int32_t n = h->d.n;
  for (int64_t i = 0; i < count; ++i)
    if (validator[i] < 0 || validator[i] >= n)
      return h->fail(BH_ERR_INVALID, "bh_verify_fixed: validator slot out of range");
  (void)hipSetDevice(h->device);
  const size_t need = (size_t)count * (3 * 32 + 4 + 1) + 64;
  if (need > h->sig_cap) {
    if (h->sig_buf) (void)hipFree(h->sig_buf);
    h->sig_buf = nullptr;
    h->sig_cap = 0;
    HIPCHK(h, hipMalloc((void **)&h->sig_buf, need));
    h->sig_cap = need;
  }
  uint8_t *dh = h->sig_buf, *dr = dh + count * 32, *ds = dr + count * 32;
  int32_t *dv = reinterpret_cast<int32_t *>(ds + count * 32);
  uint8_t *dok = reinterpret_cast<uint8_t *>(dv + count);
  HIPCHK(h, hipMemcpyAsync(dh, hashes, (size_t)count * 32, hipMemcpyHostToDevice, h->stream));
  HIPCHK(h, hipMemcpyAsync(dr, sig_r, (size_t)count * 32, hipMemcpyHostToDevice, h->stream));
  HIPCHK(h, hipMemcpyAsync(ds, sig_s, (size_t)count * 32, hipMemcpyHostToDevice, h->stream));
  HIPCHK(h, hipMemcpyAsync(dv, validator, (size_t)count * 4, hipMemcpyHostToDevice, h->stream));
  HIPCHK(h, hipEventRecord(h->ev_sig[0], h->stream));
  bh::launch_verify_fixed(dh, dr, ds, dv, n, h->sig_window, h->sig_tab, count, dok, h->stream);
  HIPCHK(h, hipGetLastError());
  HIPCHK(h, hipEventRecord(h->ev_sig[1], h->stream));
  HIPCHK(h, hipMemcpyAsync(ok, dok, (size_t)count, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  HIPCHK(h, hipEventElapsedTime(&h->verify_fixed_ms, h->ev_sig[0], h->ev_sig[1]));
  return BH_OK;
}

}  // extern "C"

namespace {

template <class T>
int regrow(bh_handle *h, T **p, size_t old_count, size_t new_count, size_t per) {
  T *q = nullptr;
  HIPCHK(h, hipMalloc((void **)&q, std::max<size_t>(new_count * per, 1) * sizeof(T)));
  if (*p && old_count)
    HIPCHK(h, hipMemcpyAsync(q, *p, old_count * per * sizeof(T), hipMemcpyDeviceToDevice, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  if (*p) (void)hipFree(*p);
  *p = q;
  return BH_OK;
}

// the pool's entry checks and its tables (allocated by the first call; sized
// again if bh_reset changed the round capacity)
int pool_ready(bh_handle *h, const char *who) {
  if (sharded(h) || h->no_results())
    return h->fail(BH_ERR_STATE, "%s: one shard (block signatures are not sharded)", who);
  if (!h->frames_on) return h->fail(BH_ERR_STATE, "%s: the handle was created without frames", who);
  (void)hipSetDevice(h->device);
  bh::SigPool &sp = h->sp;
  const int32_t n = h->d.n, R1 = h->d.R_cap + 1;
  if (h->sp_on && sp.R1 == R1) return BH_OK;
  HIPCHK(h, hipStreamSynchronize(h->stream));
  void *old[] = {sp.set, sp.rs, sp.cnt, sp.winner, sp.misc};
  for (void *p : old)
    if (p) (void)hipFree(p);
  sp.set = nullptr, sp.rs = nullptr, sp.cnt = nullptr, sp.winner = nullptr, sp.misc = nullptr;
  h->sp_on = false;
  const size_t rows = (size_t)R1 + 1, cells = rows * (size_t)n;
  HIPCHK(h, hipMalloc((void **)&sp.set, cells));
  HIPCHK(h, hipMalloc((void **)&sp.rs, cells * 64));
  HIPCHK(h, hipMalloc((void **)&sp.cnt, rows * 4));
  HIPCHK(h, hipMalloc((void **)&sp.winner, cells * 4));
  HIPCHK(h, hipMalloc((void **)&sp.misc, 4 * 8));
  if (!h->sp_reset_shash) HIPCHK(h, hipMalloc((void **)&h->sp_reset_shash, 96));
  HIPCHK(h, hipMemset(sp.set, 0, cells));
  HIPCHK(h, hipMemset(sp.cnt, 0, rows * 4));
  HIPCHK(h, hipMemset(sp.winner, 0xff, cells * 4));
  HIPCHK(h, hipMemset(sp.misc, 0, 4 * 8));
  sp.n = n;
  sp.R1 = R1;
  sp.trust = (n + 2) / 3;  // ceil(n / 3), hashgraph.go:55
  h->sp_on = true;
  h->sig_anchor = -1;
  return BH_OK;
}

// the row of the signature tables of block `b` (BlockSignature.Index), -1 if
// the handle does not hold it
int32_t block_row(const bh_handle *h, int64_t b) {
  const int64_t first = h->reset_on ? h->reset_block + 1 : 0, k = b - first;
  if (k >= 0 && k < (int64_t)h->blocks.size()) return h->blocks[(size_t)k].rr;
  if (h->reset_on && b == h->reset_block) return h->sp.R1;
  return -1;
}

}  // namespace

extern "C" {

int bh_add_block_signatures(bh_handle *h, int64_t count, const int32_t *validator, const int64_t *block_index,
                            const uint8_t *sig_r, const uint8_t *sig_s) {
  if (!h) return BH_ERR_INVALID;
  if (int rc = pool_ready(h, "bh_add_block_signatures")) return rc;
  if (count < 0 || (count > 0 && (!validator || !block_index || !sig_r || !sig_s)))
    return h->fail(BH_ERR_INVALID, "bh_add_block_signatures: null buffer or bad count");
  if (count == 0) return BH_OK;
  const int32_t n = h->d.n;
  for (int64_t i = 0; i < count; ++i)
    if (validator[i] < -1 || validator[i] >= n)
      return h->fail(BH_ERR_INVALID, "bh_add_block_signatures: validator slot out of range");
  if (h->pool_count + count > INT32_MAX) return h->fail(BH_ERR_CAPACITY, "bh_add_block_signatures: pool too large");
  bh::SigPool &sp = h->sp;
  const int64_t need = h->pool_count + count;
  if (need > h->pool_cap) {
    const size_t oc = (size_t)h->pool_count, nc = (size_t)std::max<int64_t>(need, 2 * h->pool_cap + 1024);
    int rc = BH_OK;
    if (!rc) rc = regrow(h, &sp.val, oc, nc, 1);
    if (!rc) rc = regrow(h, &sp.blk, oc, nc, 1);
    if (!rc) rc = regrow(h, &sp.prs, oc, nc, 64);
    if (!rc) rc = regrow(h, &sp.seen, oc, nc, 1);
    if (!rc) rc = regrow(h, &sp.val2, 0, nc, 1);
    if (!rc) rc = regrow(h, &sp.blk2, 0, nc, 1);
    if (!rc) rc = regrow(h, &sp.prs2, 0, nc, 64);
    if (!rc) rc = regrow(h, &sp.seen2, 0, nc, 1);
    if (!rc) rc = regrow(h, &sp.row, 0, nc, 1);
    if (!rc) rc = regrow(h, &sp.stat, 0, nc, 1);
    if (rc) return rc;
    h->pool_cap = (int64_t)nc;
  }
  std::vector<uint8_t> rs((size_t)count * 64);
  for (int64_t i = 0; i < count; ++i) {
    memcpy(rs.data() + 64 * i, sig_r + 32 * i, 32);
    memcpy(rs.data() + 64 * i + 32, sig_s + 32 * i, 32);
  }
  const int64_t at = h->pool_count;
  hipStream_t s = h->stream;
  HIPCHK(h, hipMemcpyAsync(sp.val + at, validator, (size_t)count * 4, hipMemcpyHostToDevice, s));
  HIPCHK(h, hipMemcpyAsync(sp.blk + at, block_index, (size_t)count * 8, hipMemcpyHostToDevice, s));
  HIPCHK(h, hipMemcpyAsync(sp.prs + 64 * at, rs.data(), rs.size(), hipMemcpyHostToDevice, s));
  HIPCHK(h, hipMemsetAsync(sp.seen + at, 0xff, (size_t)count * 4, s));
  HIPCHK(h, hipStreamSynchronize(s));
  h->pool_count = need;
  return BH_OK;
}

int bh_set_block_signature(bh_handle *h, int64_t block, int32_t validator, const uint8_t *r, const uint8_t *s) {
  if (!h) return BH_ERR_INVALID;
  if (int rc = pool_ready(h, "bh_set_block_signature")) return rc;
  if (!r || !s || validator < 0 || validator >= h->d.n)
    return h->fail(BH_ERR_INVALID, "bh_set_block_signature: null buffer or validator slot out of range");
  const int32_t row = block_row(h, block);
  if (row < 0) return h->fail(BH_ERR_KEY_NOT_FOUND, "GetBlock(%lld): no such block", (long long)block);
  uint8_t rs[64];
  memcpy(rs, r, 32);
  memcpy(rs + 32, s, 32);
  HIPCHK(h, hipMemcpyAsync(h->sp_reset_shash + 32, rs, 64, hipMemcpyHostToDevice, h->stream));
  bh::launch_sig_set(h->sp, row, validator, h->sp_reset_shash + 32, h->stream);
  HIPCHK(h, hipGetLastError());
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return BH_OK;
}

int bh_set_reset_block_sign_hash(bh_handle *h, const uint8_t *hash32) {
  if (!h) return BH_ERR_INVALID;
  if (!hash32) return h->fail(BH_ERR_INVALID, "bh_set_reset_block_sign_hash: null hash");
  if (!h->reset_on || h->reset_block < 0)
    return h->fail(BH_ERR_STATE, "bh_set_reset_block_sign_hash: the handle holds no Reset block");
  if (int rc = pool_ready(h, "bh_set_reset_block_sign_hash")) return rc;
  HIPCHK(h, hipMemcpyAsync(h->sp_reset_shash, hash32, 32, hipMemcpyHostToDevice, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  h->sp_reset_ver += 1;
  return BH_OK;
}

int bh_process_sig_pool(bh_handle *h, int64_t *accepted, int64_t *remaining) {
  if (!h) return BH_ERR_INVALID;
  if (int rc = pool_ready(h, "bh_process_sig_pool")) return rc;
  if (!h->sig_window) return h->fail(BH_ERR_STATE, "bh_process_sig_pool before bh_set_validators");
  bh::SigPool &sp = h->sp;
  hipStream_t s = h->stream;
  // the frame of every block cut since the last call (per block, not per signature)
  const int64_t nb = (int64_t)h->blocks.size();
  if (nb > h->sp_blk_cap) {
    if (int rc = regrow(h, &h->sp_blk_rr, (size_t)h->sp_blk_up, (size_t)std::max<int64_t>(nb, 2 * h->sp_blk_cap + 256), 1))
      return rc;
    h->sp_blk_cap = std::max<int64_t>(nb, 2 * h->sp_blk_cap + 256);
  }
  if (nb > h->sp_blk_up) {
    std::vector<int32_t> rr((size_t)(nb - h->sp_blk_up));
    for (int64_t k = h->sp_blk_up; k < nb; ++k) rr[(size_t)(k - h->sp_blk_up)] = h->blocks[(size_t)k].rr;
    HIPCHK(h, hipMemcpyAsync(h->sp_blk_rr + h->sp_blk_up, rr.data(), rr.size() * 4, hipMemcpyHostToDevice, s));
    HIPCHK(h, hipStreamSynchronize(s));
    h->sp_blk_up = nb;
  }
  sp.window = h->sig_window;
  sp.tab = h->sig_tab;
  sp.blk_rr = h->sp_blk_rr;
  sp.first_block = h->reset_on ? h->reset_block + 1 : 0;
  sp.nblocks = nb;
  sp.reset_block = h->reset_on ? h->reset_block : -1;
  sp.reset_shash = h->sp_reset_shash;
  sp.reset_ver = h->sp_reset_ver;
  if (int rc = sig_events(h)) return rc;
  HIPCHK(h, hipEventRecord(h->ev_sig[0], s));
  bh::launch_sig_pool_pass(h->fr, sp, h->pool_count, s);
  HIPCHK(h, hipGetLastError());
  HIPCHK(h, hipEventRecord(h->ev_sig[1], s));
  int64_t misc[4] = {0, 0, 0, 0};  // the one read-back
  HIPCHK(h, hipMemcpyAsync(misc, sp.misc, sizeof misc, hipMemcpyDeviceToHost, s));
  HIPCHK(h, hipStreamSynchronize(s));
  HIPCHK(h, hipEventElapsedTime(&h->pool_ms, h->ev_sig[0], h->ev_sig[1]));
  if (h->pool_count > 0 && misc[1] > 0) {  // the survivors are in the second buffers
    std::swap(sp.val, sp.val2);
    std::swap(sp.blk, sp.blk2);
    std::swap(sp.prs, sp.prs2);
    std::swap(sp.seen, sp.seen2);
    h->pool_count = misc[3];
  }
  h->sig_anchor = misc[0] - 1;
  h->sig_accepted = misc[1];
  h->sig_verified = misc[2];
  h->sig_verified_total += misc[2];
  if (accepted) *accepted = misc[1];
  if (remaining) *remaining = h->pool_count;
  return BH_OK;
}

int64_t bh_get_block_signature_counts(bh_handle *h, int64_t first, int64_t count, int32_t *counts) {
  if (!h) return -BH_ERR_INVALID;
  if (int rc = pool_ready(h, "bh_get_block_signature_counts")) return -rc;
  const int64_t nb = (int64_t)h->blocks.size();
  if (first < 0 || count < 0 || first + count > nb)
    return -h->fail(BH_ERR_INVALID, "bh_get_block_signature_counts: blocks out of range");
  if (!counts || count == 0) return nb;
  (void)hipStreamSynchronize(h->stream);
  const int32_t r0 = h->blocks[(size_t)first].rr, r1 = h->blocks[(size_t)(first + count - 1)].rr + 1;
  std::vector<int32_t> c((size_t)(r1 - r0));
  if (hipMemcpy(c.data(), h->sp.cnt + r0, c.size() * 4, hipMemcpyDeviceToHost) != hipSuccess)
    return -h->fail(BH_ERR_DEVICE, "bh_get_block_signature_counts: device copy failed");
  for (int64_t i = 0; i < count; ++i) counts[i] = c[(size_t)(h->blocks[(size_t)(first + i)].rr - r0)];
  return nb;
}

int32_t bh_get_block_signatures(bh_handle *h, int64_t block, int32_t *validators, uint8_t *r, uint8_t *s,
                                int32_t cap) {
  if (!h) return -BH_ERR_INVALID;
  if (int rc = pool_ready(h, "bh_get_block_signatures")) return -rc;
  const int32_t row = block_row(h, block), n = h->d.n;
  if (row < 0) return -h->fail(BH_ERR_KEY_NOT_FOUND, "GetBlock(%lld): no such block", (long long)block);
  std::vector<uint8_t> set((size_t)n), rs((size_t)n * 64);
  if (hipStreamSynchronize(h->stream) != hipSuccess ||
      hipMemcpy(set.data(), h->sp.set + (int64_t)row * n, set.size(), hipMemcpyDeviceToHost) != hipSuccess ||
      hipMemcpy(rs.data(), h->sp.rs + (int64_t)row * n * 64, rs.size(), hipMemcpyDeviceToHost) != hipSuccess)
    return -h->fail(BH_ERR_DEVICE, "bh_get_block_signatures: device copy failed");
  int32_t k = 0;
  for (int32_t v = 0; v < n; ++v) {
    if (!set[(size_t)v]) continue;
    if (k < cap) {
      if (validators) validators[k] = v;
      if (r) memcpy(r + 32 * k, rs.data() + 64 * v, 32);
      if (s) memcpy(s + 32 * k, rs.data() + 64 * v + 32, 32);
    }
    ++k;
  }
  return k;
}

int bh_get_anchor_block(bh_handle *h, int64_t *index) {
  if (!h || !index) return BH_ERR_INVALID;
  if (sharded(h)) return h->fail(BH_ERR_STATE, "bh_get_anchor_block: one shard (block signatures are not sharded)");
  *index = h->sig_anchor;
  return BH_OK;
}

int64_t bh_get_sig_pool(bh_handle *h, int32_t *validator, int64_t *block_index, uint8_t *sig_r, uint8_t *sig_s,
                        int64_t cap) {
  if (!h) return -BH_ERR_INVALID;
  if (int rc = pool_ready(h, "bh_get_sig_pool")) return -rc;
  const int64_t m = std::min(h->pool_count, std::max<int64_t>(cap, 0));
  if (m > 0) {
    std::vector<uint8_t> rs((size_t)m * 64);
    bool ok = hipStreamSynchronize(h->stream) == hipSuccess;
    if (ok && validator) ok = hipMemcpy(validator, h->sp.val, (size_t)m * 4, hipMemcpyDeviceToHost) == hipSuccess;
    if (ok && block_index) ok = hipMemcpy(block_index, h->sp.blk, (size_t)m * 8, hipMemcpyDeviceToHost) == hipSuccess;
    if (ok) ok = hipMemcpy(rs.data(), h->sp.prs, rs.size(), hipMemcpyDeviceToHost) == hipSuccess;
    if (!ok) return -h->fail(BH_ERR_DEVICE, "bh_get_sig_pool: device copy failed");
    for (int64_t i = 0; i < m; ++i) {
      if (sig_r) memcpy(sig_r + 32 * i, rs.data() + 64 * i, 32);
      if (sig_s) memcpy(sig_s + 32 * i, rs.data() + 64 * i + 32, 32);
    }
  }
  return h->pool_count;
}

int bh_get_sig_stats(bh_handle *h, bh_sig_stats *o) {
  if (!h || !o) return BH_ERR_INVALID;
  o->pool = h->pool_count;
  o->verified = h->sig_verified;
  o->accepted = h->sig_accepted;
  o->verified_total = h->sig_verified_total;
  o->table_bytes = h->sig_window ? (int64_t)bh::fixed_table_bytes(h->d.n, h->sig_window) : 0;
  o->window_bits = h->sig_window;
  o->trust_count = (h->d.n + 2) / 3;
  o->verify_signatures_ms = h->verify_ms;
  o->verify_fixed_ms = h->verify_fixed_ms;
  o->set_validators_ms = h->tables_ms;
  o->process_sig_pool_ms = h->pool_ms;
  return BH_OK;
}

}  // extern "C"
