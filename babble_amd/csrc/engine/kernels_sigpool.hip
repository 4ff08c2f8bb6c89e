// kernels_sigpool.hip -- ECDSA P-256 verification against a fixed signer set.
//
// Reference: block signatures.  Every validator signs every block
// (node.go:605-630); ProcessSigPool (hashgraph.go:1236-1300) and CheckBlock
// (hashgraph.go:1483-1497) verify them with Block.Verify (block.go:234-254)
// -> crypto.Verify -> Go's ecdsa.Verify(pub, hash, r, s).  The signers are
// the handle's n participants, so their keys are tabulated once
// (bh_set_validators) and u1 G + u2 Q becomes table additions only.
//
// Table layout (uint32 words, Montgomery form, affine):
//   tab[slot][j][d - 1][16]   slot in [0, n]: validator slot, n = the generator G
//                             j in [0, 256 / W): window
//                             d in [1, 2^W): the point d 2^(W j) P_slot, x[8] || y[8]
// so 64 (2^W - 1) (256 / W) bytes per slot: 522,240 B at W = 8, 61,440 B at
// W = 4.  A scalar k = sum_j d_j 2^(W j) gives k P = sum_j tab[.][j][d_j - 1]:
// 256 / W mixed additions and no doubling; a zero window adds nothing.
// Indices are 64-bit: 513 slots at W = 8 are 268 MB.
#include "engine.h"
#include "p256.h"

namespace bh {

__device__ __forceinline__ void to_affine(const J &p, F *x, F *y) {
  const F zi = mpow(p.z, EC_PM2, EC_P, EC_MINV_P, fconst(EC_ONEP));
  const F zi2 = psqr(zi);
  *x = pmul(p.x, zi2);
  *y = pmul(p.y, pmul(zi2, zi));
}

__device__ __forceinline__ void store_entry(uint32_t *e, const F &x, const F &y) {
  uint4 *q = reinterpret_cast<uint4 *>(e);
  q[0] = make_uint4(x.v[0], x.v[1], x.v[2], x.v[3]);
  q[1] = make_uint4(x.v[4], x.v[5], x.v[6], x.v[7]);
  q[2] = make_uint4(y.v[0], y.v[1], y.v[2], y.v[3]);
  q[3] = make_uint4(y.v[4], y.v[5], y.v[6], y.v[7]);
}

__device__ __forceinline__ void load_entry(const uint32_t *e, F *x, F *y) {
  const uint4 *q = reinterpret_cast<const uint4 *>(e);
  const uint4 a = q[0], b = q[1], c = q[2], d = q[3];
  x->v[0] = a.x, x->v[1] = a.y, x->v[2] = a.z, x->v[3] = a.w;
  x->v[4] = b.x, x->v[5] = b.y, x->v[6] = b.z, x->v[7] = b.w;
  y->v[0] = c.x, y->v[1] = c.y, y->v[2] = c.z, y->v[3] = c.w;
  y->v[4] = d.x, y->v[5] = d.y, y->v[6] = d.z, y->v[7] = d.w;
}

// One thread per (slot, window): B = 2^(W j) P by doublings, then the
// multiples 2 B .. (2^W - 1) B by repeated mixed addition of B (the first is
// pmadd's doubling case), each made affine by one field inversion.  P has
// prime order q and d 2^(W j) < 2^256 < 2 q is no multiple of q for d < 2^W,
// so no entry is the point at infinity.
template <int W>
__global__ __launch_bounds__(64) void k_fixed_tables(const uint8_t *pub, int32_t n, uint32_t *tab) {
  constexpr int NW = 256 / W, NE = (1 << W) - 1;
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (int64_t)(n + 1) * NW) return;
  const int32_t slot = (int32_t)(t / NW), j = (int32_t)(t % NW);
  F x, y;
  if (slot < n) {
    const uint8_t *pk = pub + 64 * (int64_t)slot;
    x = pmul(load_be(pk), fconst(EC_R2P));
    y = pmul(load_be(pk + 32), fconst(EC_R2P));
  } else {
    x = fconst(EC_GX);
    y = fconst(EC_GY);
  }
  J acc{x, y, fconst(EC_ONEP)};
  if (j > 0) {
    for (int k = 0; k < W * j; ++k) acc = pdbl(acc);
    to_affine(acc, &x, &y);
    acc = J{x, y, fconst(EC_ONEP)};
  }
  uint32_t *out = tab + ((int64_t)slot * NW + j) * NE * 16;
  store_entry(out, x, y);
  for (int d = 2; d <= NE; ++d) {
    acc = pmadd(acc, x, y);
    F ax, ay;
    to_affine(acc, &ax, &ay);
    store_entry(out + (int64_t)(d - 1) * 16, ax, ay);
  }
}

// ecdsa.Verify of signature i by validator val[i] (a slot in [0, n), checked
// by the caller) through the tables.  The accumulator starts at infinity and
// meets table points, so pmadd's infinity, P + P and P + (-P) cases are all
// reachable.  Instead of the affine x (a field inversion) the final test is
// X == r Z^2 (mod p), and X == (r + n) Z^2 when r + n < p: the x >= n case
// of x mod n == r (p < 2 n, so there is no third candidate).
template <int W>
__device__ __forceinline__ bool verify_fixed_one(const F &e, const F &r, const F &s, int32_t v, int32_t n,
                                                 const uint32_t *tab) {
  constexpr int NW = 256 / W, NE = (1 << W) - 1;
  if (fzero(r) || fzero(s) || !fless(r, EC_N) || !fless(s, EC_N)) return false;
  const F one_n = mmul(fconst(EC_R2N), fsmall(1), EC_N, EC_MINV_N);  // R mod n
  const F sm = mmul(s, fconst(EC_R2N), EC_N, EC_MINV_N);             // s R
  const F wm = mpow(sm, EC_NM2, EC_N, EC_MINV_N, one_n);             // s^-1 R
  const F u1 = mmul(e, wm, EC_N, EC_MINV_N), u2 = mmul(r, wm, EC_N, EC_MINV_N);  // plain form
  const uint32_t *tg = tab + (int64_t)n * NW * NE * 16, *tq = tab + (int64_t)v * NW * NE * 16;
  J acc{fconst(EC_ONEP), fconst(EC_ONEP), fsmall(0)};
  for (int j = 0; j < NW; ++j) {
    const int b = W * j;  // W divides 32: a window never straddles two limbs
    const uint32_t d1 = (u1.v[b >> 5] >> (b & 31)) & NE, d2 = (u2.v[b >> 5] >> (b & 31)) & NE;
    F x, y;
    if (d1) {
      load_entry(tg + ((int64_t)j * NE + (d1 - 1)) * 16, &x, &y);
      acc = pmadd(acc, x, y);
    }
    if (d2) {
      load_entry(tq + ((int64_t)j * NE + (d2 - 1)) * 16, &x, &y);
      acc = pmadd(acc, x, y);
    }
  }
  if (fzero(acc.z)) return false;
  const F z2 = psqr(acc.z);
  if (feq(acc.x, pmul(pmul(r, fconst(EC_R2P)), z2))) return true;
  F rn;
  uint64_t c = 0;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const uint64_t t = (uint64_t)r.v[k] + EC_N[k] + c;
    rn.v[k] = (uint32_t)t;
    c = t >> 32;
  }
  if (c || !fless(rn, EC_P)) return false;
  return feq(acc.x, pmul(pmul(rn, fconst(EC_R2P)), z2));
}

template <int W>
__global__ __launch_bounds__(128) void k_verify_fixed(const uint8_t *hash, const uint8_t *sr, const uint8_t *ss,
                                                      const int32_t *val, int32_t n, const uint32_t *tab,
                                                      int64_t count, uint8_t *ok) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  const F e = load_be(hash + 32 * i), r = load_be(sr + 32 * i), s = load_be(ss + 32 * i);
  ok[i] = verify_fixed_one<W>(e, r, s, val[i], n, tab) ? 1 : 0;
}

// ---------------------------------------------------------------------------
// ProcessSigPool (hashgraph.go:1236-1300) as four launches.  The reference's
// loop is order-independent except for which duplicate wins (the later one)
// and the anchor is max(old, blocks that accepted a signature in this pass and
// now hold more than trustCount), so: verdicts and an atomic max of the pool
// position per (block, validator); the winners commit; counts are final;
// atomic max of the anchor; a stable compaction of the survivors.
template <int W>
__global__ __launch_bounds__(128) void k_pool_verify(Frames fr, SigPool sp, int64_t count) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  sp.stat[i] = 0;
  sp.row[i] = -1;
  const int32_t v = sp.val[i];
  if (v < 0) return;  // unknown validator: stays pooled
  const int64_t b = sp.blk[i], k = b - sp.first_block;
  int32_t row = -1, ver = 0;
  const uint8_t *hash = nullptr;
  if (k >= 0 && k < sp.nblocks) {
    const int32_t f = sp.blk_rr[k];
    if (fr.fvalid[f]) {
      row = f;
      ver = fr.bver[f];
      hash = fr.shash + (int64_t)f * 32;
    }
  } else if (b == sp.reset_block && sp.reset_ver >= 0) {
    row = sp.R1;
    ver = sp.reset_ver;
    hash = sp.reset_shash;
  }
  if (row < 0) return;              // block not held: stays pooled
  if (sp.seen[i] == ver) return;    // judged invalid against this very body: not verified again
  atomicAdd((unsigned long long *)&sp.misc[2], 1ull);
  const uint8_t *rs = sp.prs + 64 * i;
  const bool ok = verify_fixed_one<W>(load_be(hash), load_be(rs), load_be(rs + 32), v, sp.n, sp.tab);
  if (ok) {
    sp.stat[i] = 1;
    sp.row[i] = row;
    atomicMax(&sp.winner[(int64_t)row * sp.n + v], (int32_t)i);
  } else {
    sp.seen[i] = ver;
  }
}

__global__ __launch_bounds__(256) void k_pool_commit(SigPool sp, int64_t count) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count || !sp.stat[i]) return;
  const int64_t slot = (int64_t)sp.row[i] * sp.n + sp.val[i];
  if (sp.winner[slot] != (int32_t)i) return;  // a later valid entry for the pair replaces this one
  for (int k = 0; k < 64; ++k) sp.rs[slot * 64 + k] = sp.prs[64 * i + k];
  if (!sp.set[slot]) {
    sp.set[slot] = 1;
    atomicAdd(&sp.cnt[sp.row[i]], 1);
  }
}

__global__ __launch_bounds__(256) void k_pool_anchor(SigPool sp, int64_t count) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count || !sp.stat[i]) return;
  atomicAdd((unsigned long long *)&sp.misc[1], 1ull);
  sp.winner[(int64_t)sp.row[i] * sp.n + sp.val[i]] = -1;  // (scratch for the next pass)
  if (sp.cnt[sp.row[i]] > sp.trust) atomicMax((unsigned long long *)&sp.misc[0], (unsigned long long)(sp.blk[i] + 1));
}

// stable compaction of the entries with stat == 0 into the second buffers:
// one workgroup walks the pool in chunks of 1024 with a running base (a call
// that accepted nothing skips it, so a live node's call with nothing new
// costs the verdict kernel's early exits only)
__global__ __launch_bounds__(1024) void k_pool_compact(SigPool sp, int64_t count) {
  __shared__ int32_t sc[1024];
  __shared__ int64_t base;
  const int t = threadIdx.x;
  if (sp.misc[1] == 0) {  // nothing left the pool: it stays where it is (the host does not swap)
    if (t == 0) sp.misc[3] = count;
    return;
  }
  if (t == 0) base = 0;
  __syncthreads();
  for (int64_t c0 = 0; c0 < count; c0 += 1024) {
    const int64_t i = c0 + t;
    const int32_t keep = i < count && !sp.stat[i] ? 1 : 0;
    sc[t] = keep;
    __syncthreads();
    for (int d = 1; d < 1024; d <<= 1) {  // inclusive scan
      const int32_t x = t >= d ? sc[t - d] : 0;
      __syncthreads();
      sc[t] += x;
      __syncthreads();
    }
    if (keep) {
      const int64_t o = base + sc[t] - 1;
      sp.val2[o] = sp.val[i];
      sp.blk2[o] = sp.blk[i];
      sp.seen2[o] = sp.seen[i];
      for (int k = 0; k < 64; ++k) sp.prs2[64 * o + k] = sp.prs[64 * i + k];
    }
    __syncthreads();
    if (t == 0) base += sc[1023];
    __syncthreads();
  }
  if (t == 0) sp.misc[3] = base;
}

void launch_sig_pool_pass(const Frames &fr, const SigPool &sp, int64_t count, hipStream_t st) {
  (void)hipMemsetAsync(sp.misc + 1, 0, 3 * 8, st);
  if (count <= 0) return;
  const unsigned g = (unsigned)((count + 127) / 128), g2 = (unsigned)((count + 255) / 256);
  if (sp.window == 8)
    k_pool_verify<8><<<g, 128, 0, st>>>(fr, sp, count);
  else
    k_pool_verify<4><<<g, 128, 0, st>>>(fr, sp, count);
  k_pool_commit<<<g2, 256, 0, st>>>(sp, count);
  k_pool_anchor<<<g2, 256, 0, st>>>(sp, count);
  k_pool_compact<<<1, 1024, 0, st>>>(sp, count);
}

// Block.SetSignature as Core.SignBlock uses it (core.go:152-161): no
// verification, no anchor move
__global__ void k_sig_set(SigPool sp, int32_t row, int32_t v, const uint8_t *rs) {
  const int64_t slot = (int64_t)row * sp.n + v;
  for (int k = 0; k < 64; ++k) sp.rs[slot * 64 + k] = rs[k];
  if (!sp.set[slot]) {
    sp.set[slot] = 1;
    sp.cnt[row] += 1;
  }
}

void launch_sig_set(const SigPool &sp, int32_t row, int32_t v, const uint8_t *rs, hipStream_t st) {
  k_sig_set<<<1, 1, 0, st>>>(sp, row, v, rs);
}

size_t fixed_table_bytes(int32_t n, int window) {
  return (size_t)(n + 1) * (size_t)(256 / window) * (size_t)((1 << window) - 1) * 64;
}

void launch_fixed_tables(const uint8_t *pub, int32_t n, int window, uint32_t *tab, hipStream_t st) {
  const int64_t threads = (int64_t)(n + 1) * (256 / window);
  const unsigned g = (unsigned)((threads + 63) / 64);
  if (window == 8)
    k_fixed_tables<8><<<g, 64, 0, st>>>(pub, n, tab);
  else
    k_fixed_tables<4><<<g, 64, 0, st>>>(pub, n, tab);
}

void launch_verify_fixed(const uint8_t *hash, const uint8_t *r, const uint8_t *s, const int32_t *val, int32_t n,
                         int window, const uint32_t *tab, int64_t count, uint8_t *ok, hipStream_t st) {
  if (count <= 0) return;
  const unsigned g = (unsigned)((count + 127) / 128);
  if (window == 8)
    k_verify_fixed<8><<<g, 128, 0, st>>>(hash, r, s, val, n, tab, count, ok);
  else
    k_verify_fixed<4><<<g, 128, 0, st>>>(hash, r, s, val, n, tab, count, ok);
}

}  // namespace bh
