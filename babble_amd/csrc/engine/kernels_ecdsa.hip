// kernels_ecdsa.hip -- batched ECDSA P-256 signature verification.
//
// Reference: Event.Verify() (event.go:194-209) decodes the creator's public
// key and the signature (r, s) and calls crypto.Verify -> Go's
// ecdsa.Verify(pub, hash, r, s) (crypto/utils.go:43-51), for every event
// InsertEvent receives (hashgraph.go:716-721).  SURVEY 8(f) row 2.
// ecdsa.Verify: r, s in [1, n-1]; e = the 32-byte hash as an integer (the
// P-256 order has 256 bits, so no truncation); w = s^-1 mod n;
// (x1, y1) = (e w) G + (r w) Q; valid iff the point is finite and
// x1 mod n == r.
//
// One thread per signature.  Field and scalar elements are 8 x 32-bit limbs
// in Montgomery form (CIOS multiplication, R = 2^256); points in Jacobian
// coordinates with a = -3 (dbl-2001-b) and mixed additions of the affine
// G and Q (madd-2007-bl, with its doubling / infinity cases); u1 G + u2 Q by
// Shamir's interleaving (256 doublings); inverses by Fermat exponentiation.
// Integer-only: the result is exact, checked against the generator's
// signatures and a pure-Python verify.
#include "engine.h"
#include "p256.h"

namespace bh {

// hash / r / s: 32 B big-endian per signature; key[i] selects the public
// key pub[key][0..64) = x || y big-endian; ok[i] = 1 if it verifies
__global__ __launch_bounds__(128) void k_ecdsa_verify(const uint8_t *hash, const uint8_t *sr, const uint8_t *ss,
                                                      const int32_t *key, const uint8_t *pub, int64_t count,
                                                      uint8_t *ok) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  const F e = load_be(hash + 32 * i), r = load_be(sr + 32 * i), s = load_be(ss + 32 * i);
  const uint8_t *pk = pub + 64 * (int64_t)key[i];
  const F qx = load_be(pk), qy = load_be(pk + 32);
  bool valid = !fzero(r) && !fzero(s) && fless(r, EC_N) && fless(s, EC_N);
  if (valid) {
    const F one_n = mmul(fconst(EC_R2N), fsmall(1), EC_N, EC_MINV_N);  // R mod n
    const F sm = mmul(s, fconst(EC_R2N), EC_N, EC_MINV_N);             // s R
    const F wm = mpow(sm, EC_NM2, EC_N, EC_MINV_N, one_n);             // s^-1 R
    const F u1 = mmul(e, wm, EC_N, EC_MINV_N), u2 = mmul(r, wm, EC_N, EC_MINV_N);  // plain form
    const F qxm = pmul(qx, fconst(EC_R2P)), qym = pmul(qy, fconst(EC_R2P));
    const F gx = fconst(EC_GX), gy = fconst(EC_GY);
    J acc{fconst(EC_ONEP), fconst(EC_ONEP), fsmall(0)};
    for (int b = 255; b >= 0; --b) {
      acc = pdbl(acc);
      if ((u1.v[b >> 5] >> (b & 31)) & 1u) acc = pmadd(acc, gx, gy);
      if ((u2.v[b >> 5] >> (b & 31)) & 1u) acc = pmadd(acc, qxm, qym);
    }
    if (fzero(acc.z)) {
      valid = false;
    } else {
      const F zi = mpow(acc.z, EC_PM2, EC_P, EC_MINV_P, fconst(EC_ONEP));
      F x = pmul(pmul(acc.x, psqr(zi)), fsmall(1));  // affine x, plain form
      if (!fless(x, EC_N)) {                         // x mod n (x < p < 2n)
        uint64_t br = 0;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const uint64_t t = (uint64_t)x.v[j] - EC_N[j] - br;
          x.v[j] = (uint32_t)t;
          br = (t >> 63) & 1;
        }
      }
      valid = feq(x, r);
    }
  }
  ok[i] = valid ? 1 : 0;
}

void launch_ecdsa_verify(const uint8_t *hash, const uint8_t *r, const uint8_t *s, const int32_t *key,
                         const uint8_t *pub, int64_t count, uint8_t *ok, hipStream_t st) {
  if (count <= 0) return;
  k_ecdsa_verify<<<(unsigned)((count + 127) / 128), 128, 0, st>>>(hash, r, s, key, pub, count, ok);
}

}  // namespace bh
