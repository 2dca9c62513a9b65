// Workgroup id -> (column block, row block, K slice) of the FMT's weight-streaming GEMM (fmt_gemm_body) without a run-time
// division: the divisors (row blocks, column blocks, (column block, K slice) pairs) are the same for every workgroup of a launch,
// so the host turns each into a multiply-high constant once per launch and the kernel's head is shifts and three scalar
// multiplies in front of its first operand load.  Plain C++ (no HIP header): tests/fmt_block_decode_main.cpp builds it with the
// host compiler and holds it against the formula with / and % for every shape the launchers produce.
#pragma once

#if defined(__HIPCC__)
#define FMT_HD __host__ __device__ __forceinline__
#else
#define FMT_HD inline
#endif

// n / d == (n * mul) >> sh for 0 <= n < 2^28 (Granlund & Montgomery, as ImgpDiv in imgp_kernels.hpp): with l = ceil(log2 d),
// sh = 28 + l and mul = floor(2^sh / d) + 1, 2^sh <= mul * d <= 2^sh + 2^l; mul <= 2^29 + 1.
struct FmtDiv {
  unsigned mul, sh;
};
inline FmtDiv fmt_make_div(unsigned d) {
  unsigned l = 0;
  while ((1u << l) < d) ++l;
  FmtDiv v;
  v.sh = 28u + l;
  v.mul = (unsigned)((1ull << v.sh) / d + 1ull);
  return v;
}
FMT_HD unsigned fmt_div(unsigned n, unsigned mul, unsigned sh) { return (unsigned)(((unsigned long long)n * mul) >> sh); }
FMT_HD unsigned fmt_div(unsigned n, const FmtDiv& d) { return fmt_div(n, d.mul, d.sh); }
constexpr unsigned kFmtDivMax = 1u << 28;  // dividends must stay below this

// 6 dwords, made by fmt_make_decode.  bits: [0,6) shift of / mblk, [6,12) of / nbx, [12,18) of / nbn, [18,20) log2 P,
// bit 20: XCD-affine walk (nbx a multiple of 8), bit 21: K slices <-> XCDs (affine and ksplit a divisor of 8, P = 8 / ksplit)
struct GemmDecode {
  unsigned mblk_mul;      // slot / mblk
  unsigned nbx, nbx_mul;  // (column block, K slice) pairs = nbn * ksplit (nbn when the launch does not split K); id / nbx
  unsigned nbn, nbn_mul;  // column blocks N / BN; pair / nbn
  unsigned bits;
};
enum { kDecAffine = 1u << 20, kDecKsXcd = 1u << 21 };

// nbn column blocks x mblk row blocks (x ksplit K slices when `partial`, the EPI_PARTIAL launches)
inline GemmDecode fmt_make_decode(int nbn, int mblk, int ksplit, bool partial) {
  GemmDecode d;
  const unsigned nbx = (unsigned)(partial ? nbn * ksplit : nbn);
  const FmtDiv dm = fmt_make_div((unsigned)mblk), dx = fmt_make_div(nbx), dn = fmt_make_div((unsigned)nbn);
  d.mblk_mul = dm.mul, d.nbx = nbx, d.nbx_mul = dx.mul, d.nbn = (unsigned)nbn, d.nbn_mul = dn.mul;
  d.bits = dm.sh | (dx.sh << 6) | (dn.sh << 12);
  if ((nbx & 7u) == 0u) {
    d.bits |= kDecAffine;
    if (partial && (8 % ksplit) == 0) {
      unsigned p = 0;
      while ((8u >> p) != (unsigned)ksplit) ++p;  // P = 8 / ksplit = 1 << p
      d.bits |= kDecKsXcd | (p << 18);
    }
  }
  return d;
}

struct GemmBlock {
  int bx, by, ks;
};
// Row blocks of one column block read the same weights: they get consecutive slots on ONE XCD (ids congruent mod 8 share an
// XCD's L2).  K slice <-> XCD affinity: the 8 / ksplit XCDs that own slice ks fetch only that slice of the activations (r01 PMC:
// with slices spread over all XCDs fc2 fetched its 1.5 MB operand 8 times, 12.6 MB against 8.4 MB of weights).
FMT_HD GemmBlock fmt_block_decode(const GemmDecode& d, unsigned mblk, unsigned id, bool partial) {
  unsigned bx, by, ks = 0u;
  if (d.bits & kDecAffine) {
    const unsigned slot = id >> 3, q = fmt_div(slot, d.mblk_mul, d.bits & 63u);
    by = slot - q * mblk;
    bx = q * 8u + (id & 7u);
  } else {
    by = fmt_div(id, d.nbx_mul, (d.bits >> 6) & 63u);
    bx = id - by * d.nbx;
  }
  if (partial) {
    if (d.bits & kDecKsXcd) {
      const unsigned p = (d.bits >> 18) & 3u, x = bx & 7u;
      ks = x >> p;
      bx = ((bx >> 3) << p) + (x & ((1u << p) - 1u));
    } else {
      ks = fmt_div(bx, d.nbn_mul, (d.bits >> 12) & 63u);
      bx -= ks * d.nbn;
    }
  }
  return GemmBlock{(int)bx, (int)by, (int)ks};
}
