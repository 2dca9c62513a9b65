// Segment comparison kernels of float_cmp_segments (include/float_hip.h): per segment the sums of (a - b)^2 and b^2, the
// maximum |a - b|, the number of pairs beyond a threshold and the number of non-finite pairs.  Bandwidth-bound (8 bytes read
// per pair, ~12 fp64 operations), so everything is fp64 from the first add and the result does not depend on how the work was
// cut: cmp_partial_kernel writes one row of 5 doubles per (segment, slice), cmp_fold_kernel adds the slices of a segment in
// a fixed order.  No atomics: bitwise repeatable.
#pragma once
#include "common.hpp"

constexpr int kCmpThreads = 256;
constexpr int kCmpStats = 5;
constexpr int kCmpUnroll = 4;  // 16-byte loads of a and of b in flight per thread

struct CmpAcc {
  double d2 = 0.0, b2 = 0.0, mx = 0.0;
  unsigned long long beyond = 0ull, bad = 0ull;
};

__device__ __forceinline__ void cmp_pair(float a, float b, double thr, CmpAcc& c) {
  const bool fin = (__float_as_uint(a) & 0x7f800000u) != 0x7f800000u && (__float_as_uint(b) & 0x7f800000u) != 0x7f800000u;
  const double bd = fin ? (double)b : 0.0;
  const double d = fin ? (double)a - (double)b : 0.0;
  const double ad = fabs(d);
  c.d2 += d * d;
  c.b2 += bd * bd;
  c.mx = fmax(c.mx, ad);
  c.beyond += ad > thr ? 1ull : 0ull;
  c.bad += fin ? 0ull : 1ull;
}

// b shares a's offset from a 16-byte boundary (ALIGNED) or not: then its 16 bytes are read as an under-aligned vector
template <bool ALIGNED>
__device__ __forceinline__ fh_f4v cmp_load_b(const float* p) {
  if constexpr (ALIGNED) {
    return __builtin_nontemporal_load(reinterpret_cast<const fh_f4v*>(p));
  } else {
    fh_f4v v;
    __builtin_memcpy(&v, p, sizeof(v));
    return v;
  }
}

// 16-byte groups [v0, v1) of a segment's aligned body: pa is 16-byte aligned
template <bool B_ALIGNED>
__device__ __forceinline__ void cmp_body(const float* __restrict__ pa, const float* __restrict__ pb, long long v0, long long v1,
                                         double thr, CmpAcc& c) {
  long long i = v0 + threadIdx.x;
  for (; i + (kCmpUnroll - 1) * kCmpThreads < v1; i += kCmpUnroll * kCmpThreads) {
    fh_f4v va[kCmpUnroll], vb[kCmpUnroll];
#pragma unroll
    for (int u = 0; u < kCmpUnroll; ++u) {
      va[u] = __builtin_nontemporal_load(reinterpret_cast<const fh_f4v*>(pa) + i + u * kCmpThreads);
      vb[u] = cmp_load_b<B_ALIGNED>(pb + 4 * (i + u * kCmpThreads));
    }
#pragma unroll
    for (int u = 0; u < kCmpUnroll; ++u)
#pragma unroll
      for (int j = 0; j < 4; ++j) cmp_pair(va[u][j], vb[u][j], thr, c);
  }
  for (; i < v1; i += kCmpThreads) {
    const fh_f4v va = __builtin_nontemporal_load(reinterpret_cast<const fh_f4v*>(pa) + i);
    const fh_f4v vb = cmp_load_b<B_ALIGNED>(pb + 4 * i);
#pragma unroll
    for (int j = 0; j < 4; ++j) cmp_pair(va[j], vb[j], thr, c);
  }
}

__device__ __forceinline__ double cmp_wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ double cmp_wave_max(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
  return v;
}

// grid = n_seg * slices workgroups of 256 threads; workgroup (seg, sl) covers 16-byte groups [nv * sl / slices,
// nv * (sl + 1) / slices) of the segment's aligned body; slice 0 also takes the head, the last slice the tail (< 4 elements
// each).  work[(seg * slices + sl) * 5 + k] = the slice's partial of statistic k.
__global__ __launch_bounds__(kCmpThreads) void cmp_partial_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                                  long long seg_len, int slices, float thr_f,
                                                                  double* __restrict__ work) {
  const int seg = blockIdx.x / slices, sl = blockIdx.x - seg * slices;
  const int tid = threadIdx.x;
  const float* pa = a + (long long)seg * seg_len;
  const float* pb = b + (long long)seg * seg_len;
  const double thr = (double)thr_f;
  long long head = (long long)(((16u - (unsigned)((uintptr_t)pa & 15u)) & 15u) >> 2);
  if (head > seg_len) head = seg_len;
  const long long nv = (seg_len - head) >> 2;
  const long long tail0 = head + 4 * nv;
  const long long v0 = nv * sl / slices, v1 = nv * (sl + 1) / slices;
  CmpAcc c;
  if (((uintptr_t)(pb + head) & 15u) == 0) cmp_body<true>(pa + head, pb + head, v0, v1, thr, c);
  else cmp_body<false>(pa + head, pb + head, v0, v1, thr, c);
  if (sl == 0 && tid < head) cmp_pair(pa[tid], pb[tid], thr, c);
  if (sl == slices - 1 && tail0 + tid < seg_len) cmp_pair(pa[tail0 + tid], pb[tail0 + tid], thr, c);
  // wave64 shuffles, then the four waves through LDS in wave order (counts are exact in a double up to 2^53)
  double v[kCmpStats] = {cmp_wave_sum(c.d2), cmp_wave_sum(c.b2), cmp_wave_max(c.mx), cmp_wave_sum((double)c.beyond),
                         cmp_wave_sum((double)c.bad)};
  __shared__ double red[kCmpThreads / 64][kCmpStats];
  if ((tid & 63) == 0) {
#pragma unroll
    for (int k = 0; k < kCmpStats; ++k) red[tid >> 6][k] = v[k];
  }
  __syncthreads();
  if (tid < kCmpStats) {
    double r = red[0][tid];
#pragma unroll
    for (int w = 1; w < kCmpThreads / 64; ++w) r = tid == 2 ? fmax(r, red[w][tid]) : r + red[w][tid];
    work[(size_t)blockIdx.x * kCmpStats + tid] = r;
  }
}

// one wave per segment: lane l adds slices l, l + 64, ... in that order, then the lanes by shuffles
__global__ __launch_bounds__(64) void cmp_fold_kernel(const double* __restrict__ work, int slices, double* __restrict__ stats) {
  const int seg = blockIdx.x, lane = threadIdx.x;
  double v[kCmpStats] = {0.0, 0.0, 0.0, 0.0, 0.0};
  for (int s = lane; s < slices; s += 64) {
    const double* w = work + ((size_t)seg * slices + s) * kCmpStats;
#pragma unroll
    for (int k = 0; k < kCmpStats; ++k) v[k] = k == 2 ? fmax(v[k], w[k]) : v[k] + w[k];
  }
#pragma unroll
  for (int k = 0; k < kCmpStats; ++k) v[k] = k == 2 ? cmp_wave_max(v[k]) : cmp_wave_sum(v[k]);
  if (lane < kCmpStats) {
    double r = v[0];
#pragma unroll
    for (int k = 1; k < kCmpStats; ++k) r = lane == k ? v[k] : r;
    stats[(size_t)seg * kCmpStats + lane] = r;
  }
}
