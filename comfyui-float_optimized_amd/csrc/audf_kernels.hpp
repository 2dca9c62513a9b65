// Kernels of float_aud_front (include/float_hip.h): channel mean, band-limited resampling and zero-mean / unit-variance of a
// waveform in HBM.  The windowed sinc is evaluated where it is used, so there is no polyphase table and any pair of rates is
// served exactly.
//   audf_resample_kernel  a workgroup owns kAudfTile consecutive outputs, stages the mono mix of the input span they read
//                         into LDS (coalesced, channels summed while loading, zero outside the clip) and every lane walks the
//                         2 W + 2 taps of its output from there
//   audf_mix_kernel       rate_in == rate_out: the mono mix itself
//   both also write the tile's sum of y and of y^2 as fp64 partials when normalising; audf_fold_kernel adds the partials in a
//   fixed order (no atomics: bitwise repeatable, like cmp_fold_kernel) and audf_norm_kernel rewrites a in place.
// Lanes read the LDS at a stride of about rate_in / rate_out samples: conflict-free for odd strides (48 kHz -> 16 kHz: 3),
// 2-way for 32 kHz, mixed for 44.1 kHz (2 or 3 between neighbours).  Left as it is: the per-tap cost is the 114 instructions
// of the filter (hipcc's inlined sinpif / cospif most of them), not the one ds_read_b32 beside them.
#pragma once
#include "common.hpp"

constexpr int kAudfTile = 256;          // outputs per workgroup = threads per workgroup (tests/test_aud_front_gpu.py: TILE)
constexpr size_t kAudfMaxLds = 160000;  // bytes of staged input a workgroup may ask for (a CU has 160 KiB)
constexpr int kAudfHead = 2;            // work[0] = mean, work[1] = 1 / sqrt(var + 1e-7); then 2 doubles per tile

struct AudfPlan {
  long long n_in, n_out, ch_stride;
  int channels, up, down;  // rate_out / g, rate_in / g
  int W;                   // ceil(zeros / c): taps j = q - W ... q + W + 1 cover every |j - pos| <= zeros / c
  int zeros, stats;
  double c, inv_up, inv_zeros;
};

__device__ __forceinline__ double audf_wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// the tile's (sum y, sum y^2): wave shuffles, then the four waves through LDS in wave order
__device__ __forceinline__ void audf_tile_stats(float y, bool valid, double* __restrict__ work) {
  const int tid = threadIdx.x;
  const double yd = valid ? (double)y : 0.0;
  const double s1 = audf_wave_sum(yd), s2 = audf_wave_sum(yd * yd);
  __shared__ double red[kAudfTile / 64][2];
  if ((tid & 63) == 0) {
    red[tid >> 6][0] = s1;
    red[tid >> 6][1] = s2;
  }
  __syncthreads();
  if (tid < 2) {
    double r = red[0][tid];
#pragma unroll
    for (int w = 1; w < kAudfTile / 64; ++w) r += red[w][tid];
    work[kAudfHead + 2 * (size_t)blockIdx.x + tid] = r;
  }
}

__device__ __forceinline__ float audf_mono(const float* __restrict__ w, long long ch_stride, int channels, long long j) {
  float s = w[j];
  for (int c = 1; c < channels; ++c) s += w[(long long)c * ch_stride + j];
  return s / (float)channels;
}

// x * sinc(t) * cos^2(pi t / (2 zeros)) of tap distance d = j - pos (exact to fp64 rounding).  t and its range reduction are
// fp64 (t up to 32: an fp32 t would carry 2^-24 * 32 into the sine's argument); the reduced argument, both trigonometric
// functions and the weight are fp32; the sum over the taps is fp64 again (one v_fma_f64 beside 114 instructions of weight), so
// that what is left is the rounding of the weights, whatever the number of taps (156 at 48 kHz, 3254 at 64 : 1).  At the clamp
// t = +-zeros the reduced argument is 0: the weight is exactly 0.
__device__ __forceinline__ double audf_tap(float x, double d, const AudfPlan& p) {
  const double zr = (double)p.zeros;
  const double t = fmin(fmax(d * p.c, -zr), zr);
  const double n = rint(t);
  const float f = (float)(t - n);                                      // [-0.5, 0.5], exact difference
  const float sgn = ((int)n & 1) ? -1.f : 1.f;
  const float pt = (float)(t * 3.14159265358979323846);
  const float sinc = pt == 0.f ? 1.f : sgn * sinpif(f) / pt;
  const float win = 0.5f + 0.5f * cospif((float)(t * p.inv_zeros));  // cos^2(a) = (1 + cos 2a) / 2
  return (double)x * (double)(sinc * win);                            // an exact product
}

// grid = ceil(n_out / kAudfTile) workgroups of kAudfTile threads; dynamic LDS: the tile's staged samples (audf_api.hip)
__global__ __launch_bounds__(kAudfTile) void audf_resample_kernel(const float* __restrict__ w, float* __restrict__ a,
                                                                  double* __restrict__ work, const AudfPlan p) {
  extern __shared__ __attribute__((aligned(16))) float audf_xs[];
  const int tid = threadIdx.x;
  // position of the tile's first output in 64-bit integers (m * down passes 2^31 after 304 s of 44.1 kHz); the lanes'
  // offsets from it fit 32 bits: r0 + 255 * down < 2^20 + 255 * 2^20
  const long long m0 = (long long)blockIdx.x * kAudfTile;
  const long long num0 = m0 * (long long)p.down;
  const long long q0 = num0 / p.up;
  const unsigned r0 = (unsigned)(num0 - q0 * p.up);
  const unsigned last = r0 + (unsigned)(kAudfTile - 1) * (unsigned)p.down;
  const int n_stage = (int)(last / (unsigned)p.up) + 2 * p.W + 2;  // <= the launch's LDS (audf_api.hip)
  const long long first = q0 - p.W;
  for (int i = tid; i < n_stage; i += kAudfTile) {
    const long long j = first + i;
    audf_xs[i] = (j >= 0 && j < p.n_in) ? audf_mono(w, p.ch_stride, p.channels, j) : 0.f;
  }
  __syncthreads();
  const unsigned num = r0 + (unsigned)tid * (unsigned)p.down;
  const unsigned dq = num / (unsigned)p.up;
  const double frac = (double)(num - dq * (unsigned)p.up) * p.inv_up;  // pos - q in [0, 1)
  const float* xs = audf_xs + dq;                                      // x[q - W]; the last tap read is xs[2 W + 1]
  double acc0 = 0.0, acc1 = 0.0;
  const int taps = 2 * p.W + 2;
  for (int k = 0; k < taps; k += 2) {
    acc0 += audf_tap(xs[k], (double)(k - p.W) - frac, p);
    acc1 += audf_tap(xs[k + 1], (double)(k + 1 - p.W) - frac, p);
  }
  const float y = (float)((acc0 + acc1) * p.c);
  const bool valid = m0 + tid < p.n_out;
  if (valid) a[m0 + tid] = y;
  if (p.stats) audf_tile_stats(y, valid, work);
}

__global__ __launch_bounds__(kAudfTile) void audf_mix_kernel(const float* __restrict__ w, float* __restrict__ a,
                                                             double* __restrict__ work, const AudfPlan p) {
  const long long m = (long long)blockIdx.x * kAudfTile + threadIdx.x;
  const bool valid = m < p.n_out;
  float y = 0.f;
  if (valid) a[m] = y = audf_mono(w, p.ch_stride, p.channels, m);
  if (p.stats) audf_tile_stats(y, valid, work);
}

// one workgroup: thread t adds tiles t, t + 256, ... in that order, then the threads in a fixed tree
__global__ __launch_bounds__(kAudfTile) void audf_fold_kernel(double* __restrict__ work, long long n_tiles, long long n_out) {
  const int tid = threadIdx.x;
  double s1 = 0.0, s2 = 0.0;
  for (long long t = tid; t < n_tiles; t += kAudfTile) {
    s1 += work[kAudfHead + 2 * t];
    s2 += work[kAudfHead + 2 * t + 1];
  }
  s1 = audf_wave_sum(s1);
  s2 = audf_wave_sum(s2);
  __shared__ double red[kAudfTile / 64][2];
  if ((tid & 63) == 0) {
    red[tid >> 6][0] = s1;
    red[tid >> 6][1] = s2;
  }
  __syncthreads();
  if (tid == 0) {
    double t1 = red[0][0], t2 = red[0][1];
#pragma unroll
    for (int w = 1; w < kAudfTile / 64; ++w) {
      t1 += red[w][0];
      t2 += red[w][1];
    }
    const double mean = t1 / (double)n_out;
    const double var = fmax(t2 / (double)n_out - mean * mean, 0.0);  // biased; a constant y: 0, not a negative rounding
    work[0] = mean;
    work[1] = 1.0 / sqrt(var + 1e-7);
  }
}

__global__ __launch_bounds__(kAudfTile) void audf_norm_kernel(float* __restrict__ a, const double* __restrict__ work, long long n_out) {
  const long long m = (long long)blockIdx.x * kAudfTile + threadIdx.x;
  if (m < n_out) a[m] = (float)(((double)a[m] - work[0]) * work[1]);
}
