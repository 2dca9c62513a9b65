// HIP kernels of the S3FD face detector (host_models.sfd_forward / sfd_decode_dense / sfd_nms are the definition): VGG-16
// trunk, six detection heads, box decoding and greedy NMS, run once per clip on the detector's 360-px view.  Activations are
// NHWC in the operand type T like the encoder's (16-bit in production, fp32 in the verification mode), accumulation is fp32.
// The maps are large and shallow (360 x 640 x 64 at the top), the opposite corner from the encoder's shapes; the convs read
// both operands straight from global memory, and whether LDS staging would pay here has not been measured.
// Every kernel takes n stacked views of one size (float_sfd_*_batch): the maps are packed [n][H][W][C], and the pixel index of a
// launch runs over n x pixels, so the small deep maps of several views share 64-pixel tiles.  An output element's arithmetic
// (taps, then 32-channel steps) does not depend on where its pixel sits in a tile or in the stack: view i of a stacked call is
// bit for bit the single-view call.
#pragma once
#include "common.hpp"

constexpr int kSfdLevels = 6;
constexpr int kSfdHeadC = 16;  // conf + loc of a level stacked (8 or 6 channels), zero-padded to one 16-wide MFMA tile

// ------------------------------------------------------------------------------------------
// conv1_1 (3 -> 64, 3 x 3, pad 1) + ReLU, direct: reads the (H, W, 3) uint8 RGB view, flips to BGR, subtracts the mean
// (104, 117, 123); the zero padding is of the mean-subtracted image, as torch pads it.  One thread = one pixel x 8 channels.
// w: [ky][kx][c_bgr][64] fp32, bias [64].
template <class T>
__global__ __launch_bounds__(256) void sfd_first_kernel(const unsigned char* __restrict__ rgb, const float* __restrict__ w,
                                                        const float* __restrict__ bias, typename T::elem* __restrict__ out, int n, int H,
                                                        int W, unsigned long long* sat) {
  __shared__ float sw[27 * 64];
  __shared__ float sb[64];
  for (int i = threadIdx.x; i < 27 * 64; i += 256) sw[i] = w[i];
  if (threadIdx.x < 64) sb[threadIdx.x] = bias[threadIdx.x];
  __syncthreads();
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (size_t)n * H * W * 8) return;
  const int cg = (int)(idx & 7);
  const size_t p = idx >> 3;  // over the n stacked views
  const size_t view = p / ((size_t)H * W), pl = p - view * ((size_t)H * W);
  rgb += view * ((size_t)H * W * 3);
  const int y = (int)(pl / W), x = (int)(pl - (size_t)y * W);
  const float mean[3] = {104.f, 117.f, 123.f};
  float in[27];
#pragma unroll
  for (int ky = 0; ky < 3; ++ky) {
#pragma unroll
    for (int kx = 0; kx < 3; ++kx) {
      const int iy = y + ky - 1, ix = x + kx - 1;
      const bool ok = iy >= 0 && iy < H && ix >= 0 && ix < W;
      const unsigned char* s = rgb + ((size_t)(ok ? iy : 0) * W + (ok ? ix : 0)) * 3;
#pragma unroll
      for (int c = 0; c < 3; ++c) in[(ky * 3 + kx) * 3 + c] = ok ? (float)s[2 - c] - mean[c] : 0.f;
    }
  }
  float acc[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) acc[i] = sb[cg * 8 + i];
#pragma unroll
  for (int t = 0; t < 27; ++t) {
#pragma unroll
    for (int i = 0; i < 8; ++i) acc[i] += in[t] * sw[t * 64 + cg * 8 + i];
  }
  typename T::pack8 o;
#pragma unroll
  for (int i = 0; i < 8; ++i) T::set(o, i, fmaxf(acc[i], 0.f));
  unsigned rm = 0u;
  fh_track_pack<T>(rm, o);
  fh_range_flush<T>(sat, rm);
  T::store8(out + p * 64 + cg * 8, o);
}

// ------------------------------------------------------------------------------------------
// Conv2d as an implicit GEMM on MFMA, the encoder's scheme (enc_conv_kernel) with this network's epilogue: k x k taps
// (3 x 3 or 1 x 1), stride 1 | 2, any zero padding (fc6 pads by 3).  M = output pixels of the n stacked views (64 per workgroup, 16 per wave), N = NT * 16
// output channels, K = taps x Cin in 32-channel steps; a lane's 16 bytes are 8 consecutive channels of one pixel (A) or of one
// (tap, output channel) weight row (B), both straight from global memory.  Operands are swapped (D = W * X^T): a lane ends
// with 4 consecutive channels of one pixel.  Epilogue: + bias, optional ReLU; NHWC store in T (range-tracked) or, for the heads,
// an fp32 NHWC store.  Cin is a multiple of 32, Cout (padded) a multiple of NT * 16.
struct SfdConvArgs {
  const void* X;      // [n][Hi][Wi][Cin] T::elem
  const void* W;      // [k*k][Cout][Cin] T::elem
  void* Y;            // [n][Ho][Wo][Cout] T::elem or nullptr
  float* Yf32;        // [n][Ho][Wo][Cout] fp32 or nullptr
  const float* bias;  // [Cout]
  int n, Hi, Wi, Cin, Cout, Ho, Wo, k, stride, pad, relu;
  unsigned long long* sat;  // range counter of the 16-bit stores (fh_range_flush)
};

template <class T, int NT>
__global__ __launch_bounds__(256) void sfd_conv_kernel(SfdConvArgs g) {
  typedef typename T::elem E;
  typedef typename T::pack8 P8;
  const E* gX = reinterpret_cast<const E*>(g.X);
  const E* const gW = reinterpret_cast<const E*>(g.W);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int r16 = lane & 15, q = lane >> 4;
  const int npix = g.Ho * g.Wo;
  const int m = blockIdx.x * 64 + w * 16 + r16;
  const int n0 = blockIdx.y * NT * 16;
  const bool mvalid = m < g.n * npix;
  const int view = mvalid ? m / npix : 0, ml = mvalid ? m - view * npix : 0;
  gX += (size_t)view * g.Hi * g.Wi * g.Cin;
  const int oy = ml / g.Wo, ox = ml - oy * g.Wo;
  f32x4 acc[NT];
#pragma unroll
  for (int j = 0; j < NT; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int nchunk = g.Cin >> 5;
  for (int ty = 0; ty < g.k; ++ty) {
    const int iy = oy * g.stride - g.pad + ty;
    for (int tx = 0; tx < g.k; ++tx) {
      const int ix = ox * g.stride - g.pad + tx;
      const bool ok = mvalid && iy >= 0 && iy < g.Hi && ix >= 0 && ix < g.Wi;
      const E* xa = gX + ((size_t)(ok ? iy : 0) * g.Wi + (ok ? ix : 0)) * g.Cin + q * 8;
      const E* wb = gW + ((size_t)(ty * g.k + tx) * g.Cout + n0 + r16) * g.Cin + q * 8;
      for (int c = 0; c < nchunk; c += 2) {
        P8 a[2], b[2][NT];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const bool live = c + h < nchunk;
          a[h] = (ok && live) ? T::load8(xa + (c + h) * 32) : T::zero8();
#pragma unroll
          for (int j = 0; j < NT; ++j) b[h][j] = live ? T::load8(wb + (size_t)j * 16 * g.Cin + (c + h) * 32) : T::zero8();
        }
#pragma unroll
        for (int h = 0; h < 2; ++h)
#pragma unroll
          for (int j = 0; j < NT; ++j) acc[j] = T::mfma(b[h][j], a[h], acc[j]);
      }
    }
  }
  if (!mvalid) return;
  unsigned rm = 0u;
#pragma unroll
  for (int j = 0; j < NT; ++j) {
    const int co = n0 + j * 16 + q * 4;
    const float4 bb = *reinterpret_cast<const float4*>(g.bias + co);
    float v[4] = {acc[j][0] + bb.x, acc[j][1] + bb.y, acc[j][2] + bb.z, acc[j][3] + bb.w};
    if (g.relu) {
#pragma unroll
      for (int r = 0; r < 4; ++r) v[r] = fmaxf(v[r], 0.f);
    }
    if (g.Y) fh_store4<T>(reinterpret_cast<E*>(g.Y) + (size_t)m * g.Cout + co, v[0], v[1], v[2], v[3], rm);
    if (g.Yf32) *reinterpret_cast<float4*>(g.Yf32 + (size_t)m * g.Cout + co) = float4{v[0], v[1], v[2], v[3]};
  }
  fh_range_flush<T>(g.sat, rm);
}

// ------------------------------------------------------------------------------------------
// max_pool2d(2, 2) in floor mode on NHWC, n stacked views: (Hi, Wi) -> (Hi / 2, Wi / 2), an odd last row / column is dropped.
// One thread = one output pixel x 8 channels.
template <class T>
__global__ __launch_bounds__(256) void sfd_pool_kernel(const typename T::elem* __restrict__ in, typename T::elem* __restrict__ out,
                                                       int n, int Hi, int Wi, int C, unsigned long long* sat) {
  const int Ho = Hi >> 1, Wo = Wi >> 1, c8 = C >> 3;
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (size_t)n * Ho * Wo * c8) return;
  const int cg = (int)(idx % c8);
  const size_t p = idx / c8;  // over the n stacked views
  const size_t view = p / ((size_t)Ho * Wo), pl = p - view * ((size_t)Ho * Wo);
  const int y = (int)(pl / Wo), x = (int)(pl - (size_t)y * Wo);
  const typename T::elem* s = in + ((view * Hi + (size_t)(2 * y)) * Wi + 2 * x) * C + cg * 8;
  const typename T::pack8 a = T::load8(s), b = T::load8(s + C), c = T::load8(s + (size_t)Wi * C), d = T::load8(s + (size_t)Wi * C + C);
  typename T::pack8 o;
#pragma unroll
  for (int i = 0; i < 8; ++i) T::set(o, i, fmaxf(fmaxf(T::get(a, i), T::get(b, i)), fmaxf(T::get(c, i), T::get(d, i))));
  unsigned rm = 0u;
  fh_track_pack<T>(rm, o);
  fh_range_flush<T>(sat, rm);
  T::store8(out + p * C + cg * 8, o);
}

// ------------------------------------------------------------------------------------------
// L2Norm over channels: y[c] = x[c] / (sqrt(sum_c x^2) + 1e-10) * weight[c], the sum in fp32.  One wave per pixel (every lane
// of it reaches the cross-lane sum; lanes beyond C / 8 add 0), a lane holds 8 channels per step, C <= 1024.
template <class T>
__global__ __launch_bounds__(256) void sfd_l2norm_kernel(const typename T::elem* __restrict__ in, const float* __restrict__ weight,
                                                         typename T::elem* __restrict__ out, int npix, int C, unsigned long long* sat) {
  const int pix = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (pix >= npix) return;  // per wave
  const int c8n = C >> 3;
  typename T::pack8 v[2];
  float ss = 0.f;
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int c8 = lane + 64 * j;
    v[j] = c8 < c8n ? T::load8(in + (size_t)pix * C + c8 * 8) : T::zero8();
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const float f = T::get(v[j], i);
      ss += f * f;
    }
  }
  ss = wave_sum(ss);
  const float d = sqrtf(ss) + 1e-10f;
  unsigned rm = 0u;
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int c8 = lane + 64 * j;
    if (c8 >= c8n) continue;
    typename T::pack8 o;
#pragma unroll
    for (int i = 0; i < 8; ++i) T::set(o, i, T::get(v[j], i) / d * weight[c8 * 8 + i]);
    fh_track_pack<T>(rm, o);
    T::store8(out + (size_t)pix * C + c8 * 8, o);
  }
  fh_range_flush<T>(sat, rm);
}

// ------------------------------------------------------------------------------------------
// A level's head output [npix][16] fp32 (conf rows first, then the 4 loc rows) -> the definition's two maps, fp32 NCHW:
// conf [2][npix] (level 0's 4 conf channels maxed out: channel 0 = max of the first three, channel 1 = the fourth) and loc
// [4][npix].  raw holds n stacked views; view v's maps lie view_stride floats behind view v - 1's.
__global__ __launch_bounds__(256) void sfd_maps_kernel(const float* __restrict__ raw, float* __restrict__ conf, float* __restrict__ loc,
                                                       int n, size_t view_stride, int npix, int nconf) {
  const int pg = blockIdx.x * 256 + threadIdx.x;
  if (pg >= n * npix) return;
  const int view = pg / npix, p = pg - view * npix;
  const float* r = raw + (size_t)pg * kSfdHeadC;
  conf += view * view_stride;
  loc += view * view_stride;
  conf[p] = nconf == 4 ? fmaxf(fmaxf(r[0], r[1]), r[2]) : r[0];
  conf[(size_t)npix + p] = r[nconf - 1];
#pragma unroll
  for (int j = 0; j < 4; ++j) loc[(size_t)j * npix + p] = r[nconf + j];
}

// ------------------------------------------------------------------------------------------
// Decoding of every position (host_models.sfd_decode_dense): level i has stride s = 2^(i + 2) (level 3 too, beyond the image
// included), prior centre (s / 2 + x s, s / 2 + y s), prior size 4 s, variances (0.1, 0.2); score = 1 / (1 + exp(c0 - c1)).
// maps: per level conf [2][n] then loc [4][n] at float offset 6 * pos0[level]; dense: [P][5] = x1, y1, x2, y2, score in
// position order (level, y, x).  blockIdx.y = the view: its maps at 6 P floats, its rows at 5 P floats per view.
struct SfdGeom {
  int h[kSfdLevels], w[kSfdLevels];
  int pos0[kSfdLevels + 1];  // first position of a level; pos0[6] = P
};

__global__ __launch_bounds__(256) void sfd_decode_kernel(const float* __restrict__ maps, SfdGeom g, float* __restrict__ dense) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= g.pos0[kSfdLevels]) return;
  maps += (size_t)blockIdx.y * 6 * g.pos0[kSfdLevels];
  dense += (size_t)blockIdx.y * 5 * g.pos0[kSfdLevels];
  int l = 0;
#pragma unroll
  for (int i = 1; i < kSfdLevels; ++i) l += p >= g.pos0[i] ? 1 : 0;
  int h = 0, w = 0, p0 = 0;
#pragma unroll
  for (int i = 0; i < kSfdLevels; ++i) {
    if (i == l) h = g.h[i], w = g.w[i], p0 = g.pos0[i];
  }
  const int q = p - p0, n = h * w;
  const int y = q / w, x = q - y * w;
  const float* b = maps + (size_t)6 * p0;
  const float c0 = b[q], c1 = b[(size_t)n + q];
  const float l0 = b[(size_t)2 * n + q], l1 = b[(size_t)3 * n + q], l2 = b[(size_t)4 * n + q], l3 = b[(size_t)5 * n + q];
  const float s = (float)(4 << l);
  const float score = 1.f / (1.f + expf(c0 - c1));
  const float cx = 0.5f * s + (float)x * s + l0 * 0.1f * 4.f * s, cy = 0.5f * s + (float)y * s + l1 * 0.1f * 4.f * s;
  const float bw = 4.f * s * expf(0.2f * l2), bh = 4.f * s * expf(0.2f * l3);
  float* o = dense + (size_t)p * 5;
  o[0] = cx - 0.5f * bw;
  o[1] = cy - 0.5f * bh;
  o[2] = cx + 0.5f * bw;
  o[3] = cy + 0.5f * bh;
  o[4] = score;
}

// ------------------------------------------------------------------------------------------
// Selection in ONE workgroup per view (blockIdx.x = the view; host_models.sfd_select): the positions with score > score_thr are compacted in position order by
// a ballot prefix scan (no atomic cursor: the order never depends on timing), ranked by (score descending, position ascending)
// in LDS, and run through the greedy NMS (`+1` areas, a box is dropped when its IoU with a kept one EXCEEDS iou_thr).
// boxes: up to max_boxes rows of 5 floats in keep order; counts = {kept, candidates}, both the TRUE numbers: with
// candidates > cap nothing is selected (kept = 0) and the caller runs the definition on `dense`, which stays valid.
// Per view: P dense rows, max_boxes rows of boxes, 2 counts.  Dynamic LDS: cap * 32 bytes.
__global__ __launch_bounds__(256) void sfd_select_kernel(const float* __restrict__ dense, int P, float score_thr, float iou_thr, int cap,
                                                         int max_boxes, float* __restrict__ boxes, int* __restrict__ counts) {
  extern __shared__ float s_dyn[];
  float* s_box = s_dyn;                                  // [cap][4]
  float* s_score = s_dyn + (size_t)cap * 4;              // [cap]
  int* s_pos = reinterpret_cast<int*>(s_score + cap);    // [cap]
  int* s_ord = s_pos + cap;                              // [cap]: rank -> candidate
  int* s_sup = s_ord + cap;                              // [cap]: by rank
  __shared__ int s_wtot[4];
  __shared__ int s_base;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  dense += (size_t)blockIdx.x * P * 5;
  boxes += (size_t)blockIdx.x * max_boxes * 5;
  counts += blockIdx.x * 2;
  if (tid == 0) s_base = 0;
  __syncthreads();
  for (int base = 0; base < P; base += 256) {
    const int p = base + tid;
    const float sc = p < P ? dense[(size_t)p * 5 + 4] : 0.f;
    const bool f = p < P && sc > score_thr;
    const unsigned long long m = __ballot(f);
    if (lane == 0) s_wtot[wv] = __popcll(m);
    __syncthreads();
    int idx = s_base + __popcll(m & ((1ull << lane) - 1ull));
    for (int j = 0; j < wv; ++j) idx += s_wtot[j];
    if (f && idx < cap) {
      s_score[idx] = sc;
      s_pos[idx] = p;
#pragma unroll
      for (int j = 0; j < 4; ++j) s_box[idx * 4 + j] = dense[(size_t)p * 5 + j];
    }
    __syncthreads();
    if (tid == 0) s_base += s_wtot[0] + s_wtot[1] + s_wtot[2] + s_wtot[3];
    __syncthreads();
  }
  const int total = s_base;
  if (total > cap) {
    if (tid == 0) counts[0] = 0, counts[1] = total;
    return;
  }
  const int n = total;
  for (int i = tid; i < n; i += 256) {
    const float si = s_score[i];
    const int pi = s_pos[i];
    int r = 0;
    for (int j = 0; j < n; ++j) r += (s_score[j] > si || (s_score[j] == si && s_pos[j] < pi)) ? 1 : 0;
    s_ord[r] = i;
    s_sup[i] = 0;
  }
  __syncthreads();
  int kept = 0;
  for (int k = 0; k < n; ++k) {
    if (!s_sup[k]) {  // uniform: written before the barrier that ended the last round
      const int i = s_ord[k];
      const float x1 = s_box[i * 4], y1 = s_box[i * 4 + 1], x2 = s_box[i * 4 + 2], y2 = s_box[i * 4 + 3];
      const float ai = (x2 - x1 + 1.f) * (y2 - y1 + 1.f);
      for (int r = k + 1 + tid; r < n; r += 256) {
        if (s_sup[r]) continue;
        const int j = s_ord[r];
        const float u1 = s_box[j * 4], v1 = s_box[j * 4 + 1], u2 = s_box[j * 4 + 2], v2 = s_box[j * 4 + 3];
        const float iw = fmaxf(0.f, fminf(x2, u2) - fmaxf(x1, u1) + 1.f), ih = fmaxf(0.f, fminf(y2, v2) - fmaxf(y1, v1) + 1.f);
        const float inter = iw * ih;
        if (inter / (ai + (u2 - u1 + 1.f) * (v2 - v1 + 1.f) - inter) > iou_thr) s_sup[r] = 1;
      }
      if (tid == 0 && kept < max_boxes) {
        float* o = boxes + (size_t)kept * 5;
        o[0] = x1, o[1] = y1, o[2] = x2, o[3] = y2, o[4] = s_score[i];
      }
      ++kept;
    }
    __syncthreads();
  }
  if (tid == 0) counts[0] = kept, counts[1] = total;
}
