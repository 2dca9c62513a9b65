// C-ABI entry points of the encoder's motion pass (include/float_hip.h, section "encoder"): one lambda row per driving frame
// (reference encoder.py:262-277, `fc(net_app(input_target))`) for T stacked 8-bit frames, and the driving rows of
// Synthesis.forward (styledecoder.py:497-508).  The frames go through in blocks of `block` frames with a scratch of their
// own; the handle's source-portrait state (res[], s_r, the maps behind float_enc_feats16) is never touched.
#include <math.h>

#include "dec_kernels.hpp"  // dec_conv16_kernel / dec_conv_kernel: the LDS-tiled 3x3 convs of the decoder take [F][R][R][C] as they are
#include "enc_handle.hpp"
#include "encm_kernels.hpp"

namespace {

constexpr size_t kLdsMax = 160 * 1024;  // per workgroup on gfx950

template <class T>
int reserve_impl(float_enc* h, int block) {
  typedef typename T::elem E;
  EncMotion& m = h->motion;
  if (m.block == block) return FLOAT_OK;
  FH_CHECK_HIP(hipDeviceSynchronize());  // a motion call on any stream may still use the old scratch
  m.release();
  const float_enc_cfg_t& c = h->cfg;
  size_t in0 = (size_t)c.size * c.size * h->C0, rest = 0;  // level 0's input; the largest map below it
  for (size_t l = 1; l < h->resR.size(); ++l) rest = std::max(rest, (size_t)h->resR[l] * h->resR[l] * h->resC[l]);
  size_t t1 = 0;
  for (const ResBlk& B : h->blocks) t1 = std::max(t1, (size_t)B.R * B.R * B.conv1.cout);
  const size_t rows = (size_t)block * std::max(c.dim, 64) * sizeof(float);
  const size_t want[6] = {block * in0 * sizeof(E), block * rest * sizeof(E), block * t1 * sizeof(E), rows, rows, rows};
  void** dst[6] = {&m.xa, &m.xb, &m.t1, (void**)&m.s, (void**)&m.fa, (void**)&m.fb};
  for (int i = 0; i < 6; ++i) {
    const hipError_t e = hipMalloc(dst[i], want[i]);
    if (e != hipSuccess) {
      m.release();
      fh_set_error("float_enc_motion_reserve: hipMalloc(%zu) for %d frames failed: %s", want[i], block, hipGetErrorString(e));
      return FLOAT_E_NOMEM;
    }
    m.bytes += want[i];
  }
  m.block = block;
  // dynamic LDS above the 64 KiB default
  auto raise = [](auto kern, size_t bytes) { (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes); };
  raise(encm_tail_kernel<T, 4>, kLdsMax);
  raise(encm_tail_kernel<T, 2>, kLdsMax);
  raise(dec_conv16_kernel<T, 2, 3, 3>, (size_t)32 * 1024 * T::EB);
  raise(dec_conv_kernel<T, 2>, (size_t)32 * 1024 * T::EB);
  (void)hipGetLastError();
  return FLOAT_OK;
}

// conv1 of a ResBlock - EqualConv2d(C, C, 3, padding 1) + FusedLeakyReLU - for F stacked frames on the decoder's kernels:
// 16 x 16 tiles of one frame over a (frame, tile) grid from 16 px up (the kernel enc_api.hip runs per image; its tile cursor
// carries the frame), and below that the generic kernel whose 256 rows of M hold 4 whole 8-px frames or 16 whole 4-px frames,
// each staged with its own zero border, behind one weight slab per chunk.
template <class T>
int launch_conv1(float_enc* h, const EConv& L, const void* X, int R, int F, void* Y, hipStream_t st) {
  constexpr size_t RB = 32 * T::EB;
  ConvArgs g;
  memset(&g, 0, sizeof(g));
  g.X = X, g.Wt = L.W, g.Y = Y;
  g.bias = L.bias, g.act = 1;
  g.sat = h->sat, g.F = F;
  g.Hi = g.Wi = g.Ho = g.Wo = g.OH = g.OW = R;
  g.Cin = L.cin, g.Cout = L.cout;
  g.sy = g.sx = 1;
  g.ntaps = 9;
  for (int t = 0; t < 9; ++t) g.dy[t] = (signed char)(t / 3 - 1), g.dx[t] = (signed char)(t % 3 - 1);
  g.dymin = g.dxmin = -1;
  const unsigned ncb = (unsigned)(L.cout / 32);
  if (R >= 16) {
    g.tiles_x = g.tiles_y = R / 16;
    g.tpw = 1;
    const unsigned ngroups = (unsigned)(g.tiles_x * g.tiles_y * F);
    dim3 grid(ngroups, ncb);
    if (ncb > 1) {  // the channel blocks of a tile side by side on one XCD (dec_group_cb)
      g.ngroups = ngroups, g.ncb = ncb;
      grid = dim3(ngroups * ncb, 1);
    }
    const size_t smem = (size_t)18 * 18 * RB + (size_t)9 * 32 * RB + 3 * 32 * sizeof(float);  // halo, weights, epilogue operands
    hipLaunchKernelGGL((dec_conv16_kernel<T, 2, 3, 3>), grid, dim3(256), smem, st, g);
  } else {
    FH_REQUIRE(R == 8 || R == 4, "conv1 of the motion pass: unexpected resolution %d", R);
    g.lth = g.ltw = R == 8 ? 3 : 2;
    g.lnf = 8 - 2 * g.lth;
    g.hh = g.hw = R + 2;
    g.tiles_x = g.tiles_y = 1;
    const int nf = 1 << g.lnf, npix = nf * g.hh * g.hw;
    const size_t smem = (size_t)npix * RB + (size_t)9 * 32 * RB;
    hipLaunchKernelGGL((dec_conv_kernel<T, 2>), dim3((unsigned)((F + nf - 1) / nf), ncb), dim3(256), smem, st, g);
  }
  FH_CHECK_HIP(hipGetLastError());
  return FLOAT_OK;
}

template <class T, int NT>
int launch_tail_nt(float_enc* h, const ResBlk& B, const void* t1, const void* x, int F, void* y, hipStream_t st) {
  EncmTailArgs g;
  memset(&g, 0, sizeof(g));
  g.T1 = t1, g.X = x, g.Y = y;
  g.W2 = B.conv2.W, g.Ws = B.skip.W, g.bias = B.conv2.bias;
  g.F = F, g.R = B.R, g.C = B.conv2.cin, g.Cout = B.conv2.cout;
  const int Ro = B.R / 2;
  g.lto = Ro >= 8 ? 3 : (Ro == 4 ? 2 : 1);
  g.lnf = 6 - 2 * g.lto;  // 64 rows of M
  while (g.lnf > 0 && encm_tail_lds<T, NT>(g.lto, g.lnf) > kLdsMax) --g.lnf;
  const size_t smem = encm_tail_lds<T, NT>(g.lto, g.lnf);
  FH_REQUIRE(smem <= kLdsMax, "ResBlock tail: %zu bytes of LDS", smem);
  g.tiles = Ro >> g.lto;
  g.fir2 = B.fir2, g.firs = B.firs;
  g.sat = h->sat;
  const int nf = 1 << g.lnf;
  dim3 grid((unsigned)(g.tiles * g.tiles * ((F + nf - 1) / nf)), (unsigned)(g.Cout / (NT * 16)));
  hipLaunchKernelGGL((encm_tail_kernel<T, NT>), grid, dim3(256), smem, st, g);
  FH_CHECK_HIP(hipGetLastError());
  return FLOAT_OK;
}

// 64 output channels per workgroup with 16-bit operands where the layer has them (the blurred tiles are formed once per
// channel block), 32 in the fp32 verification mode (twice the bytes per LDS row)
template <class T>
int launch_tail(float_enc* h, const ResBlk& B, const void* t1, const void* x, int F, void* y, hipStream_t st) {
  if (!T::is32 && B.conv2.cout % 64 == 0) return launch_tail_nt<T, 4>(h, B, t1, x, F, y, st);
  return launch_tail_nt<T, 2>(h, B, t1, x, F, y, st);
}

template <class T>
int motion_impl(float_enc* h, const uint8_t* frames, int T_, float* lam, hipStream_t st) {
  typedef typename T::elem E;
  const float_enc_cfg_t& c = h->cfg;
  const EncMotion& m = h->motion;
  const int nb = (int)h->blocks.size();
  const size_t fpix = (size_t)c.size * c.size;
  int rc;
  for (int t0 = 0; t0 < T_; t0 += m.block) {
    const int F = std::min(m.block, T_ - t0);
    {
      const size_t tot = F * fpix * (h->C0 / 8);
      hipLaunchKernelGGL((encm_first_kernel<T>), dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, st, frames + t0 * fpix * 3, h->w0, h->b0,
                         reinterpret_cast<E*>(m.xa), F * fpix, h->C0, h->sat);
    }
    void *x = m.xa, *y = m.xb;
    for (int b = 0; b < nb; ++b) {
      const ResBlk& B = h->blocks[b];
      if ((rc = launch_conv1<T>(h, B.conv1, x, B.R, F, m.t1, st))) return rc;
      if ((rc = launch_tail<T>(h, B, m.t1, x, F, y, st))) return rc;
      std::swap(x, y);
    }
    // EqualConv2d(C, dim, 4) and Encoder.fc as GEMMs over the block's rows; the last layer writes the caller's lambda rows
    hipLaunchKernelGGL((encm_last_kernel<T>), dim3((unsigned)(c.dim / 16), (unsigned)((F + 15) / 16)), dim3(256), 0, st,
                       reinterpret_cast<const E*>(x), reinterpret_cast<const E*>(h->last.W), m.s, F, h->last.cin, c.dim);
    const float* cur = m.s;
    float* pp[2] = {m.fa, m.fb};
    for (size_t j = 0; j < h->fc.size(); ++j) {
      const FcLayer& L = h->fc[j];
      const bool lastl = j + 1 == h->fc.size();
      float* dst = lastl ? lam + (size_t)t0 * c.dim_motion : pp[j & 1];
      hipLaunchKernelGGL(encm_fc_kernel, dim3((unsigned)((L.n + 3) / 4), (unsigned)((F + 7) / 8)), dim3(256), 0, st, cur, L.W, L.b,
                         1.0f / sqrtf((float)L.k), dst, F, L.n, L.k, L.n);
      cur = dst;
    }
    FH_CHECK_HIP(hipGetLastError());
  }
  return FLOAT_OK;
}

template <class F>
int by_dtype(float_enc* h, F&& f) {
  if (h->cfg.dtype == FLOAT_DT_FP32) return f(FP32());
  return h->cfg.dtype == FLOAT_DT_BF16 ? f(BF16()) : f(FP16());
}

}  // namespace

extern "C" {

int float_enc_motion_reserve(float_enc_t* h, int32_t block) {
  FH_REQUIRE(h, "null argument to float_enc_motion_reserve");
  FH_REQUIRE(block >= 1, "float_enc_motion_reserve: block must be at least 1 frame (got %d)", block);
  return by_dtype(h, [&](auto t) { return reserve_impl<decltype(t)>(h, block); });
}

int float_enc_motion(float_enc_t* h, const uint8_t* frames, int32_t T, float* lam, void* stream) {
  FH_REQUIRE(h && frames && lam, "null argument to float_enc_motion");
  FH_REQUIRE(T >= 1, "float_enc_motion: T must be at least 1 frame (got %d)", T);
  if (h->motion.block == 0) {
    const int rc = float_enc_motion_reserve(h, 8);
    if (rc) return rc;
  }
  return by_dtype(h, [&](auto t) { return motion_impl<decltype(t)>(h, frames, T, lam, (hipStream_t)stream); });
}

int float_enc_drive_rows(float_enc_t* h, const float* lam, int32_t T, int32_t mode, const float* lam_source, const float* lam_start,
                         float* r_d, void* stream) {
  FH_REQUIRE(h && lam && r_d, "null argument to float_enc_drive_rows");
  FH_REQUIRE(T >= 1, "float_enc_drive_rows: T must be at least 1 row (got %d)", T);
  FH_REQUIRE(mode == 0 || mode == 1, "float_enc_drive_rows: mode must be 0 (absolute) or 1 (relative), got %d", mode);
  FH_REQUIRE(h->Q != nullptr, "float_enc_drive_rows: the encoder was created without 'direction.weight'");
  FH_REQUIRE(mode == 0 || lam_source != nullptr, "float_enc_drive_rows: the relative mode needs lam_source");
  const size_t tot = (size_t)T * h->cfg.dim;
  hipLaunchKernelGGL(encm_rows_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, (hipStream_t)stream, lam, lam_source,
                     lam_start ? lam_start : lam, h->Q, r_d, T, h->cfg.dim, h->cfg.dim_motion, mode);
  FH_CHECK_HIP(hipGetLastError());
  return FLOAT_OK;
}

}  // extern "C"
