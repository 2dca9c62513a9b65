// The encoder handle (float_enc_t): packed weights and the source portrait's activations, shared by the once-per-clip
// appearance pass (enc_api.hip) and the per-frame motion pass over stacked driving frames (encm_api.hip).
#pragma once
#include "common.hpp"
#include "enc_fir.hpp"
#include "tuning.hpp"

struct EConv {
  void* W = nullptr;     // [k*k][Cout][Cin] T::elem, equalised-lr scale folded in
  float* bias = nullptr; // [Cout] FusedLeakyReLU bias or nullptr
  int cin = 0, cout = 0, k = 0;
};

struct ResBlk {
  EConv conv1, conv2, skip;
  int R = 0;  // input resolution
  EncFir fir2, firs;  // the Blur in front of conv2 / of the skip conv, flipped (enc_blur_taps)
};

struct FcLayer {
  float* W = nullptr;
  float* b = nullptr;
  int n = 0, k = 0;
};

// Scratch of the motion pass for `block` stacked frames (float_enc_motion_reserve).  It belongs to that pass alone: nothing
// the appearance pass leaves in the handle (res[], s_r) is read or written through it.
struct EncMotion {
  int block = 0;
  void *xa = nullptr, *xb = nullptr, *t1 = nullptr;  // [block][R][R][C] T::elem: level input / output (ping-pong), conv1 output
  float *s = nullptr, *fa = nullptr, *fb = nullptr;  // [block][dim]: rows of the 4x4 -> 1x1 conv, Encoder.fc ping-pong
  size_t bytes = 0;
  void release() {
    for (void* p : {xa, xb, t1, (void*)s, (void*)fa, (void*)fb})
      if (p) (void)hipFree(p);
    *this = EncMotion();
  }
};

struct float_enc {
  float_enc_cfg_t cfg;
  EncTune tune;
  DevicePool pool;
  int C0 = 0;
  float *w0 = nullptr, *b0 = nullptr;  // convs.0: [C0][3] scaled, [C0]
  std::vector<ResBlk> blocks;
  EConv last;                          // EqualConv2d(C, dim, 4, padding 0, no bias)
  std::vector<FcLayer> fc;
  float* Q = nullptr;                  // [dim][dim_motion] of QR(direction.weight + 1e-8), or nullptr
  // activations: res[i] (NHWC 16-bit) for i = 0..n_blocks (res[0] = convs.0 output), scratch for
  // conv1 output, the two blurred images and the skip branch
  std::vector<void*> res;  // T::elem
  std::vector<int> resR, resC;
  void *t1 = nullptr, *tb = nullptr, *tsk = nullptr;
  float *s_r = nullptr, *fcA = nullptr, *fcB = nullptr;
  unsigned long long* sat = nullptr;  // range counter of every 16-bit activation store (float_enc_saturation): conv1 of the ResBlocks runs the decoder's kernel (overflow -> inf, counted), the other layers clamp at 65504 and count
  EncMotion motion;
};
