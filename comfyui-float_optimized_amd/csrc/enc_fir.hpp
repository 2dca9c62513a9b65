// The 16 taps of the Blur of a down-sampling ConvLayer of the encoder (enc_blur_kernel, encm_tail_kernel):
// k[a][b] = weight of in[Y + a - pad][X + b - pad] = the layer's `kernel` buffer flipped in both axes.
#pragma once

struct EncFir {
  float k[16];
};
