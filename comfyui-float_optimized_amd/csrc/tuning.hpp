// Every environment switch of the native library, in one place.  A handle reads its record ONCE, in its create function
// (FmtTune::from_env() and friends - the only code under csrc/ that looks at the environment), and keeps it for its lifetime:
// what a handle launches depends on the environment it was created under and on nothing that happens afterwards.  Functions that
// have no handle (the GEMM service, the decoder's unit operators) take the record as a parameter.  Host-only C++.
#pragma once
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <string>

// The decoder's rule: a whole number inside [lo, hi], anything else falls back to the default.
inline int env_int(const char* name, int dflt, int lo, int hi) {
  const char* v = getenv(name);
  if (!v || !*v) return dflt;
  char* end = nullptr;
  const long x = strtol(v, &end, 10);
  return (end && *end == 0 && x >= lo && x <= hi) ? (int)x : dflt;
}
// The FMT's rule: plain atoi when the variable is set.
inline int env_atoi(const char* name, int dflt) {
  const char* v = getenv(name);
  return v ? atoi(v) : dflt;
}
inline bool env_set(const char* name) { return getenv(name) != nullptr; }
// A list as sscanf("%d,%d,...") (sep ',') or sscanf("%lf %lf ...") (sep ' ') reads it: up to n numbers, the entries the text does
// not reach keep their value; returns how many were read.
inline int env_scan(const char* s, int* v) { int n = 0; return sscanf(s, "%d%n", v, &n) == 1 ? n : 0; }
inline int env_scan(const char* s, double* v) { int n = 0; return sscanf(s, "%lf%n", v, &n) == 1 ? n : 0; }
template <class V>
int env_list(const char* name, V* v, int n, char sep = ',') {
  const char* s = getenv(name);
  int got = 0;
  while (s && got < n) {
    const int used = env_scan(s, v + got);
    if (!used) break;
    ++got;
    s += used;
    if (sep == ',' && *s++ != ',') break;
  }
  return got;
}

// A per-layer tiling override of the one-clip chain: (row tiles, column tiles, K-splitting waves) per workgroup.
struct LayerPlan {
  int v[3] = {0, 0, 0};
  bool on() const { return v[0] > 0; }
};

enum { RB_QKV = 0, RB_PROJ, RB_FC1, RB_FC2 };

struct FmtTune {
  bool wide = true;      // FLOAT_FMT_WIDE=0 falls back to the generic tiling for the fused adaLN projection (A/B measurement)
  int wide_variant = 7;  // FLOAT_FMT_WIDE_VARIANT: 6 / 7 = LDS-DMA 192 x 320 tile where the shape allows (else 2): lock step / wave rows half a step apart; register-staged 192 x 128 family: 0 = 96 rows x 4 k-blocks per chunk, 1 = 96 x 2, 2 = 192 x 2, 3 = 192 x 4, 4 / 5 = 8 waves
  bool big = true;       // FLOAT_FMT_BIG=0 keeps the one-tile-per-workgroup kernels on rows padded per evaluation instead of the persistent projection kernel (the A/B switch)
  bool rb = true;        // FLOAT_FMT_RB=0 keeps the 48 x 64 tiling for stacked clips instead of the row-blocked LDS-DMA tile (the A/B switch)
  // FLOAT_FMT_RB_TOUCH = k-blocks of every weight column tile the LayerNorm in front of a row-blocked GEMM pulls (0 = off).
  // Measured, ms per 250 evaluations of 4 / 16 clips: none 152.2 / 408.4, 4 k-blocks 151.8, 8: 151.4, 16: 150.6 / 404.6 (kept),
  // 32 (the whole K of every tile): 150.8 / 410.0.
  int rb_touch = 16;
  struct Rb {
    int n = 0, shape = -1, ksplit = 1;  // n = numbers given (0: no override)
  } rb_layer[4];        // FLOAT_FMT_RB_QKV / _PROJ / _FC1 / _FC2 = "shape[,ksplit]": row-blocked tile 0 = 96 x 64, 1 = 96 x 128, 2 = 192 x 128 (< 0: the weight-streaming tiling); ksplit 1 | 2 | 4 | 8, proj and fc2 only
  int full_nw = 8;       // FLOAT_FMT_FULL_NW: waves of the full-height (CFG epilogue) tiling, 8 or 4
  int plan[6] = {0, 0, 0, 0, 0, 0};  // FLOAT_FMT_PLAN="mtw,nt,nw (narrow), mtw,nt,nw (wide)": tiling of the CFG-batched shapes, tuning aid
  LayerPlan plan_layer[4];           // FLOAT_FMT_PLAN_QKV / _PROJ / _FC1 / _FC2 = "mtw,nt,nw": per-layer tiling of the one-clip chain, tuning aid
  int fc2_split = 4;     // FLOAT_FMT_FC2_SPLIT: K slices of mlp.fc2 whose sum the next LayerNorm folds, 1 | 2 | 4 (0 = in-GEMM gate*residual epilogue)
  int proj_split = 0;    // FLOAT_FMT_PROJ_SPLIT: same for attn.proj
  // FLOAT_FMT_TOUCH bit mask - who pulls whose weights: 1 LayerNorm -> qkv and fc1 (64: only LN2 -> fc1, 128: only LN1 -> qkv),
  // 2 attention -> proj, 4 fc1 -> fc2, 8 qkv -> proj, 16 proj -> fc1, 32 fc2 -> the next block's qkv / the head.
  // Default 2 + 4 + 32 + 128 (r01, ms per 250 evaluations, same box: none 90.8, 2+4 87.6, 4+32 86.0-86.7, 2+4+32 83.2-83.5 after the
  // head change, + LN1 -> qkv 82.5; touching fc1's weights - from LayerNorm, proj or qkv - never paid).
  // Round 2, with the adaLN weights out of the step (105 MB less cycling through the Infinity Cache per evaluation): LN2 -> fc1
  // now pays too: 230 = 166 + 64 gives 83.6 vs 84.9 ms (proj -> fc1 instead: 85.8; attention or qkv as extra pullers: 85.2-86.0).
  int touch = 230;
  bool hoist = true;     // FLOAT_FMT_HOIST=0 launches the adaLN projection once per evaluation instead of once per batch of evaluations (bitwise the same numbers; the A/B switch)
  int zgroup = 0;        // FLOAT_FMT_ZGROUP: column blocks of an XCD that share activation tiles through L2; 0 = per kernel: 4 (fmt_gemm_wide_kernel), 2 (fmt_gemm_dma_kernel)
  int ln_rows = 1;       // FLOAT_FMT_LN_ROWS: rows (waves) per LayerNorm workgroup, 1..4 (4 rows per workgroup: +0.4 %)
  int attn_qpw = 8, attn_lpq = 16;  // FLOAT_FMT_ATTN="qpw,lpq": queries per workgroup / lanes per query, 16 or 8 (r01: 16 lanes 81.5-81.9 ms per 250 evaluations, 8 lanes 82.3-82.9)
  bool no_tokblk = false;  // FLOAT_FMT_NO_TOKBLK (set at all): the all-rows-per-workgroup head GEMM for one clip, at most 15 row tiles (a debugging aid)
  bool pack_host = false;  // FLOAT_PACK_HOST=1 packs the weights in the host loop instead of on the device (the A/B switch; equal bit for bit)

  static FmtTune from_env() {
    FmtTune t;
    t.wide = env_atoi("FLOAT_FMT_WIDE", 1) != 0;
    t.wide_variant = env_atoi("FLOAT_FMT_WIDE_VARIANT", t.wide_variant);
    t.big = env_atoi("FLOAT_FMT_BIG", 1) != 0;
    t.rb = env_atoi("FLOAT_FMT_RB", 1) != 0;
    t.rb_touch = env_atoi("FLOAT_FMT_RB_TOUCH", t.rb_touch);
    static const char* const layers[4] = {"QKV", "PROJ", "FC1", "FC2"};
    for (int l = 0; l < 4; ++l) {
      const std::string s = layers[l];
      int rb[2] = {-1, 1};
      t.rb_layer[l].n = env_list(("FLOAT_FMT_RB_" + s).c_str(), rb, 2);
      t.rb_layer[l].shape = rb[0];
      t.rb_layer[l].ksplit = rb[1];
      env_list(("FLOAT_FMT_PLAN_" + s).c_str(), t.plan_layer[l].v, 3);
    }
    t.full_nw = env_atoi("FLOAT_FMT_FULL_NW", t.full_nw);
    env_list("FLOAT_FMT_PLAN", t.plan, 6);
    t.fc2_split = env_atoi("FLOAT_FMT_FC2_SPLIT", t.fc2_split);
    t.proj_split = env_atoi("FLOAT_FMT_PROJ_SPLIT", t.proj_split);
    t.touch = env_atoi("FLOAT_FMT_TOUCH", t.touch);
    t.hoist = env_atoi("FLOAT_FMT_HOIST", 1) != 0;
    t.zgroup = std::max(0, env_atoi("FLOAT_FMT_ZGROUP", 0));
    t.ln_rows = std::max(1, std::min(4, env_atoi("FLOAT_FMT_LN_ROWS", 1)));
    int attn[2] = {t.attn_qpw, t.attn_lpq};
    env_list("FLOAT_FMT_ATTN", attn, 2);
    t.attn_lpq = attn[1] == 16 ? 16 : 8;
    t.attn_qpw = std::max(1, std::min(512 / t.attn_lpq, attn[0]));
    t.no_tokblk = env_set("FLOAT_FMT_NO_TOKBLK");
    t.pack_host = env_atoi("FLOAT_PACK_HOST", 0) != 0;
    return t;
  }
};

struct DecTune {
  // FLOAT_DEC_LDS_PAD=<bytes>, 0..163840: every launch of the level kernels (3x3 conv, up-conv + blur, flow) asks for at least that
  // much dynamic LDS, i.e. the decoder's occupancy is capped (82 000: ONE workgroup per CU instead of two - room for a 98-KB workgroup
  // of the FMT chain beside it when the two stages overlap on two streams, pipeline.generate_to_host_overlap).  0 = off.
  int lds_pad = 0;
  // Ride-along hand-over (float_dec_frames_host): copy workgroups per carrying launch (FLOAT_DEC_RIDE_WGS, 0..64, rounded down to a
  // multiple of 8; 0 = no launch carries), the lowest resolution whose launches carry a share (FLOAT_DEC_RIDE_MIN_RES, 64..512), and
  // the pause between a wave's 1-KiB stores in units of 512 clocks (FLOAT_DEC_RIDE_PACE, 0..64).  Unpaced, the copy saturates PCIe
  // (55 GB/s) and its posted writes queue in front of the compute workgroups' memory traffic: the 512-px flow launch took 665 us
  // instead of 508 with a 217 us copy inside; at ~45 GB/s (16 workgroups, pace 4) it takes 548 (in-kernel stamps, -DDEC_STAMPS).
  // Round 3: the launches got shorter (flow kernel -35 %), pace 3 (~52 GB/s) leaves less of the last share exposed: 27.66 vs 28.03
  // ms per 250 frames.
  unsigned ride_wgs = 16;
  int ride_min_res = 64;
  unsigned ride_pace = 3;
  // FLOAT_DEC_RIDE_W="12 numbers" in (0, 1e6): weight of a carrying launch, rows 64 / 128 / 256 / 512 px x (up-conv, conv2, flow) -
  // launch durations (tools/probes/trace_sequence.py on the round-3 kernels: {203,155,61},{178,175,118},{242,226,215},{318,256,336})
  // shifted toward the flow launches, which absorb a share without getting longer while the 512-px convs are stretched by theirs
  // (a trace of the carrying batch: +49 / +56 us there, +6 on the flow launch): 26.35 vs 26.80 ms per 250 frames decode + hand-over
  // round 6 (launches now {178,142,52},{158,155,99},{220,206,175},{277,235,146}: the last level's flow launch is a third of what it
  // was): decode + hand-over per 250 frames 25.1-25.3 ms with the row below against 26.4-26.9 with round 5's {..,{290,225,370}},
  // 25.4 / 25.7 / 25.3 / 25.6 for four neighbours, 26.8 with equal shares (tools/probes/dec_host2.py)
  double ride_w[4][3] = {{170, 140, 50}, {170, 155, 100}, {220, 200, 180}, {300, 250, 120}};
  bool cb_order = true;    // FLOAT_DEC_CB_ORDER=0: output-channel blocks as grid.y (the round-1 order; A/B switch of dec_group_cb)
  // Output channels per workgroup of the 3x3 conv: FLOAT_DEC_CONV_BN = 32 | 64 in the 16x16-tile kernel (64 where the layer has them:
  // each A fragment feeds twice the MFMAs - 22.75 vs 23.10 ms per 250 frames since the kernel's address arithmetic went; before that
  // the 32-channel tiles' doubled workgroup count won, 33.9 vs 35.2), FLOAT_DEC_CONV_BN_LO = 32 | 64 in the generic low-resolution
  // kernel (the A/B switches)
  int conv_bn = 64, conv_bn_lo = 32;
  int tpw = 0;             // FLOAT_DEC_TPW, 1..4096: tiles per workgroup of the 16x16-tile conv (0 = by tile count: 4 / 2 / 1), tuning aid
  bool no_zfuse = false;   // FLOAT_DEC_NO_ZFUSE (set at all): the transposed conv class by class through the generic kernel instead of dec_zconv4_kernel
  int zblur_min = 64;      // FLOAT_DEC_ZBLUR_MIN, 16..4096: transposed conv + blur in one launch from this resolution up
  int flow_pix = 0;        // FLOAT_DEC_FLOW_PIX = 1 | 2 | 4: pixels per lane group and iteration of dec_flow_kernel (0 = by channel count), tuning aid
  int flow_wgs = 2048;     // FLOAT_DEC_FLOW_WGS, 8..2^20: workgroups of a dec_flow_kernel launch (8 per CU)
  bool flow_epi = true;    // FLOAT_DEC_FLOW_EPI=0 keeps dec_flow_kernel on the last level instead of ToFlow in conv2's epilogue
  bool yuv_fused = true;   // FLOAT_DEC_YUV_FUSED=0: I420 frames through u8 RGB + dec_rgb8_to_i420_kernel on the product path too (A/B switch, tests)
  bool write_pyr = false;  // FLOAT_DEC_WRITE_PYR (set at all): the last level stores its flow / rgb pyramids too
  bool copy_memcpy = false;  // FLOAT_DEC_COPY=memcpy: same-stream hand-over by hipMemcpyAsync instead of ride-along copy workgroups
  bool style_norm = true;    // FLOAT_DEC_STYLE_NORM=0: styles are not divided by their max |s| before the demodulation

  static DecTune from_env() {
    DecTune t;
    t.lds_pad = env_int("FLOAT_DEC_LDS_PAD", 0, 0, 160 * 1024);
    t.ride_wgs = (unsigned)env_int("FLOAT_DEC_RIDE_WGS", 16, 0, 64) / 8 * 8;
    t.ride_min_res = env_int("FLOAT_DEC_RIDE_MIN_RES", 64, 64, 512);
    t.ride_pace = (unsigned)env_int("FLOAT_DEC_RIDE_PACE", 3, 0, 64);
    double w[12];
    if (env_list("FLOAT_DEC_RIDE_W", w, 12, ' ') == 12)
      for (int i = 0; i < 12; ++i)
        if (w[i] > 0.0 && w[i] < 1e6) t.ride_w[i / 3][i % 3] = w[i];
    t.cb_order = env_atoi("FLOAT_DEC_CB_ORDER", 1) != 0;
    t.conv_bn = env_int("FLOAT_DEC_CONV_BN", 64, 32, 64);
    t.conv_bn_lo = env_int("FLOAT_DEC_CONV_BN_LO", 32, 32, 64);
    t.tpw = env_int("FLOAT_DEC_TPW", 0, 0, 4096);
    t.no_zfuse = env_set("FLOAT_DEC_NO_ZFUSE");
    t.zblur_min = env_int("FLOAT_DEC_ZBLUR_MIN", 64, 16, 4096);
    t.flow_pix = env_int("FLOAT_DEC_FLOW_PIX", 0, 0, 4);
    t.flow_wgs = env_int("FLOAT_DEC_FLOW_WGS", 2048, 8, 1 << 20);
    t.flow_epi = env_int("FLOAT_DEC_FLOW_EPI", 1, 0, 1) != 0;
    t.yuv_fused = env_int("FLOAT_DEC_YUV_FUSED", 1, 0, 1) != 0;
    t.write_pyr = env_set("FLOAT_DEC_WRITE_PYR");
    const char* copy = getenv("FLOAT_DEC_COPY");
    t.copy_memcpy = copy && !strcmp(copy, "memcpy");
    t.style_norm = env_int("FLOAT_DEC_STYLE_NORM", 1, 0, 1) != 0;
    return t;
  }
};

struct EncTune {
  bool no_tiles = false;  // FLOAT_ENC_NO_TILES (set at all): the ResBlocks' conv1 through the generic 3x3 kernel instead of the decoder's LDS-staged one
  static EncTune from_env() { return EncTune{env_set("FLOAT_ENC_NO_TILES")}; }
};

struct AudTune {
  bool attn_mfma = true;  // FLOAT_AUD_ATTN_MFMA=0: one wave per query instead of the matrix-pipe attention kernel
  static AudTune from_env() { return AudTune{env_atoi("FLOAT_AUD_ATTN_MFMA", 1) != 0}; }
};
