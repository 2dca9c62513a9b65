// Source policy of float_img_front_frames_planes (include/float_hip.h): the frame-stacked front end reading planar or
// semi-planar YUV as a decoder hands it out - 8, 10 or 12 bits, 4:2:0, 4:2:2 or 4:4:4, odd sides, pitched rows, planes at any
// byte offset of the frame, 16-bit samples low- or high-aligned.  The work split, the taps and the 64-bit totals in registers are
// imgv_frames_kernel's (imgv_kernels.hpp), unchanged; this file is only its staging stage, the sibling of ImgySrc
// (imgy_kernels.hpp).  The colour rule is host_models.yuv_planes_to_rgb8 (common.hpp: fh_yuv_to_rgb_deep), in int32.
//   Template parameters are what changes the code: BITS (8 | 16, the width of a stored sample), HS and VS (chroma geometry) and
//   CENTRE.  The bit shift, the depth mask, the byte step between chroma samples (planar or semi-planar) and every offset and
//   pitch are uniform kernel arguments: NV12, NV21, P010 and yuv420p10le run the same instantiation.
//   Luma: a lane takes 4 consecutive samples of the span - one dword at 8 bits, two at 16 - by imgx_load4: the aligned dword
//   where the bytes wanted lie in one, two aligned dwords funnel-shifted where they straddle, bytes where those dwords would
//   leave `data` (its first and last bytes).  The alignment is decided per load from the address, so a pitch that is no multiple
//   of 4 - every row at another phase - is the ordinary path.  A span begins on a multiple of HS (first_col) and every chunk on a
//   multiple of 4 after it, so the four samples share 4 / HS chroma samples in every chunk; the last group of an odd-width row is
//   short and its last chroma sample serves one column.
//   Chroma, VS = 2 (4:2:0): a chroma row serves two luma rows and stays in LDS across them, as in ImgySrc - one slot, or two
//   under CENTRE (libjpeg's h2v2 triangle rule needs the near and the far row), chosen by the chroma row's parity and tagged with
//   the row held, so a far row becomes near without a second load.  An entry is U | V << 8 in 16 bits at 8-bit samples (two per
//   dword) and U | V << 16 in a dword at 16-bit samples, shifted and masked when it is loaded; replicated edge columns are entries
//   like any other (one dword of lead in front, the right neighbour behind, clamped at load time).
//   Chroma, VS = 1, HS = 2 (4:2:2): a chroma row serves one luma row, so holding it buys nothing: a lane loads the two samples
//   of its own group straight to registers.  Under CENTRE (h2v1: out[2 i] = (3 c[i] + c[i - 1] + 1) >> 2, out[2 i + 1] =
//   (3 c[i] + c[i + 1] + 2) >> 2) the left neighbour is the previous lane's second sample and the right neighbour the next lane's
//   first: they come through the wave's lane crossbar (DPP wave_shr:1 / wave_shl:1, one v_mov_b32_dpp each - the listing shows no
//   ds_bpermute), and only lane 0, lane 63 and the lane of the span's last group load a clamped neighbour themselves.  No LDS slot,
//   no barrier in front of the luma load.  The exchange needs every lane, so the group loop has a wave-uniform trip count and
//   idle lanes are predicated, not branched away.
//   4:4:4: U and V are loaded like luma, four samples per lane; no chroma state at all, and one chroma rule.
// LDS per wave: stage_px dwords of RGB, then the slots of VS = 2.  At 8 bits that is ImgySrc's budget (2048 pixels: 8 KiB + 2 x
//   about 2 KiB, 48.2 KiB per workgroup).  At 16 bits an entry is a dword, two per group: a 2048-pixel slice would need 4 x (8 +
//   2 x 4.1) = 64.8 KiB, over the 64 KiB of a workgroup, so the 16-bit stage cap is kImgxStage16 = 1024: 4 x (4 + 2 x 2.02) =
//   32.2 KiB.  Wider spans are walked in chunks by imgv_row_sums as before.  Staging stores are one 16-byte write per lane, slot
//   reads 2 - 4 consecutive dwords per lane, unit stride across lanes: no conflicts.  Only wave-level barriers.
// Expected limiter: not the HBM read (1.5 - 6 bytes per pixel; ImgySrc measured 0.06 - 0.13 of the streaming rate at 1080p ->
//   512 px) but the chain of dependent latencies per source row; 4:2:2 and 4:4:4 have no chroma fill and barrier in that chain,
//   4:2:0 at 16 bits has twice the luma and chroma dwords of ImgySrc in it.  Measured (DESIGN.md section 6,
//   tools/probes/driveyuvbench.py --format): 250 frames of 1080p -> 512 px take 1.33 / 1.60 ms as P010 ("nearest" / "centre") and
//   1.77 / 2.16 ms as yuv422p10le, against 1.14 / 1.35 ms for ImgySrc on yuv420p: slower with every load a row adds, none near HBM.
// Exact integer arithmetic: matrix instructions have no place here.
#pragma once
#include "imgv_kernels.hpp"

constexpr int kImgxStage8 = 2048;   // packed pixels of a wave's RGB slice at 8-bit samples, at most (a multiple of 4)
constexpr int kImgxStage16 = 1024;  // at 16-bit samples (the arithmetic is above)
constexpr int kDppWaveShl1 = 0x130, kDppWaveShr1 = 0x138;  // lane i reads lane i + 1 | i - 1 of the WAVE; the end lane reads 0

struct ImgxArgs {
  ImgvArgs v;                     // frames: the block's first frame; out, sizes, scale, stage_px, rects as there; bytes, channels, rgba_mode, bkg are not read
  FhYuvInv k;                     // the matrix's row of kFhYuvInverse
  const unsigned char* data;      // the caller's buffer and its length: the bounds of the dword loads
  unsigned long long data_bytes;
  long long frame_stride, y_off, u_off, v_off;  // bytes
  int y_pitch, c_pitch, c_step;   // bytes; c_step between neighbouring samples of one chroma plane
  int shift, mask, s;             // sample = (word >> shift) & mask; s = depth - 8
  int cw, ch;                     // chroma plane sides: ceil(src_w / HS), ceil(src_h / VS)
  int chroma_dw;                  // dwords of one chroma slot (a multiple of 4; VS = 2 only)
};

// up to 4 bytes at `at`, of which the first `valid` are wanted and lie in the buffer (the others are whatever lies there, or 0)
template <bool STREAM>
__device__ __forceinline__ unsigned imgx_load4(uintptr_t at, int valid, uintptr_t safe_lo, uintptr_t safe_hi) {
  const uintptr_t al = at & ~(uintptr_t)3;
  const unsigned sh = 8 * (unsigned)(at & 3);
  const unsigned* q = reinterpret_cast<const unsigned*>(al);
  if (al >= safe_lo && al + 4 <= safe_hi) {
    const unsigned lo = STREAM ? __builtin_nontemporal_load(q) : q[0];
    if (sh + 8 * (unsigned)valid <= 32u) return lo >> sh;
    if (al + 8 <= safe_hi) {
      const unsigned hi = STREAM ? __builtin_nontemporal_load(q + 1) : q[1];
      return (unsigned)((((unsigned long long)hi << 32) | lo) >> sh);
    }
  }
  const unsigned char* b = reinterpret_cast<const unsigned char*>(at);
  unsigned v = 0;
  for (int j = 0; j < valid; ++j) v |= (unsigned)b[j] << (8 * j);
  return v;
}

template <int CTRL>
__device__ __forceinline__ unsigned imgx_dpp(unsigned v) {
  return (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, 0xf, 0xf, true);
}

template <int BITS, int HS, int VS, bool CENTRE>
struct ImgxSrc {
  static_assert((BITS == 8 || BITS == 16) && ((HS == 2 && VS == 2) || (HS == 2 && VS == 1) || (HS == 1 && VS == 1 && !CENTRE)), "ImgxSrc");
  using Args = ImgxArgs;
  static constexpr int kBytes = BITS / 8;
  static constexpr int kSlots = VS == 2 ? (CENTRE ? 2 : 1) : 0;
  static constexpr int kEpd = BITS == 8 ? 2 : 1;    // entries of a slot per dword
  static constexpr int kGroupDw = 2 / kEpd;         // dwords of a group's two samples
  static constexpr int kLead = CENTRE ? kEpd : 0;   // entries (one dword) in front of the span's first chroma sample
  static constexpr int kExtraDw = CENTRE ? 2 : 0;   // that dword and the right neighbour's
  static constexpr int kEsh = BITS == 8 ? 8 : 16;   // V's place in an entry
  __device__ static const ImgvArgs& common(const Args& a) { return a.v; }
  __device__ static int slice(const Args& a) { return a.v.stage_px + kSlots * a.chroma_dw; }
  __device__ static int first_col(int c) { return c & ~(HS - 1); }

  const unsigned char *luma, *cu, *cv;  // the frame's planes
  const unsigned char* clo;             // semi-planar: the first byte of the interleaved plane
  int w, cw, ch, y_pitch, c_pitch, c_step;
  bool semi, swapped;                   // semi-planar; and V in front of U there
  int shift, mask, s;
  uintptr_t safe_lo, safe_hi;  // the aligned part of the buffer
  unsigned* slots;             // kSlots x chroma_dw dwords
  int chroma_dw;
  int held0, held1, held_col;  // the chroma row in each slot, and the luma column their entries begin at (-1: nothing)
  FhYuvInv k;

  __device__ ImgxSrc(const Args& a, int fr, const ImgfPlan&, unsigned* own)
      : w(a.v.src_w), cw(a.cw), ch(a.ch), y_pitch(a.y_pitch), c_pitch(a.c_pitch), c_step(a.c_step), shift(BITS == 8 ? 0 : a.shift),
        mask(BITS == 8 ? 255 : a.mask), s(BITS == 8 ? 0 : a.s), slots(own), chroma_dw(a.chroma_dw), held0(-1), held1(-1), held_col(-1), k(a.k) {
    const unsigned char* frame = (const unsigned char*)a.v.frames + (long long)fr * a.frame_stride;
    luma = frame + a.y_off, cu = frame + a.u_off, cv = frame + a.v_off;
    semi = c_step == 2 * kBytes, swapped = a.v_off < a.u_off, clo = swapped ? cv : cu;
    safe_lo = ((uintptr_t)a.data + 3) & ~(uintptr_t)3, safe_hi = ((uintptr_t)a.data + a.data_bytes) & ~(uintptr_t)3;
  }

  // one stored sample (1 or 2 bytes, inside the frame) as its value
  __device__ __forceinline__ unsigned word(const unsigned char* p) const {
    if (BITS == 8) return p[0];
    const unsigned x = ((uintptr_t)p & 1) == 0 ? *reinterpret_cast<const unsigned short*>(p) : ((unsigned)p[0] | ((unsigned)p[1] << 8));
    return (x >> shift) & (unsigned)mask;
  }
  // chroma sample c (clamped to the plane) of chroma row r as an entry
  __device__ __forceinline__ unsigned entry(int r, int c) const {
    const size_t at = (size_t)r * c_pitch + (size_t)min(max(c, 0), cw - 1) * c_step;
    return word(cu + at) | (word(cv + at) << kEsh);
  }

  // N consecutive stored words at p, the first `valid` of them inside the plane row -> their values (the others: anything)
  template <int N, bool STREAM>
  __device__ __forceinline__ void words(const unsigned char* p, int valid, unsigned out[N]) const {
    constexpr int kDw = (N * kBytes + 3) / 4;
    unsigned d[kDw];
#pragma unroll
    for (int j = 0; j < kDw; ++j) {
      const int left = valid * kBytes - 4 * j;
      d[j] = left > 0 ? imgx_load4<STREAM>((uintptr_t)p + 4 * j, min(left, 4), safe_lo, safe_hi) : 0u;
    }
#pragma unroll
    for (int i = 0; i < N; ++i) {
      if (BITS == 8)
        out[i] = (d[i >> 2] >> (8 * (i & 3))) & 255u;
      else
        out[i] = ((d[i >> 1] >> (16 * (i & 1))) >> shift) & (unsigned)mask;
    }
  }

  // chroma samples c0 ... c0 + N - 1 of chroma row r, the first `valid` inside the plane: planar, or de-interleaved
  template <int N>
  __device__ __forceinline__ void chroma(int r, int c0, int valid, unsigned u[N], unsigned v[N]) const {
    const size_t at = (size_t)r * c_pitch + (size_t)c0 * c_step;
    if (semi) {
      unsigned uv[2 * N];
      words<2 * N, false>(clo + at, 2 * valid, uv);
#pragma unroll
      for (int i = 0; i < N; ++i) u[i] = uv[2 * i + (swapped ? 1 : 0)], v[i] = uv[2 * i + (swapped ? 0 : 1)];
    } else {
      words<N, false>(cu + at, valid, u);
      words<N, false>(cv + at, valid, v);
    }
  }

  // dword q < dwords of `slot`: entries kEpd q (+ 1), the chroma samples col_first + kEpd q (+ 1) of chroma row r, clamped
  __device__ __forceinline__ void fill(int lane, int slot, int r, int col_first, int dwords) {
    unsigned* dst = slots + slot * chroma_dw;
    for (int q = lane; q < dwords; q += kImgvCols) {
      const int c = col_first + kEpd * q;
      unsigned e;
      if (kEpd == 1) {
        e = entry(r, c);
      } else if (c >= 0 && c + 1 < cw) {
        unsigned u[2], v[2];
        chroma<2>(r, c, 2, u, v);
        e = u[0] | (v[0] << 8) | (u[1] << 16) | (v[1] << 24);
      } else {
        e = entry(r, c) | (entry(r, c + 1) << 16);
      }
      dst[q] = e;
    }
  }

  __device__ __forceinline__ unsigned rgb(unsigned Y, int U, int V) const { return fh_yuv_to_rgb_deep<BITS>(k, s, (int)Y, U, V); }

  __device__ __forceinline__ void stage(unsigned* px, int lane, int row, int col0, int n) {
    const int groups = (n + 3) >> 2;
    const int r = VS == 2 ? row >> 1 : row;
    int near_slot = 0, far_slot = 0;
    if (VS == 2) {
      if (col0 != held_col) held0 = held1 = -1, held_col = col0;
      near_slot = CENTRE ? (r & 1) : 0;
      const int far = !CENTRE ? r : (row & 1) ? min(r + 1, ch - 1) : max(r - 1, 0);
      far_slot = CENTRE ? (far & 1) : 0;
      const int dwords = groups * kGroupDw + kExtraDw, col_first = (col0 >> 1) - kLead;
      bool loaded = false;
      if ((near_slot ? held1 : held0) != r) {
        fill(lane, near_slot, r, col_first, dwords);
        (near_slot ? held1 : held0) = r, loaded = true;
      }
      if (CENTRE && (far_slot ? held1 : held0) != far) {
        fill(lane, far_slot, far, col_first, dwords);
        (far_slot ? held1 : held0) = far, loaded = true;
      }
      if (loaded) {
        __builtin_amdgcn_wave_barrier();
        __threadfence_block();
      }
    }
    const unsigned char* yrow = luma + (size_t)row * y_pitch + (size_t)col0 * kBytes;
    const unsigned *cn = slots + near_slot * chroma_dw, *cf = slots + far_slot * chroma_dw;
    constexpr unsigned m = (1u << kEsh) - 1u;  // an entry's U
    for (int g0 = 0; g0 < groups; g0 += kImgvCols) {  // the same trip count in every lane: the 4:2:2 exchange reads its neighbours
      const int g = g0 + lane;
      const bool live = g < groups;
      const int left = n - 4 * g;  // luma samples of the group that exist (live: at least 1)
      unsigned Y[4] = {0u, 0u, 0u, 0u};
      if (live) words<4, true>(yrow + (size_t)4 * g * kBytes, min(4, left), Y);
      int u[4], v[4];
      if (HS == 1) {
        unsigned cu4[4] = {0u, 0u, 0u, 0u}, cv4[4] = {0u, 0u, 0u, 0u};
        if (live) chroma<4>(r, col0 + 4 * g, min(4, left), cu4, cv4);
#pragma unroll
        for (int i = 0; i < 4; ++i) u[i] = (int)cu4[i], v[i] = (int)cv4[i];
      } else if (VS == 2) {
        if (!live) continue;  // nothing is exchanged: an idle lane may leave
        if (!CENTRE) {
          unsigned ea, eb;
          if (kEpd == 2) {
            const unsigned e = cn[g];
            ea = e & 0xffffu, eb = e >> 16;
          } else {
            ea = cn[2 * g], eb = cn[2 * g + 1];
          }
          u[0] = u[1] = (int)(ea & m), v[0] = v[1] = (int)(ea >> kEsh);
          u[2] = u[3] = (int)(eb & m), v[2] = v[3] = (int)(eb >> kEsh);
        } else {
          // the left neighbour, the group's two samples, the right neighbour, of the near and the far row; t = 3 near + far
          unsigned nl, na, nb, nr, fl, fa, fb, fr;
          if (kEpd == 2) {
            const unsigned n0 = cn[g], n1 = cn[g + 1], n2 = cn[g + 2], f0 = cf[g], f1 = cf[g + 1], f2 = cf[g + 2];
            nl = n0 >> 16, na = n1 & 0xffffu, nb = n1 >> 16, nr = n2 & 0xffffu;
            fl = f0 >> 16, fa = f1 & 0xffffu, fb = f1 >> 16, fr = f2 & 0xffffu;
          } else {
            nl = cn[2 * g], na = cn[2 * g + 1], nb = cn[2 * g + 2], nr = cn[2 * g + 3];
            fl = cf[2 * g], fa = cf[2 * g + 1], fb = cf[2 * g + 2], fr = cf[2 * g + 3];
          }
          auto tu = [](unsigned a, unsigned b) { return 3 * (int)(a & m) + (int)(b & m); };
          auto tv = [](unsigned a, unsigned b) { return 3 * (int)(a >> kEsh) + (int)(b >> kEsh); };
          const int ul = tu(nl, fl), ua = tu(na, fa), ub = tu(nb, fb), ur = tu(nr, fr);
          const int vl = tv(nl, fl), va = tv(na, fa), vb = tv(nb, fb), vr = tv(nr, fr);
          u[0] = (3 * ua + ul + 8) >> 4, u[1] = (3 * ua + ub + 7) >> 4, u[2] = (3 * ub + ua + 8) >> 4, u[3] = (3 * ub + ur + 7) >> 4;
          v[0] = (3 * va + vl + 8) >> 4, v[1] = (3 * va + vb + 7) >> 4, v[2] = (3 * vb + va + 8) >> 4, v[3] = (3 * vb + vr + 7) >> 4;
        }
      } else {  // 4:2:2: the group's two samples straight to registers, as entries
        const int c0 = (col0 >> 1) + 2 * g;
        unsigned ea = 0u, eb = 0u;
        if (live) {
          unsigned cu2[2], cv2[2];
          const int have = min(2, cw - c0);
          chroma<2>(r, c0, have, cu2, cv2);
          ea = cu2[0] | (cv2[0] << kEsh);
          eb = have == 2 ? (cu2[1] | (cv2[1] << kEsh)) : ea;  // past the plane: the last sample again
        }
        if (!CENTRE) {
          u[0] = u[1] = (int)(ea & m), v[0] = v[1] = (int)(ea >> kEsh);
          u[2] = u[3] = (int)(eb & m), v[2] = v[3] = (int)(eb >> kEsh);
        } else {
          unsigned el, er;  // the previous lane's second sample and the next lane's first
          if (kEpd == 2) {
            const unsigned e = ea | (eb << 16);
            el = imgx_dpp<kDppWaveShr1>(e) >> 16, er = imgx_dpp<kDppWaveShl1>(e) & 0xffffu;
          } else {
            el = imgx_dpp<kDppWaveShr1>(eb), er = imgx_dpp<kDppWaveShl1>(ea);
          }
          if (live && lane == 0) el = entry(r, c0 - 1);
          if (live && (lane == kImgvCols - 1 || g == groups - 1)) er = entry(r, c0 + 2);
          const int ul = (int)(el & m), ua = (int)(ea & m), ub = (int)(eb & m), ur = (int)(er & m);
          const int vl = (int)(el >> kEsh), va = (int)(ea >> kEsh), vb = (int)(eb >> kEsh), vr = (int)(er >> kEsh);
          u[0] = (3 * ua + ul + 1) >> 2, u[1] = (3 * ua + ub + 2) >> 2, u[2] = (3 * ub + ua + 1) >> 2, u[3] = (3 * ub + ur + 2) >> 2;
          v[0] = (3 * va + vl + 1) >> 2, v[1] = (3 * va + vb + 2) >> 2, v[2] = (3 * vb + va + 1) >> 2, v[3] = (3 * vb + vr + 2) >> 2;
        }
      }
      if (live) {
        uint4 o;
        o.x = rgb(Y[0], u[0], v[0]), o.y = rgb(Y[1], u[1], v[1]), o.z = rgb(Y[2], u[2], v[2]), o.w = rgb(Y[3], u[3], v[3]);
        *reinterpret_cast<uint4*>(px + 4 * g) = o;  // the slice is 16-byte aligned and a multiple of 4 pixels long
      }
    }
  }
};
