// Source policy of float_img_front_frames_yuv (include/float_hip.h): the frame-stacked front end reading planar (I420) or
// semi-planar (NV12) 8-bit YUV 4:2:0.  The work split, the taps and the 64-bit totals in registers are imgv_frames_kernel's
// (imgv_kernels.hpp) - this file is only its staging stage: how a wave turns the span of one source row into packed RGB dwords
// in its LDS slice.  The colour rule is host_models.yuv420_to_rgb8 (common.hpp: kFhYuvInverse, fh_yuv_to_rgb), in int32.
//   Work: a lane takes 4 consecutive luma pixels of the span, which begins on an even source column (first_col), so the four
//   share exactly two chroma samples.  Y is one dword load where the address is 4-byte aligned, two aligned dwords funnel-shifted
//   where it is not (a row of width 134 changes alignment from row to row, and a frame pointer may be odd), and bytes where
//   those dwords would leave the block of frames (its first and last bytes).  The lane converts as the pixels arrive and stores
//   its four packed dwords with one 16-byte LDS write.
//   Chroma stays in LDS across luma rows.  A wave walks its rows top to bottom; when row >> 1 changes it loads the chroma span of
//   the new chroma row - a lane takes 2 samples: one dword (NV12: U V U V), or two 16-bit loads (I420; two bytes each where the
//   row starts on an odd address) - and keeps it as packed U | V << 8 in 16-bit entries, two per dword.  "centre" (libjpeg's
//   h2v2 triangle rule) needs the near and the far chroma row: two slots, chosen by the chroma row's parity, each tagged with
//   the row it holds, so a row that was far becomes near without a second load, and the replicated first and last rows and
//   columns are entries like any other (two entries of padding on the left, the right neighbour on the right, clamped when they
//   are loaded).  So a chroma byte is fetched once per band, not once per luma row, and a luma pixel costs 1.5 bytes of reads.
//   A span wider than the slice is walked in chunks (imgv_row_sums); every chunk begins on an even column (the slice's length is
//   a multiple of 4), so chroma phase carries over; the chroma slots then hold one chunk and are loaded per chunk and row.
// LDS per wave: stage_px dwords of RGB (at most kImgyStage = 2048 pixels, 8 KiB), then 1 or 2 chroma slots of chroma_dw =
//   stage_px / 4 + 4 dwords rounded up to a multiple of 4, so that every wave's slice begins on 16 bytes (about 2 KiB each): at
//   most 12.1 KiB per wave and 48.2 KiB per workgroup of the 64 KiB.  The staging
//   stores are unit stride (16 bytes per lane) and the chroma reads one to three consecutive dwords per lane, unit stride across
//   lanes: neither conflicts.  The tap reads are imgv_frames_kernel's, stride about P / Q dwords across lanes, left alone for
//   its reason.  Only wave-level barriers; nothing is shared between waves.
// Expected limiter: the HBM read of the windows at 1.5 bytes per pixel (against 3 for 8-bit RGB).  Measured (DESIGN.md section 6,
//   tools/probes/driveyuvbench.py): that is NOT the limiter at 1080p -> 512 px - 250 frames take 1.13 ms ("nearest") and 1.33 ms
//   ("centre") against 1.00 ms for 8-bit RGB, 0.06 and 0.13 of the streaming read.  Supposed, not measured: the chain of
//   dependent latencies per source row, which the chroma load and its barrier in front of the luma load lengthen.
// Exact integer arithmetic: matrix instructions have no place here.
#pragma once
#include "imgv_kernels.hpp"

constexpr int kImgyStage = 2048;  // packed pixels of a wave's RGB slice, at most (a multiple of 4)
enum { kImgyI420 = 0, kImgyNv12 = 1 };

struct ImgyArgs {
  ImgvArgs v;     // frames, out, bytes, sizes, scale, stage_px and rects as there; channels, rgba_mode and bkg are not read
  FhYuvInv k;     // the matrix's row of kFhYuvInverse
  int chroma_dw;  // dwords of one chroma slot (a multiple of 4)
};

// 4 bytes at `at`, of which the first `valid` lie in the block: one aligned dword, two funnel-shifted, or bytes
template <bool STREAM>
__device__ __forceinline__ unsigned imgy_load4(uintptr_t at, int valid, uintptr_t safe_lo, uintptr_t safe_hi) {
  const uintptr_t al = at & ~(uintptr_t)3;
  const unsigned* q = reinterpret_cast<const unsigned*>(al);
  if (al == at && al >= safe_lo && al + 4 <= safe_hi) return STREAM ? __builtin_nontemporal_load(q) : *q;
  if (al >= safe_lo && al + 8 <= safe_hi) {
    const unsigned lo = STREAM ? __builtin_nontemporal_load(q) : q[0], hi = STREAM ? __builtin_nontemporal_load(q + 1) : q[1];
    return (unsigned)((((unsigned long long)hi << 32) | lo) >> (8 * (unsigned)(at & 3)));
  }
  const unsigned char* b = reinterpret_cast<const unsigned char*>(at);
  unsigned v = 0;
  for (int j = 0; j < valid; ++j) v |= (unsigned)b[j] << (8 * j);
  return v;
}

// 2 bytes at p, both in the frame
__device__ __forceinline__ unsigned imgy_load2(const unsigned char* p) {
  if (((uintptr_t)p & 1) == 0) return *reinterpret_cast<const unsigned short*>(p);
  return (unsigned)p[0] | ((unsigned)p[1] << 8);
}

template <int LAYOUT, bool CENTRE>
struct ImgySrc {
  using Args = ImgyArgs;
  static constexpr int kSlots = CENTRE ? 2 : 1;
  // "centre" reads a neighbour on either side of a group's two samples.  Two different counts, equal only by coincidence:
  static constexpr int kLead = CENTRE ? 2 : 0;     // 16-bit entries (one dword) in front of the span's first chroma sample
  static constexpr int kExtraDw = CENTRE ? 2 : 0;  // dwords of a slot beyond one per group: that leading one and the right neighbour's
  __device__ static const ImgvArgs& common(const Args& a) { return a.v; }
  __device__ static int slice(const Args& a) { return a.v.stage_px + kSlots * a.chroma_dw; }
  __device__ static int first_col(int c) { return c & ~1; }

  const unsigned char *luma, *cu, *cv;  // the frame's Y plane; its U and V planes, or its UV plane twice
  int w, cw, ch;                        // luma width; chroma width and height
  uintptr_t safe_lo, safe_hi;           // the aligned part of the block's frames
  unsigned* slots;                      // kSlots x chroma_dw dwords
  int chroma_dw;
  int held0, held1, held_col;  // the chroma row in each slot, and the luma column their entries begin at (-1: nothing)
  FhYuvInv k;

  __device__ ImgySrc(const Args& a, int fr, const ImgfPlan&, unsigned* own)
      : w(a.v.src_w), cw(a.v.src_w >> 1), ch(a.v.src_h >> 1), slots(own), chroma_dw(a.chroma_dw), held0(-1), held1(-1), held_col(-1), k(a.k) {
    const size_t plane = (size_t)a.v.src_h * a.v.src_w;
    luma = (const unsigned char*)a.v.frames + (size_t)fr * (plane + plane / 2);
    cu = luma + plane;
    cv = LAYOUT == kImgyNv12 ? cu : cu + plane / 4;
    safe_lo = ((uintptr_t)a.v.frames + 3) & ~(uintptr_t)3, safe_hi = ((uintptr_t)a.v.frames + a.v.bytes) & ~(uintptr_t)3;
  }

  // chroma sample c of chroma row r as an entry
  __device__ __forceinline__ unsigned entry(int r, int c) const {
    if (LAYOUT == kImgyNv12) {
      const unsigned char* p = cu + (size_t)r * w + 2 * c;
      return (unsigned)p[0] | ((unsigned)p[1] << 8);
    }
    const size_t at = (size_t)r * cw + c;
    return (unsigned)cu[at] | ((unsigned)cv[at] << 8);
  }

  // entries 2 q, 2 q + 1 of `slot` for q < pairs: chroma samples col_first + 2 q (+ 1) of chroma row r, clamped to the plane
  __device__ __forceinline__ void fill(int lane, int slot, int r, int col_first, int pairs) {
    unsigned* dst = slots + slot * chroma_dw;
    for (int q = lane; q < pairs; q += kImgvCols) {
      const int c = col_first + 2 * q;
      unsigned e;
      if (c >= 0 && c + 1 < cw) {
        if (LAYOUT == kImgyNv12) {
          e = imgy_load4<false>((uintptr_t)(cu + (size_t)r * w + 2 * c), 4, safe_lo, safe_hi);
        } else {
          const size_t at = (size_t)r * cw + c;
          const unsigned u2 = imgy_load2(cu + at), v2 = imgy_load2(cv + at);
          e = (u2 & 255u) | ((v2 & 255u) << 8) | ((u2 >> 8) << 16) | ((v2 >> 8) << 24);
        }
      } else {
        e = entry(r, min(max(c, 0), cw - 1)) | (entry(r, min(max(c + 1, 0), cw - 1)) << 16);
      }
      dst[q] = e;
    }
  }

  __device__ __forceinline__ void stage(unsigned* px, int lane, int row, int col0, int n) {
    const int groups = (n + 3) >> 2, r = row >> 1;
    if (col0 != held_col) held0 = held1 = -1, held_col = col0;
    const int near_slot = CENTRE ? (r & 1) : 0;
    const int far = !CENTRE ? r : (row & 1) ? min(r + 1, ch - 1) : max(r - 1, 0), far_slot = CENTRE ? (far & 1) : 0;
    const int pairs = groups + kExtraDw, col_first = (col0 >> 1) - kLead;
    bool loaded = false;
    if ((near_slot ? held1 : held0) != r) {
      fill(lane, near_slot, r, col_first, pairs);
      (near_slot ? held1 : held0) = r, loaded = true;
    }
    if (CENTRE && (far_slot ? held1 : held0) != far) {
      fill(lane, far_slot, far, col_first, pairs);
      (far_slot ? held1 : held0) = far, loaded = true;
    }
    if (loaded) {
      __builtin_amdgcn_wave_barrier();
      __threadfence_block();
    }
    const unsigned char* yrow = luma + (size_t)row * w + col0;
    const unsigned *cn = slots + near_slot * chroma_dw, *cf = slots + far_slot * chroma_dw;
    for (int g = lane; g < groups; g += kImgvCols) {
      const unsigned yy = imgy_load4<true>((uintptr_t)(yrow + 4 * g), min(4, n - 4 * g), safe_lo, safe_hi);
      int u[4], v[4];
      if (!CENTRE) {
        const unsigned e = cn[g];
        u[0] = u[1] = (int)(e & 255u), v[0] = v[1] = (int)((e >> 8) & 255u);
        u[2] = u[3] = (int)((e >> 16) & 255u), v[2] = v[3] = (int)(e >> 24);
      } else {
        // entries 2 g + 1 ... 2 g + 4: the left neighbour, the group's two samples, the right neighbour; s = 3 near + far
        const unsigned n0 = cn[g], n1 = cn[g + 1], n2 = cn[g + 2], f0 = cf[g], f1 = cf[g + 1], f2 = cf[g + 2];
        auto s = [](unsigned a, unsigned b, int sh) { return 3 * (int)((a >> sh) & 255u) + (int)((b >> sh) & 255u); };
        const int ul = s(n0, f0, 16), ua = s(n1, f1, 0), ub = s(n1, f1, 16), ur = s(n2, f2, 0);
        const int vl = s(n0, f0, 24), va = s(n1, f1, 8), vb = s(n1, f1, 24), vr = s(n2, f2, 8);
        u[0] = (3 * ua + ul + 8) >> 4, u[1] = (3 * ua + ub + 7) >> 4, u[2] = (3 * ub + ua + 8) >> 4, u[3] = (3 * ub + ur + 7) >> 4;
        v[0] = (3 * va + vl + 8) >> 4, v[1] = (3 * va + vb + 7) >> 4, v[2] = (3 * vb + va + 8) >> 4, v[3] = (3 * vb + vr + 7) >> 4;
      }
      uint4 o;
      o.x = fh_yuv_to_rgb(k, (int)(yy & 255u), u[0], v[0]), o.y = fh_yuv_to_rgb(k, (int)((yy >> 8) & 255u), u[1], v[1]);
      o.z = fh_yuv_to_rgb(k, (int)((yy >> 16) & 255u), u[2], v[2]), o.w = fh_yuv_to_rgb(k, (int)(yy >> 24), u[3], v[3]);
      *reinterpret_cast<uint4*>(px + 4 * g) = o;  // the slice is 16-byte aligned and a multiple of 4 pixels long
    }
  }
};
