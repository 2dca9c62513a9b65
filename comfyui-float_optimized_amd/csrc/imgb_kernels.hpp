// Kernels of float_img_blend (include/float_hip.h): the face joined to the portrait by a Laplacian pyramid of their DIFFERENCE,
// bitwise host_models.paste_multiband_rgb8.  Integers throughout, no atomics; `levels` launches down, `levels` launches up, the
// frame on grid z.
//   D_0 = 16 (F - S) over the window, D_{l+1} = reduce(D_l), Lap_l = D_l - expand(D_{l+1}),
//   B_l = (M_l Lap_l + 128) >> 8, R_L = (M_L D_L + 128) >> 8, R_l = B_l + expand(R_{l+1}), out = clamp(S + ((R_0 + 8) >> 4)).
// Level l is h_l x w_l with n_{l+1} = (n_l + 1) / 2; every index is clamped to its level's own extent.
//
//   imgb_down_kernel   level l -> l + 1.  A workgroup of 256 lanes owns a tile of kImgbDownH x kImgbDownW = 16 x 32 cells of level
//                      l + 1 and stages the (2 * 16 + 3) x (2 * 32 + 3) = 35 x 67 cells of level l under it - the clamped halo
//                      included - in LDS as int16, one PLANE per channel (rows padded to 68), so that lane x of a wave reads column
//                      2 x + j: a stride of one dword, no bank is hit twice.  At l = 0 the tile is formed from the face's and the
//                      portrait's bytes as 16 (F - S); D_0 never exists in HBM.  A lane owns one column and two vertically
//                      neighbouring cells: it runs the five taps horizontally over the seven rows under them into registers (35 LDS
//                      reads for two results instead of 50), then vertically, rounds once and stores int16 x 3 to `work`.
//                      LDS 3 * 35 * 68 * 2 = 14280 B per workgroup: eleven workgroups fit the 160 KiB of a CU, the limit is the
//                      eight 256-lane workgroups (32 waves) a CU holds.
//   imgb_up_kernel     level l from D_l, D_{l+1}, R_{l+1}, M_l.  A workgroup owns a tile of kImgbUpH x kImgbUpW = 16 x 64 cells; a
//                      lane takes four neighbouring cells of one row.  The two coarse tiles under it, (16 / 2 + 2) x (64 / 2 + 2) =
//                      10 x 34 cells whatever the parity of the tile's origin, are staged once: D_{l+1} as int16, R_{l+1} as int32,
//                      channel planes of 11 x 36 (one spare row and two spare columns, read only with weight 0 or for cells outside
//                      the window).  At the top (l = levels - 1) R_{l+1} is formed while staging, (M_L D_L + 128) >> 8: R_L costs
//                      no launch and no memory.  A lane combines three coarse rows (weights 1 6 1 for an even row, 4 4 0 for an
//                      odd one) of four coarse columns into registers and reads its four cells' expand() off those - which columns
//                      and weights a cell takes depends only on the parity of the window's origin, the same for every lane of a
//                      launch.  LDS 3 * 11 * 36 * (2 + 4) = 7128 B per workgroup; eight workgroups per CU, as above.
//                      At l > 0 it stores R_l as int32 x 3.  At l = 0 its tiles cover the whole FRAME in frame coordinates (so a
//                      lane's four cells start at a multiple of four pixels = 12 bytes of the row): D_0 is formed from the bytes
//                      again, the window's cells get the clamped result, every other cell the portrait's bytes - no second launch
//                      for the copy.  FAST (src_w % 4 == 0, out 4-byte aligned): the portrait is read as three unaligned dwords and
//                      the result stored as three aligned dwords; otherwise bytes.  The bytes stored are the same.
// Widths.  |D_0| <= 16 * 255 = 4080, and reduce and expand are weighted means (weights 256 / 256 and 64 / 64, rounded to nearest),
// so |D_l| <= 4080 and |expand(D_l)| <= 4080 at every level: D fits int16, a horizontal 5-tap sum is at most 16 * 4080 and the full
// one 256 * 4080 < 2^21.  |Lap_l| <= 8160, M <= 256, so |B_l| <= 8160 and |R_l| <= 4080 + 8160 (levels - l) <= 69360 at eight
// levels: R does NOT fit int16 and is kept as int32; 64 |R| < 2^23.  Offsets of a cell inside a level are below 3 * 2^28 and are
// formed in size_t together with the frame's base.
#pragma once
#include "common.hpp"

constexpr int kImgbThreads = 256;
constexpr int kImgbMaxLevels = 8;
constexpr int kImgbDownH = 16, kImgbDownW = 32;                    // tile of level l + 1 per workgroup
constexpr int kImgbDownRows = 2 * kImgbDownH + 3, kImgbDownCols = 2 * kImgbDownW + 3, kImgbDownPitch = kImgbDownCols + 1;
constexpr int kImgbUpH = 16, kImgbUpW = 64;                        // tile of level l per workgroup: 256 lanes x 4 cells
constexpr int kImgbUpRows = kImgbUpH / 2 + 2, kImgbUpCols = kImgbUpW / 2 + 2;
constexpr int kImgbUpRowsPad = kImgbUpRows + 1, kImgbUpPitch = kImgbUpCols + 2;

struct ImgbDown {
  int in_h, in_w, out_h, out_w;  // extents of level l and l + 1
  int src_w, win_x, win_y;       // l == 0: the portrait's width and the window's origin in it
  size_t face_frame;             // l == 0: bytes of a face frame, 3 h_0 w_0
  size_t work_frame;             // bytes of `work` per frame
  size_t in_off, out_off;        // D_l (l > 0) and D_{l+1} inside a frame's work
};

struct ImgbUp {
  int dom_h, dom_w;    // what the tiles cover: l == 0: the portrait; else level l
  int win_x, win_y;    // l == 0: the window's origin in the portrait; else 0
  int h, w, ch, cw;    // extents of level l and l + 1
  size_t face_frame, work_frame, out_frame;
  size_t d_off, dc_off, rc_off, r_off;  // D_l, D_{l+1}, R_{l+1} (not TOP), R_l (l > 0) inside a frame's work
};

__device__ __forceinline__ int imgb_clamp(int v, int hi) { return min(max(v, 0), hi); }

__device__ __forceinline__ unsigned imgb_load_u32(const unsigned char* q) {  // any alignment
  unsigned v;
  __builtin_memcpy(&v, q, 4);
  return v;
}

template <bool L0>
__global__ __launch_bounds__(kImgbThreads) void imgb_down_kernel(const unsigned char* __restrict__ src, const unsigned char* __restrict__ face,
                                                                 unsigned char* __restrict__ work, const ImgbDown p) {
  __shared__ short sm[3][kImgbDownRows][kImgbDownPitch];
  const int tid = threadIdx.x;
  const int ox0 = blockIdx.x * kImgbDownW, oy0 = blockIdx.y * kImgbDownH;
  const int ix0 = 2 * ox0 - 2, iy0 = 2 * oy0 - 2;
  const size_t f = blockIdx.z;
  unsigned char* wf = work + f * p.work_frame;
  const unsigned char* ff = face + f * p.face_frame;
  const short* din = reinterpret_cast<const short*>(wf + p.in_off);
  // rows and columns of the tile that a cell of level l + 1 inside the extent reads
  const int rows = min(kImgbDownRows, 2 * (p.out_h - oy0) + 3), cols = min(kImgbDownCols, 2 * (p.out_w - ox0) + 3);
  for (int e = tid; e < rows * kImgbDownCols * 3; e += kImgbThreads) {
    const int r = e / (kImgbDownCols * 3), rem = e - r * (kImgbDownCols * 3), j = rem / 3, c = rem - 3 * j;
    if (j >= cols) continue;
    const int y = imgb_clamp(iy0 + r, p.in_h - 1), x = imgb_clamp(ix0 + j, p.in_w - 1);
    int v;
    if (L0) {
      const int fv = ff[((size_t)y * p.in_w + x) * 3 + c];
      const int sv = src[((size_t)(p.win_y + y) * p.src_w + p.win_x + x) * 3 + c];
      v = 16 * (fv - sv);
    } else {
      v = din[((size_t)y * p.in_w + x) * 3 + c];
    }
    sm[c][r][j] = (short)v;
  }
  __syncthreads();
  const int tx = tid & (kImgbDownW - 1), tq = tid / kImgbDownW;  // 32 columns x 8 pairs of rows
  const int ox = ox0 + tx, oy = oy0 + 2 * tq;
  if (ox >= p.out_w || oy >= p.out_h) return;
  short* dout = reinterpret_cast<short*>(wf + p.out_off);
  const bool two = oy + 1 < p.out_h;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    int hs[7];
#pragma unroll
    for (int i = 0; i < 7; ++i) {
      const short* s = &sm[c][4 * tq + i][2 * tx];
      hs[i] = (i < 5 || two) ? s[0] + 4 * s[1] + 6 * s[2] + 4 * s[3] + s[4] : 0;
    }
    dout[((size_t)oy * p.out_w + ox) * 3 + c] = (short)((hs[0] + 4 * hs[1] + 6 * hs[2] + 4 * hs[3] + hs[4] + 128) >> 8);
    if (two) dout[((size_t)(oy + 1) * p.out_w + ox) * 3 + c] = (short)((hs[2] + 4 * hs[3] + 6 * hs[4] + 4 * hs[5] + hs[6] + 128) >> 8);
  }
}

// expand() of a lane's four cells from the four column sums v[0 ... 3] (three coarse rows already combined): ODD is the parity
// of the first cell's window column.  Even first cell: columns c-1 c c+1 | c c+1 | c c+1 c+2 | c+1 c+2 sit at v[0 1 2 | 1 2 | 1 2 3
// | 2 3]; odd first cell: c c+1 | c c+1 c+2 | c+1 c+2 | c+1 c+2 c+3 at v[0 1 | 0 1 2 | 1 2 | 1 2 3].
template <bool ODD>
__device__ __forceinline__ void imgb_expand4(const int v[4], int e[4]) {
  if (!ODD) {
    e[0] = v[0] + 6 * v[1] + v[2], e[1] = 4 * v[1] + 4 * v[2], e[2] = v[1] + 6 * v[2] + v[3], e[3] = 4 * v[2] + 4 * v[3];
  } else {
    e[0] = 4 * v[0] + 4 * v[1], e[1] = v[0] + 6 * v[1] + v[2], e[2] = 4 * v[1] + 4 * v[2], e[3] = v[1] + 6 * v[2] + v[3];
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) e[k] = (e[k] + 32) >> 6;
}

template <bool L0, bool TOP, bool FAST, bool ODD>
__global__ __launch_bounds__(kImgbThreads) void imgb_up_kernel(const unsigned char* __restrict__ src, const unsigned char* __restrict__ face,
                                                               const short* __restrict__ m_l, const short* __restrict__ m_c,
                                                               unsigned char* __restrict__ work, unsigned char* __restrict__ out, const ImgbUp p) {
  __shared__ short smd[3][kImgbUpRowsPad][kImgbUpPitch];
  __shared__ int smr[3][kImgbUpRowsPad][kImgbUpPitch];
  const int tid = threadIdx.x;
  const int tx0 = blockIdx.x * kImgbUpW, ty0 = blockIdx.y * kImgbUpH;
  const size_t f = blockIdx.z;
  const int lx = tid & 15, ly = tid >> 4;
  const int x = tx0 + 4 * lx, y = ty0 + ly;  // the lane's first cell, in the domain's coordinates
  const int u0 = x - p.win_x, v = y - p.win_y;  // ... and in the window's
  const bool row_in = y < p.dom_h && v >= 0 && v < p.h;
  // the tile's part of the window: cells ua ... ub by va ... vb
  const int ua = max(tx0 - p.win_x, 0), ub = min(tx0 + kImgbUpW - 1 - p.win_x, p.w - 1);
  const int va = max(ty0 - p.win_y, 0), vb = min(ty0 + kImgbUpH - 1 - p.win_y, p.h - 1);
  const bool tile_in = ua <= ub && va <= vb;  // the same for every lane of the workgroup
  const int csx = ((ua + 1) >> 1) - 1, csy = ((va + 1) >> 1) - 1;  // the coarse cell staged at [0][0] (may be -1: clamped)

  unsigned char* wf = work + f * p.work_frame;
  if (tile_in) {
    const short* dc = reinterpret_cast<const short*>(wf + p.dc_off);
    const int* rc = reinterpret_cast<const int*>(wf + p.rc_off);
    for (int e = tid; e < kImgbUpRows * kImgbUpCols * 3; e += kImgbThreads) {
      const int r = e / (kImgbUpCols * 3), rem = e - r * (kImgbUpCols * 3), j = rem / 3, c = rem - 3 * j;
      const int cy = imgb_clamp(csy + r, p.ch - 1), cx = imgb_clamp(csx + j, p.cw - 1);
      const size_t at = (size_t)cy * p.cw + cx;
      const int dv = dc[at * 3 + c];
      smd[c][r][j] = (short)dv;
      smr[c][r][j] = TOP ? ((int)m_c[at] * dv + 128) >> 8 : rc[at * 3 + c];
    }
    if (tid < 3 * kImgbUpPitch) {  // the spare row: read with weight 0 only, kept defined
      const int c = tid / kImgbUpPitch, j = tid - c * kImgbUpPitch;
      smd[c][kImgbUpRows][j] = 0, smr[c][kImgbUpRows][j] = 0;
    }
    if (tid < 3 * kImgbUpRowsPad * 2) {  // the two spare columns
      const int c = tid / (kImgbUpRowsPad * 2), rem = tid - c * (kImgbUpRowsPad * 2), r = rem >> 1, j = kImgbUpCols + (rem & 1);
      smd[c][r][j] = 0, smr[c][r][j] = 0;
    }
    __syncthreads();
  }

  // the portrait's bytes under the lane's four cells (l == 0), little-endian in three words
  unsigned sw[3] = {0u, 0u, 0u};
  int ncell = 4;  // cells of the lane inside the domain
  const unsigned char* srow = nullptr;
  unsigned char* orow = nullptr;
  if (L0) {
    if (y >= p.dom_h || x >= p.dom_w) return;
    ncell = min(4, p.dom_w - x);
    const size_t at = ((size_t)y * p.dom_w + x) * 3;
    srow = src + at, orow = out + f * p.out_frame + at;
    if (FAST) {
      sw[0] = imgb_load_u32(srow), sw[1] = imgb_load_u32(srow + 4), sw[2] = imgb_load_u32(srow + 8);
    } else {
#pragma unroll
      for (int i = 0; i < 12; ++i)
        if (i < 3 * ncell) sw[i >> 2] |= (unsigned)srow[i] << (8 * (i & 3));
    }
  } else {
    if (!row_in || u0 >= p.w) return;
    ncell = min(4, p.w - u0);
  }

  if (tile_in && row_in && u0 + 3 >= 0 && u0 < p.w) {
    const int rb = ((v + 1) >> 1) - 1 - csy;                                   // first of the three staged rows
    const int wy0 = (v & 1) ? 4 : 1, wy1 = (v & 1) ? 4 : 6, wy2 = (v & 1) ? 0 : 1;  // rb + 2 <= kImgbUpRows: the spare row at most
    const int jb = ((u0 + 1) >> 1) - 1 - csx;                                  // first of the four staged columns
    const unsigned char* frow = face + f * p.face_frame + (size_t)v * p.w * 3;
    const short* drow = reinterpret_cast<const short*>(wf + p.d_off) + (size_t)v * p.w * 3;
    int* rrow = reinterpret_cast<int*>(wf + p.r_off) + (size_t)v * p.w * 3;
    int mk[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int u = u0 + k;
      mk[k] = (k < ncell && u >= 0 && u < p.w) ? (int)m_l[(size_t)v * p.w + u] : -1;  // -1: the cell is not the window's
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      int vd[4], vr[4], ed[4], er[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int j = imgb_clamp(jb + i, kImgbUpPitch - 1);  // clamped only for cells outside the window
        vd[i] = wy0 * smd[c][rb][j] + wy1 * smd[c][rb + 1][j] + wy2 * smd[c][rb + 2][j];
        vr[i] = wy0 * smr[c][rb][j] + wy1 * smr[c][rb + 1][j] + wy2 * smr[c][rb + 2][j];
      }
      imgb_expand4<ODD>(vd, ed);
      imgb_expand4<ODD>(vr, er);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if (mk[k] < 0) continue;
        const int u = u0 + k, b = 3 * k + c;  // byte b of the lane's twelve
        int d;
        const int s = (int)((sw[b >> 2] >> (8 * (b & 3))) & 255u);
        if (L0)
          d = 16 * ((int)frow[(size_t)u * 3 + c] - s);
        else
          d = drow[(size_t)u * 3 + c];
        const int r = ((mk[k] * (d - ed[k]) + 128) >> 8) + er[k];
        if (L0) {
          const unsigned o = (unsigned)min(max(s + ((r + 8) >> 4), 0), 255);
          sw[b >> 2] = (sw[b >> 2] & ~(255u << (8 * (b & 3)))) | (o << (8 * (b & 3)));
        } else {
          rrow[(size_t)u * 3 + c] = r;
        }
      }
    }
  }

  if (L0) {
    if (FAST) {  // src_w % 4 == 0 and out 4-byte aligned: 12 bytes at a multiple of 12 in a row of 3 src_w
      unsigned* o = reinterpret_cast<unsigned*>(orow);
      o[0] = sw[0], o[1] = sw[1], o[2] = sw[2];
    } else {
#pragma unroll
      for (int i = 0; i < 12; ++i)
        if (i < 3 * ncell) orow[i] = (unsigned char)(sw[i >> 2] >> (8 * (i & 3)));
    }
  }
}
