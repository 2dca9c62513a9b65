// Stand-alone host program of tests/test_fmt_block_decode.py: the division-free block decode of the FMT's weight-streaming GEMM
// (csrc/fmt_decode.hpp) against the formula with / and % that fmt_gemm_body used before it - copied here as the DEFINITION of
// the map - for every workgroup id of every launch shape the launchers produce, and the map's bijection onto the tiles.
//   c++ -std=c++17 -O1 -fsanitize=address,undefined -I <csrc> fmt_block_decode_main.cpp -o decode_check && ./decode_check
#include <cstdio>
#include <vector>

#include "fmt_decode.hpp"

// the definition: 1-D grid of (column blocks) x (row blocks); row blocks of one column block on consecutive slots of one XCD
// when the pairs are a multiple of 8, and then K slice ks on the 8 / ksplit XCDs that own it when ksplit divides 8
static void decode_def(int id, int nbn, int mblk, int ksplit, bool partial, int& bx, int& by, int& ks) {
  ks = 0;
  const int nbx = partial ? nbn * ksplit : nbn;
  if ((nbx & 7) == 0) {
    const int slot = id >> 3;
    by = slot % mblk;
    bx = (slot / mblk) * 8 + (id & 7);
  } else {
    bx = id % nbx;
    by = id / nbx;
  }
  if (partial) {
    if ((nbx & 7) == 0 && (8 % ksplit) == 0) {
      const int P = 8 / ksplit, x = bx & 7;
      ks = x / P;
      bx = (bx >> 3) * P + (x % P);
    } else {
      ks = bx / nbn;
      bx = bx % nbn;
    }
  }
}

int main() {
  // column blocks N / BN: 1 .. 72 (every residue mod 8, twice over), then the chain's and the audio encoder's widths at 16-,
  // 32- and 64-column blocks (dim_h 256 .. 1024, mlp 4096, wav2vec2 768 / 3072) and a wide N at 16 columns per block
  std::vector<int> nbns;
  for (int n = 1; n <= 72; ++n) nbns.push_back(n);
  for (int n : {96, 128, 192, 256, 800}) nbns.push_back(n);
  // row blocks: 1 .. 12 (one clip: at most 15 row tiles in blocks of 1 .. 5), then stacked clips (row tiles / 3 per block)
  std::vector<int> mblks;
  for (int m = 1; m <= 12; ++m) mblks.push_back(m);
  for (int m : {15, 45}) mblks.push_back(m);
  long shapes = 0, ids = 0;
  for (int partial = 0; partial < 2; ++partial)
    for (int ksplit : {1, 2, 3, 4, 8}) {  // 3: a K split that does not divide 8 (the generic walk)
      if (!partial && ksplit != 1) continue;  // launch_gemm: only EPI_PARTIAL launches split K over workgroups
      for (int nbn : nbns)
        for (int mblk : mblks) {
          const GemmDecode d = fmt_make_decode(nbn, mblk, ksplit, partial != 0);
          const int grid = nbn * mblk * ksplit;
          std::vector<unsigned char> seen((size_t)grid, 0);
          for (int id = 0; id < grid; ++id) {
            int bx, by, ks;
            decode_def(id, nbn, mblk, ksplit, partial != 0, bx, by, ks);
            const GemmBlock b = fmt_block_decode(d, (unsigned)mblk, (unsigned)id, partial != 0);
            if (b.bx != bx || b.by != by || b.ks != ks) {
              std::printf("MISMATCH nbn=%d mblk=%d ksplit=%d partial=%d id=%d: (%d, %d, %d), definition (%d, %d, %d)\n", nbn, mblk,
                          ksplit, partial, id, b.bx, b.by, b.ks, bx, by, ks);
              return 1;
            }
            if (bx < 0 || bx >= nbn || by < 0 || by >= mblk || ks < 0 || ks >= ksplit) {
              std::printf("OUT OF RANGE nbn=%d mblk=%d ksplit=%d partial=%d id=%d: (%d, %d, %d)\n", nbn, mblk, ksplit, partial, id, bx,
                          by, ks);
              return 1;
            }
            unsigned char& s = seen[((size_t)ks * mblk + by) * nbn + bx];
            if (s) {
              std::printf("NOT A BIJECTION nbn=%d mblk=%d ksplit=%d partial=%d: tile (%d, %d, %d) twice, id=%d\n", nbn, mblk, ksplit,
                          partial, bx, by, ks, id);
              return 1;
            }
            s = 1;
          }
          ++shapes, ids += grid;
        }
    }
  // the divider itself at the edge of its range: every divisor up to 4096 against the last dividends below 2^28
  for (unsigned dv = 1; dv <= 4096; ++dv) {
    const FmtDiv f = fmt_make_div(dv);
    for (unsigned n : {0u, 1u, dv - 1u, dv, dv + 1u, kFmtDivMax - dv - 1u, kFmtDivMax - dv, kFmtDivMax - 2u, kFmtDivMax - 1u}) {
      if (n < kFmtDivMax && fmt_div(n, f) != n / dv) {
        std::printf("DIVIDER %u / %u: %u, expected %u\n", n, dv, fmt_div(n, f), n / dv);
        return 1;
      }
    }
  }
  std::printf("ok: %ld shapes, %ld workgroup ids\n", shapes, ids);
  return 0;
}
