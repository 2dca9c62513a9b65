// Probe: what the HEAD of a launch costs in a chain of small dependent kernels (the FMT step chain's regime, as ahead_chain.hip:
// 192 workgroups, 32 KB of weights and 4 KB of activations per workgroup, the activations written by the previous stage) when
// the chain is a captured graph of 59 x 50 launches.  Three forms of the same stage:
//   A  every argument in ONE by-value struct (read by s_load from the kernarg segment) and the block decode of fmt_gemm_body
//      with run-time / and % (what the chain's GEMM does today): two dependent scalar-memory round trips and the integer
//      divisions stand in front of the first operand load
//   B  the hot arguments as 13 leading scalar dwords, which -mllvm -amdgpu-kernarg-preload-count=14 lets the command processor
//      place in SGPRs at dispatch; the rest in a trailing struct that is first used after the operand loads; decode as A
//   C  B with the decode by shifts and a multiply-high constant made on the host: no division in front of the operand loads
// All three compute the same numbers (checked).  us per stage = median over the replays of (replay time / stages).
//   hipcc --offload-arch=gfx950 -O3 -mllvm -amdgpu-kernarg-preload-count=14 launch_head.hip -o launch_head && ./launch_head
// The preload length of each form is in the listing (add --cuda-device-only -S): .amdhsa_user_sgpr_kernarg_preload_length.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <algorithm>
#include <chrono>
#include <vector>
#define CK(x) do{hipError_t e=(x); if(e!=hipSuccess){printf("%s: %s\n",#x,hipGetErrorString(e)); return 1;}}while(0)

typedef float f4 __attribute__((ext_vector_type(4)));
constexpr int NTHR = 256, WVEC = 32 * 1024 / 16;  // float4s of weights per workgroup

struct Tail {  // what an epilogue would read: first used after the operand loads
  float scale, bias;
  float* out;
  int nwg, pad[9];
};
struct ArgsA {
  const float* in;
  const f4* W;
  int nbn, mblk, ksplit;
  Tail t;
};

// the block decode of fmt_gemm_body (EPI_PARTIAL form): (column block, row block, K slice) of workgroup `id`
__device__ __forceinline__ void decode_div(int id, int nbn, int mblk, int ksplit, int& bx, int& by, int& ks) {
  const int nbx = nbn * ksplit;
  ks = 0;
  if ((nbx & 7) == 0) {
    const int slot = id >> 3;
    by = slot % mblk;
    bx = (slot / mblk) * 8 + (id & 7);
  } else {
    bx = id % nbx;
    by = id / nbx;
  }
  if ((nbx & 7) == 0 && (8 % ksplit) == 0) {
    const int P = 8 / ksplit, x = bx & 7;
    ks = x / P;
    bx = (bx >> 3) * P + (x % P);
  } else {
    ks = bx / nbn;
    bx = bx % nbn;
  }
}
// the same with host-made constants: n / d == (n * mul) >> sh for n < 2^28 (Granlund & Montgomery), P a power of two
__device__ __forceinline__ unsigned mdiv(unsigned n, unsigned mul, unsigned sh) { return (unsigned)(((unsigned long long)n * mul) >> sh); }
__device__ __forceinline__ void decode_mul(unsigned id, unsigned mblk, unsigned mul, unsigned sh, unsigned pshift, int& bx, int& by, int& ks) {
  const unsigned slot = id >> 3, q = mdiv(slot, mul, sh), x = id & 7u;
  by = (int)(slot - q * mblk);
  ks = (int)(x >> pshift);
  bx = (int)((q << pshift) + (x & ((1u << pshift) - 1u)));
}

// the stage's work behind the decode: weights of (bx, ks), activations of the workgroup rotated by 37 (another XCD's output)
#define STAGE_BODY                                                                                   \
  __shared__ float red[4];                                                                            \
  const int t = threadIdx.x;                                                                          \
  const int wb = (bx * ksplit_ + ks) * mblk_ + by; /* a bijection onto 0 .. nwg-1 */                   \
  const f4* w = W + (size_t)wb * WVEC;                                                            \
  f4 wv[WVEC / NTHR];                                                                             \
  _Pragma("unroll") for (int i = 0; i < WVEC / NTHR; ++i) wv[i] = __builtin_nontemporal_load(w + i * NTHR + t); \
  const int src = (wb + 37) % nwg_;                                                                   \
  float x[4];                                                                                         \
  _Pragma("unroll") for (int k = 0; k < 4; ++k) x[k] = in[(size_t)src * 1024 + k * 256 + t];          \
  float4 acc = make_float4(0, 0, 0, 0);                                                               \
  _Pragma("unroll") for (int i = 0; i < WVEC / NTHR; ++i) { acc.x += wv[i].x; acc.y += wv[i].y; acc.z += wv[i].z; acc.w += wv[i].w; } \
  float s = x[0] + x[1] + x[2] + x[3];                                                                \
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);                                         \
  if ((t & 63) == 0) red[t >> 6] = s;                                                                 \
  __syncthreads();                                                                                    \
  const float tot = (red[0] + red[1] + red[2] + red[3]) * (1.0f / 1024.f) + (acc.x + acc.y + acc.z + acc.w) * 1e-9f; \
  _Pragma("unroll") for (int k = 0; k < 4; ++k) tl.out[(size_t)wb * 1024 + k * 256 + t] = x[k] * tl.scale + tot * 0.5f + tl.bias;

__global__ __launch_bounds__(NTHR) void stage_a(ArgsA g) {
  int bx, by, ks;
  decode_div(blockIdx.x, g.nbn, g.mblk, g.ksplit, bx, by, ks);
  const float* in = g.in;
  const f4* W = g.W;
  const int ksplit_ = g.ksplit, mblk_ = g.mblk, nwg_ = g.t.nwg;
  const Tail& tl = g.t;
  STAGE_BODY
}
__global__ __launch_bounds__(NTHR) void stage_b(const float* in, const f4* W, int nbn, int mblk, int ksplit, int nwg, unsigned mul,
                                                unsigned sh, unsigned pshift, Tail tl) {
  int bx, by, ks;
  decode_div(blockIdx.x, nbn, mblk, ksplit, bx, by, ks);
  const int ksplit_ = ksplit, mblk_ = mblk, nwg_ = nwg;
  STAGE_BODY
}
__global__ __launch_bounds__(NTHR) void stage_c(const float* in, const f4* W, int nbn, int mblk, int ksplit, int nwg, unsigned mul,
                                                unsigned sh, unsigned pshift, Tail tl) {
  int bx, by, ks;
  decode_mul(blockIdx.x, (unsigned)mblk, mul, sh, pshift, bx, by, ks);
  const int ksplit_ = ksplit, mblk_ = mblk, nwg_ = nwg;
  STAGE_BODY
}

int main(int argc, char** argv) {
  // 192 workgroups = 16 column blocks x 3 row blocks x 4 K slices (fc2's launch)
  const int nbn = 16, mblk = 3, ksplit = 4, NWG = nbn * mblk * ksplit;
  const int STAGES = 59 * 50, REPLAYS = argc > 1 ? atoi(argv[1]) : 12;
  unsigned l = 0;
  while ((1u << l) < (unsigned)mblk) ++l;
  const unsigned sh = 28u + l, mul = (unsigned)((1ull << sh) / mblk + 1ull), pshift = 1;  // P = 8 / ksplit = 2
  float* buf[2];
  f4* W;
  const size_t wbytes = (size_t)NWG * WVEC * 16;  // 6 MB per stage; 8 rotating sets = 48 MB, beyond the 8 x 4 MB of L2
  CK(hipMalloc(&buf[0], (size_t)NWG * 4096));
  CK(hipMalloc(&buf[1], (size_t)NWG * 4096));
  CK(hipMalloc(&W, wbytes * 8));
  CK(hipMemset(W, 0, wbytes * 8));
  hipStream_t s;
  CK(hipStreamCreate(&s));
  auto Wof = [&](int i) { return W + (size_t)(i % 8) * NWG * WVEC; };
  double med[3];
  float check[3];
  for (int v = 0; v < 3; ++v) {
    hipGraph_t g;
    hipGraphExec_t ge;
    CK(hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal));
    for (int i = 0; i < STAGES; ++i) {
      Tail tl{};
      tl.scale = 0.5f, tl.bias = 1e-3f, tl.out = buf[(i + 1) & 1], tl.nwg = NWG;
      if (v == 0) {
        ArgsA a{buf[i & 1], Wof(i), nbn, mblk, ksplit, tl};
        hipLaunchKernelGGL(stage_a, dim3(NWG), dim3(NTHR), 0, s, a);
      } else {
        hipLaunchKernelGGL(v == 1 ? stage_b : stage_c, dim3(NWG), dim3(NTHR), 0, s, (const float*)buf[i & 1], (const f4*)Wof(i), nbn,
                           mblk, ksplit, NWG, mul, sh, pshift, tl);
      }
    }
    CK(hipStreamEndCapture(s, &g));
    CK(hipGraphInstantiate(&ge, g, nullptr, nullptr, 0));
    std::vector<double> us;
    for (int rep = 0; rep < REPLAYS + 2; ++rep) {
      CK(hipMemsetAsync(buf[0], 0, (size_t)NWG * 4096, s));
      CK(hipStreamSynchronize(s));
      const auto t0 = std::chrono::high_resolution_clock::now();
      CK(hipGraphLaunch(ge, s));
      CK(hipStreamSynchronize(s));
      const auto t1 = std::chrono::high_resolution_clock::now();
      if (rep >= 2) us.push_back(std::chrono::duration<double, std::micro>(t1 - t0).count() / STAGES);
    }
    std::sort(us.begin(), us.end());
    med[v] = us[us.size() / 2];
    CK(hipMemcpy(&check[v], buf[STAGES & 1] + 1234, 4, hipMemcpyDeviceToHost));
    printf("%c  %-52s median %.3f us/stage  (min %.3f, max %.3f, %d replays)  check %.9g\n", 'A' + v,
           v == 0 ? "by-value struct, decode with / and %" : (v == 1 ? "13 leading scalar dwords (preloaded), decode as A" : "B + decode by multiply-high, no division"),
           med[v], us.front(), us.back(), (int)us.size(), check[v]);
    CK(hipGraphExecDestroy(ge));
    CK(hipGraphDestroy(g));
  }
  printf("B - A %+.3f us/stage, C - B %+.3f us/stage; results %s\n", med[1] - med[0], med[2] - med[1],
         (check[0] == check[1] && check[1] == check[2]) ? "equal" : "DIFFER");
  return (check[0] == check[1] && check[1] == check[2]) ? 0 : 2;
}
