// Packed weights of the FMT's Linear layers: the device-side packing kernel, pack_linear_pool (named fp32 host tensors -> one
// FmtLin, several layers concatenated along N) and the concatenation of two packed layers.  Included by fmt_api.hip only,
// inside its anonymous namespace (the one translation unit that holds the FMT kernels' instantiations).
#pragma once
#include "fmt_gemm.hpp"

namespace {

typedef FmtLin Lin;

int round_up(int x, int m) { return (x + m - 1) / m * m; }

// f(T{}) with T the operand type of `dtype` (FLOAT_DT_BF16 / _FP16 / _FP32; the caller has checked that it is one of them)
template <class F>
auto fmt_by_dtype(int dtype, F&& f) {
  if (dtype == FLOAT_DT_BF16) return f(BF16{});
  if (dtype == FLOAT_DT_FP16) return f(FP16{});
  return f(FP32{});
}

// Weight packing ON THE DEVICE (round 6): the fp32 rows of a Linear cross PCIe once as they are and a kernel writes the
// fragment-major image - 8 consecutive k of a row = one pack (fmt_pack_off), converted with the conversion every activation
// store uses (round to nearest even, fp16 saturating at 65504).  On the host the same loop ran at ~5 ns per weight on ONE
// thread: 0.86 s for the FMT, 1.74 s for the speech-emotion model, 3.4 s per InferenceAgent.to_target(); now the time of the
// copies (tools/probes/retarget_time.py; INTEGRATION.md "Residency").  FLOAT_PACK_HOST=1 keeps the host loop (the A/B switch;
// the two images are equal bit for bit for finite weights - tests/test_variants_gpu.py).
template <class T>
__global__ __launch_bounds__(256) void fmt_pack_w_kernel(typename T::elem* __restrict__ out, const float* __restrict__ w, int N_each,
                                                         int K, int KB, int n0) {
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  const int gpr = KB * 4;  // packs per row
  const int n = (int)(idx / gpr), k0 = (int)(idx % gpr) * 8;
  if (n >= N_each) return;
  typename T::pack8 p;
#pragma unroll
  for (int i = 0; i < 8; ++i) T::set(p, i, k0 + i < K ? w[(size_t)n * K + k0 + i] : 0.f);
  T::store8(out + fmt_pack_off(n0 + n, k0, KB), p);
}

template <class T>
int pack_linear_pool(const FmtTune& tn, DevicePool* pool, const TensorTable& tt, const std::vector<std::string>& names, int N_each,
                     int K, Lin* out) {
  // Concatenate the named Linear layers along N (used to fuse every adaLN projection into one GEMM).
  typedef typename T::elem E;
  constexpr size_t esz = sizeof(E) / sizeof(u16);  // u16 slots per element (Lin::W is typed u16* for every operand type)
  const int Kp = round_up(K, 128);
  const int N = N_each * (int)names.size();
  const bool on_host = tn.pack_host;
  std::vector<E> hw;
  if (on_host) hw.assign((size_t)N * Kp, (E)0);
  std::vector<float> hb(N, 0.f);
  int rc;
  if ((rc = pool->alloc(&out->W, (size_t)N * Kp * esz, false))) return rc;
  if ((rc = pool->alloc(&out->b, hb.size(), false))) return rc;
  float* stage = nullptr;  // one Linear's fp32 rows on the device
  if (!on_host) FH_CHECK_HIP(hipMalloc(&stage, (size_t)N_each * K * sizeof(float)));
  struct Free {
    float* p;
    ~Free() {
      if (p) (void)hipFree(p);
    }
  } free_stage{stage};
  int n0 = 0;
  for (const std::string& nm : names) {
    const float_tensor_t* w = tt.find(nm + ".weight");
    const float_tensor_t* b = tt.find(nm + ".bias");
    if (!w || !b) {
      fh_set_error("missing checkpoint tensor '%s.weight/.bias'", nm.c_str());
      return FLOAT_E_MISSING;
    }
    if (w->ndim != 2 || w->shape[0] != N_each || w->shape[1] != K || TensorTable::numel(b) != N_each) {
      fh_set_error("tensor '%s.weight' has shape (%lld,%lld), expected (%d,%d)", nm.c_str(), (long long)w->shape[0],
                   (long long)(w->ndim > 1 ? w->shape[1] : 0), N_each, K);
      return FLOAT_E_INVALID;
    }
    if (on_host) {
      for (int n = 0; n < N_each; ++n) {
        const float* src = w->data + (size_t)n * K;
        for (int k = 0; k < K; ++k) hw[fmt_pack_off(n0 + n, k, Kp / 32)] = T::host_from_float(src[k]);
      }
    } else {
      // (null stream: the copy returns when the rows are on the device, the kernel runs before the next copy into `stage`)
      FH_CHECK_HIP(hipMemcpy(stage, w->data, (size_t)N_each * K * sizeof(float), hipMemcpyHostToDevice));
      const size_t packs = (size_t)N_each * (Kp / 8);
      hipLaunchKernelGGL((fmt_pack_w_kernel<T>), dim3((unsigned)((packs + 255) / 256)), dim3(256), 0, nullptr,
                         reinterpret_cast<E*>(out->W), stage, N_each, K, Kp / 32, n0);
      FH_CHECK_HIP(hipGetLastError());
    }
    for (int n = 0; n < N_each; ++n) hb[n0 + n] = b->data[n];
    n0 += N_each;
  }
  if (on_host) FH_CHECK_HIP(hipMemcpy(out->W, hw.data(), hw.size() * sizeof(E), hipMemcpyHostToDevice));
  FH_CHECK_HIP(hipMemcpy(out->b, hb.data(), hb.size() * sizeof(float), hipMemcpyHostToDevice));
  if (!on_host) FH_CHECK_HIP(hipDeviceSynchronize());  // the packed image is complete (and `stage` idle) when the call returns
  out->N = N;
  out->K = Kp;
  return FLOAT_OK;
}

// The rows of `tail` behind the rows of `head` (same K) as one packed layer in `pool`: the head's adaLN (2D outputs) rides at
// the end of the blocks' fused projection.  The two sources stay in the pool until it is released (small: ~100 MB).
template <class T>
int concat_linear_rows(DevicePool* pool, const Lin& head, const Lin& tail, Lin* out) {
  constexpr size_t esz = sizeof(typename T::elem) / sizeof(u16);
  Lin fused;
  fused.N = head.N + tail.N;
  fused.K = head.K;
  int rc;
  if ((rc = pool->alloc(&fused.W, (size_t)fused.N * fused.K * esz, false))) return rc;
  if ((rc = pool->alloc(&fused.b, (size_t)fused.N, false))) return rc;
  FH_CHECK_HIP(hipMemcpy(fused.W, head.W, (size_t)head.N * fused.K * esz * sizeof(u16), hipMemcpyDeviceToDevice));
  FH_CHECK_HIP(hipMemcpy(fused.W + (size_t)head.N * fused.K * esz, tail.W, (size_t)tail.N * fused.K * esz * sizeof(u16),
                         hipMemcpyDeviceToDevice));
  FH_CHECK_HIP(hipMemcpy(fused.b, head.b, (size_t)head.N * sizeof(float), hipMemcpyDeviceToDevice));
  FH_CHECK_HIP(hipMemcpy(fused.b + head.N, tail.b, (size_t)tail.N * sizeof(float), hipMemcpyDeviceToDevice));
  *out = fused;
  return FLOAT_OK;
}

}  // namespace
