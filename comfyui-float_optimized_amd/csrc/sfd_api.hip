// C-ABI entry points of the S3FD face detector (include/float_hip.h, section "face detector"): forward, score / box decoding
// and NMS on the detector's view of the portrait, once per clip.  host_models.sfd_* is the definition.
#include <math.h>

#include "sfd_kernels.hpp"

namespace {

struct SConv {
  void* W = nullptr;      // [k*k][cout][cin] T::elem, cout padded to the kernel's tile
  float* bias = nullptr;  // [cout] (zeros in the padding)
  int cin = 0, cout = 0, k = 0, stride = 1, pad = 0;
};

// the trunk behind conv1_1: every conv + ReLU; pool = max_pool2d(2, 2) behind it; level = the detection level whose feature map
// the conv's (un-pooled) output is, or -1
struct TrunkDef {
  const char* name;
  int cin, cout, k, stride, pad, pool, level;
};
const TrunkDef kTrunk[] = {
    {"conv1_2", 64, 64, 3, 1, 1, 1, -1},    {"conv2_1", 64, 128, 3, 1, 1, 0, -1},   {"conv2_2", 128, 128, 3, 1, 1, 1, -1},
    {"conv3_1", 128, 256, 3, 1, 1, 0, -1},  {"conv3_2", 256, 256, 3, 1, 1, 0, -1},  {"conv3_3", 256, 256, 3, 1, 1, 1, 0},
    {"conv4_1", 256, 512, 3, 1, 1, 0, -1},  {"conv4_2", 512, 512, 3, 1, 1, 0, -1},  {"conv4_3", 512, 512, 3, 1, 1, 1, 1},
    {"conv5_1", 512, 512, 3, 1, 1, 0, -1},  {"conv5_2", 512, 512, 3, 1, 1, 0, -1},  {"conv5_3", 512, 512, 3, 1, 1, 1, 2},
    {"fc6", 512, 1024, 3, 1, 3, 0, -1},     {"fc7", 1024, 1024, 1, 1, 0, 0, 3},     {"conv6_1", 1024, 256, 1, 1, 0, 0, -1},
    {"conv6_2", 256, 512, 3, 2, 1, 0, 4},   {"conv7_1", 512, 128, 1, 1, 0, 0, -1},  {"conv7_2", 128, 256, 3, 2, 1, 0, 5},
};
constexpr int kNTrunk = (int)(sizeof(kTrunk) / sizeof(kTrunk[0]));
const char* const kHeadName[kSfdLevels] = {"conv3_3_norm", "conv4_3_norm", "conv5_3_norm", "fc7", "conv6_2", "conv7_2"};
const int kHeadConf[kSfdLevels] = {4, 2, 2, 2, 2, 2};
constexpr int kSfdMinSide = 16, kSfdMaxSide = 4096, kSfdMaxCand = 2048;

// Geometry of an H x W view: the six map sizes and, for sizing the workspace, the largest activation / L2Norm map (elements)
// and head map (pixels).  Every size is non-decreasing in H and in W, so the sizes of max_h x max_w bound every smaller view.
struct SfdPlan {
  SfdGeom g;
  size_t max_act = 0, max_norm = 0, max_head = 0;
};
SfdPlan sfd_plan(int H, int W) {
  SfdPlan p;
  int h = H, w = W, pos = 0;
  p.max_act = (size_t)h * w * 64;
  for (int i = 0; i < kNTrunk; ++i) {
    const TrunkDef& L = kTrunk[i];
    h = (h + 2 * L.pad - L.k) / L.stride + 1;
    w = (w + 2 * L.pad - L.k) / L.stride + 1;
    p.max_act = std::max(p.max_act, (size_t)h * w * L.cout);
    if (L.level >= 0) {
      p.g.h[L.level] = h;
      p.g.w[L.level] = w;
      p.g.pos0[L.level] = pos;
      pos += h * w;
      if (L.level < 3) p.max_norm = std::max(p.max_norm, (size_t)h * w * L.cout);
      p.max_head = std::max(p.max_head, (size_t)h * w);
    }
    if (L.pool) h /= 2, w /= 2;
  }
  p.g.pos0[kSfdLevels] = pos;
  return p;
}

}  // namespace

struct float_sfd {
  float_sfd_cfg_t cfg;
  DevicePool pool;
  float *w0 = nullptr, *b0 = nullptr;  // conv1_1: [ky][kx][c_bgr][64], [64]
  SConv trunk[kNTrunk];
  SConv head[kSfdLevels];
  float* normw[3] = {nullptr, nullptr, nullptr};
  void *bufA = nullptr, *bufB = nullptr, *bufN = nullptr;  // T::elem: ping-pong activations, the L2-normalised map
  float *headraw = nullptr, *maps = nullptr, *dense = nullptr;
  int last_P = 0;  // positions of the last detect / post (float_sfd_dense)
  unsigned long long* sat = nullptr;
};

namespace {

// rows of `names` stacked along Cout, zero-padded to cout_pad; biases likewise
template <class T>
int pack_conv(float_sfd* h, const TensorTable& tt, const std::vector<std::string>& names, int cin, int k, int cout_pad, SConv* out) {
  typedef typename T::elem E;
  std::vector<E> hw((size_t)k * k * cout_pad * cin, T::host_from_float(0.f));
  std::vector<float> hb((size_t)cout_pad, 0.f);
  int row = 0;
  for (const std::string& nm : names) {
    const float_tensor_t* w = tt.find(nm + ".weight");
    const float_tensor_t* b = tt.find(nm + ".bias");
    if (!w || !b) {
      fh_set_error("missing checkpoint tensor '%s.weight' / '%s.bias'", nm.c_str(), nm.c_str());
      return FLOAT_E_MISSING;
    }
    FH_REQUIRE(w->ndim == 4 && w->shape[1] == cin && w->shape[2] == k && w->shape[3] == k && TensorTable::numel(b) == w->shape[0] &&
                   row + (int)w->shape[0] <= cout_pad,
               "'%s' has unexpected shapes (s3fd: (Cout, %d, %d, %d))", nm.c_str(), cin, k, k);
    const int co = (int)w->shape[0];
    for (int o = 0; o < co; ++o) {
      hb[row + o] = b->data[o];
      for (int i = 0; i < cin; ++i)
        for (int t = 0; t < k * k; ++t)
          hw[((size_t)t * cout_pad + row + o) * cin + i] = T::host_from_float(w->data[((size_t)o * cin + i) * k * k + t]);
    }
    row += co;
  }
  int rc;
  E* dW = nullptr;
  if ((rc = h->pool.alloc(&dW, hw.size(), false))) return rc;
  if ((rc = h->pool.alloc(&out->bias, hb.size(), false))) return rc;
  FH_CHECK_HIP(hipMemcpy(dW, hw.data(), hw.size() * sizeof(E), hipMemcpyHostToDevice));
  FH_CHECK_HIP(hipMemcpy(out->bias, hb.data(), hb.size() * sizeof(float), hipMemcpyHostToDevice));
  out->W = dW;
  out->cin = cin;
  out->cout = cout_pad;
  out->k = k;
  return FLOAT_OK;
}

template <class T>
int create_impl(float_sfd* h, const TensorTable& tt) {
  typedef typename T::elem E;
  int rc;
  {
    const float_tensor_t* w = tt.find("conv1_1.weight");
    const float_tensor_t* b = tt.find("conv1_1.bias");
    if (!w || !b) {
      fh_set_error("missing checkpoint tensor 'conv1_1.weight' / 'conv1_1.bias'");
      return FLOAT_E_MISSING;
    }
    FH_REQUIRE(w->ndim == 4 && w->shape[0] == 64 && w->shape[1] == 3 && w->shape[2] == 3 && w->shape[3] == 3 && TensorTable::numel(b) == 64,
               "conv1_1.weight must be (64,3,3,3)");
    std::vector<float> hw(27 * 64);
    for (int o = 0; o < 64; ++o)
      for (int c = 0; c < 3; ++c)
        for (int t = 0; t < 9; ++t) hw[(t * 3 + c) * 64 + o] = w->data[(o * 3 + c) * 9 + t];
    if ((rc = h->pool.alloc(&h->w0, hw.size(), false)) || (rc = h->pool.alloc(&h->b0, (size_t)64, false))) return rc;
    FH_CHECK_HIP(hipMemcpy(h->w0, hw.data(), hw.size() * sizeof(float), hipMemcpyHostToDevice));
    FH_CHECK_HIP(hipMemcpy(h->b0, b->data, 64 * sizeof(float), hipMemcpyHostToDevice));
  }
  for (int i = 0; i < kNTrunk; ++i) {
    const TrunkDef& L = kTrunk[i];
    if ((rc = pack_conv<T>(h, tt, {L.name}, L.cin, L.k, L.cout, &h->trunk[i]))) return rc;
    h->trunk[i].stride = L.stride;
    h->trunk[i].pad = L.pad;
    if (L.level < 0) continue;
    const std::string hn = kHeadName[L.level];
    if ((rc = pack_conv<T>(h, tt, {hn + "_mbox_conf", hn + "_mbox_loc"}, L.cout, 3, kSfdHeadC, &h->head[L.level]))) return rc;
    h->head[L.level].pad = 1;
    if (L.level < 3) {
      const float_tensor_t* nw = tt.find(hn + ".weight");
      if (!nw || TensorTable::numel(nw) != L.cout) {
        fh_set_error("missing or mis-shaped checkpoint tensor '%s.weight'", hn.c_str());
        return FLOAT_E_MISSING;
      }
      if ((rc = h->pool.alloc(&h->normw[L.level], (size_t)L.cout, false))) return rc;
      FH_CHECK_HIP(hipMemcpy(h->normw[L.level], nw->data, (size_t)L.cout * sizeof(float), hipMemcpyHostToDevice));
    }
  }
  const SfdPlan p = sfd_plan(h->cfg.max_h, h->cfg.max_w);
  auto alloc_e = [&](void** dst, size_t n) {
    E* b = nullptr;
    const int r = h->pool.alloc(&b, n, true);
    *dst = b;
    return r;
  };
  if ((rc = alloc_e(&h->bufA, p.max_act)) || (rc = alloc_e(&h->bufB, p.max_act)) || (rc = alloc_e(&h->bufN, p.max_norm))) return rc;
  const size_t P = (size_t)p.g.pos0[kSfdLevels];
  if ((rc = h->pool.alloc(&h->headraw, p.max_head * kSfdHeadC, true)) || (rc = h->pool.alloc(&h->maps, P * 6, true)) ||
      (rc = h->pool.alloc(&h->dense, P * 5, true)) || (rc = h->pool.alloc(&h->sat, 1, true)))
    return rc;
  (void)hipFuncSetAttribute(reinterpret_cast<const void*>(sfd_select_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, kSfdMaxCand * 32);
  (void)hipGetLastError();
  return FLOAT_OK;
}

template <class T>
int launch_conv(const SConv& L, const void* X, int Hi, int Wi, void* Y, float* Yf32, int relu, hipStream_t st, unsigned long long* sat) {
  SfdConvArgs g;
  memset(&g, 0, sizeof(g));
  g.X = X;
  g.W = L.W;
  g.Y = Y;
  g.Yf32 = Yf32;
  g.bias = L.bias;
  g.Hi = Hi;
  g.Wi = Wi;
  g.Cin = L.cin;
  g.Cout = L.cout;
  g.k = L.k;
  g.stride = L.stride;
  g.pad = L.pad;
  g.Ho = (Hi + 2 * L.pad - L.k) / L.stride + 1;
  g.Wo = (Wi + 2 * L.pad - L.k) / L.stride + 1;
  g.relu = relu;
  g.sat = sat;
  const int npix = g.Ho * g.Wo;
  if (npix <= 0) return FLOAT_OK;
  const int mb = (npix + 63) / 64;
  if (L.cout % 64 == 0) hipLaunchKernelGGL((sfd_conv_kernel<T, 4>), dim3(mb, L.cout / 64), dim3(256), 0, st, g);
  else hipLaunchKernelGGL((sfd_conv_kernel<T, 1>), dim3(mb, L.cout / 16), dim3(256), 0, st, g);
  FH_CHECK_HIP(hipGetLastError());
  return FLOAT_OK;
}

// the network on the view: the 12 maps (per level conf [2][n], loc [4][n], at float offset 6 * pos0[level]) into maps_out
template <class T>
int forward_impl(float_sfd* h, const unsigned char* rgb8, int H, int W, const SfdGeom& geo, float* maps_out, hipStream_t st) {
  typedef typename T::elem E;
  int rc;
  void *cur = h->bufA, *oth = h->bufB;
  int hh = H, ww = W;
  {
    const size_t tot = (size_t)H * W * 8;
    hipLaunchKernelGGL((sfd_first_kernel<T>), dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, st, rgb8, h->w0, h->b0,
                       reinterpret_cast<E*>(cur), H, W, h->sat);
  }
  for (int i = 0; i < kNTrunk; ++i) {
    const TrunkDef& L = kTrunk[i];
    if ((rc = launch_conv<T>(h->trunk[i], cur, hh, ww, oth, nullptr, 1, st, h->sat))) return rc;
    std::swap(cur, oth);
    hh = (hh + 2 * L.pad - L.k) / L.stride + 1;
    ww = (ww + 2 * L.pad - L.k) / L.stride + 1;
    const int npix = hh * ww;
    if (L.level >= 0 && npix > 0) {
      const void* feat = cur;
      if (L.level < 3) {
        hipLaunchKernelGGL((sfd_l2norm_kernel<T>), dim3((unsigned)((npix + 3) / 4)), dim3(256), 0, st, reinterpret_cast<const E*>(cur),
                           h->normw[L.level], reinterpret_cast<E*>(h->bufN), npix, L.cout, h->sat);
        feat = h->bufN;
      }
      if ((rc = launch_conv<T>(h->head[L.level], feat, hh, ww, nullptr, h->headraw, 0, st, h->sat))) return rc;
      float* conf = maps_out + (size_t)6 * geo.pos0[L.level];
      hipLaunchKernelGGL(sfd_maps_kernel, dim3((unsigned)((npix + 255) / 256)), dim3(256), 0, st, h->headraw, conf, conf + (size_t)2 * npix,
                         npix, kHeadConf[L.level]);
    }
    if (L.pool) {
      const size_t tot = (size_t)(hh / 2) * (ww / 2) * (L.cout / 8);
      if (tot)
        hipLaunchKernelGGL((sfd_pool_kernel<T>), dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, st, reinterpret_cast<const E*>(cur),
                           reinterpret_cast<E*>(oth), hh, ww, L.cout, h->sat);
      std::swap(cur, oth);
      hh /= 2;
      ww /= 2;
    }
  }
  FH_CHECK_HIP(hipGetLastError());
  return FLOAT_OK;
}

int forward(float_sfd* h, const void* rgb8, int H, int W, const SfdGeom& geo, float* maps_out, hipStream_t st) {
  const unsigned char* p = reinterpret_cast<const unsigned char*>(rgb8);
  if (h->cfg.dtype == FLOAT_DT_FP32) return forward_impl<FP32>(h, p, H, W, geo, maps_out, st);
  return h->cfg.dtype == FLOAT_DT_BF16 ? forward_impl<BF16>(h, p, H, W, geo, maps_out, st) : forward_impl<FP16>(h, p, H, W, geo, maps_out, st);
}

int post(float_sfd* h, const float* maps, const SfdGeom& geo, float score_thr, float iou_thr, float* boxes, int32_t* counts, hipStream_t st) {
  const int P = geo.pos0[kSfdLevels];
  hipLaunchKernelGGL(sfd_decode_kernel, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, st, maps, geo, h->dense);
  hipLaunchKernelGGL(sfd_select_kernel, dim3(1), dim3(256), (size_t)h->cfg.max_candidates * 32, st, h->dense, P, score_thr, iou_thr,
                     h->cfg.max_candidates, h->cfg.max_boxes, boxes, counts);
  FH_CHECK_HIP(hipGetLastError());
  h->last_P = P;
  return FLOAT_OK;
}

// the checks every entry point makes before any HIP call
int check_view(const char* fn, const float_sfd* h, int H, int W) {
  FH_REQUIRE(H >= kSfdMinSide && W >= kSfdMinSide && H <= kSfdMaxSide && W <= kSfdMaxSide,
             "%s: a %d x %d view, sides run from %d to %d", fn, H, W, kSfdMinSide, kSfdMaxSide);
  FH_REQUIRE(h != nullptr, "%s: null handle", fn);
  FH_REQUIRE(H <= h->cfg.max_h && W <= h->cfg.max_w, "%s: a %d x %d view is beyond the handle's max_h x max_w = %d x %d", fn, H, W,
             h->cfg.max_h, h->cfg.max_w);
  return FLOAT_OK;
}

}  // namespace

extern "C" {

int float_sfd_create(const float_sfd_cfg_t* cfg, const float_tensor_t* tensors, int32_t n_tensors, float_sfd_t** out) {
  FH_REQUIRE(cfg && tensors && out, "null argument to float_sfd_create");
  FH_REQUIRE(cfg->dtype == FLOAT_DT_BF16 || cfg->dtype == FLOAT_DT_FP16 || cfg->dtype == FLOAT_DT_FP32, "unknown dtype %d", cfg->dtype);
  FH_REQUIRE(cfg->max_h >= kSfdMinSide && cfg->max_h <= kSfdMaxSide && cfg->max_w >= kSfdMinSide && cfg->max_w <= kSfdMaxSide,
             "float_sfd_create: max_h x max_w = %d x %d, sides run from %d to %d", cfg->max_h, cfg->max_w, kSfdMinSide, kSfdMaxSide);
  FH_REQUIRE(cfg->max_candidates >= 1 && cfg->max_candidates <= kSfdMaxCand, "float_sfd_create: max_candidates %d outside 1 ... %d",
             cfg->max_candidates, kSfdMaxCand);
  FH_REQUIRE(cfg->max_boxes >= 1 && cfg->max_boxes <= cfg->max_candidates, "float_sfd_create: max_boxes %d outside 1 ... max_candidates",
             cfg->max_boxes);
  float_sfd* h = new float_sfd();
  h->cfg = *cfg;
  TensorTable tt(tensors, n_tensors);
  int rc = (cfg->dtype == FLOAT_DT_BF16) ? create_impl<BF16>(h, tt)
           : (cfg->dtype == FLOAT_DT_FP32) ? create_impl<FP32>(h, tt) : create_impl<FP16>(h, tt);
  if (rc) {
    float_sfd_destroy(h);
    return rc;
  }
  *out = h;
  return FLOAT_OK;
}

void float_sfd_destroy(float_sfd_t* h) {
  if (!h) return;
  h->pool.release();
  delete h;
}

int float_sfd_detect(float_sfd_t* h, const void* rgb8, int32_t H, int32_t W, float score_thr, float iou_thr, float* boxes, int32_t* counts,
                     void* stream) {
  int rc;
  if ((rc = check_view("float_sfd_detect", h, H, W))) return rc;
  FH_REQUIRE(rgb8 && boxes && counts, "float_sfd_detect: null argument");
  const SfdPlan p = sfd_plan(H, W);
  if ((rc = forward(h, rgb8, H, W, p.g, h->maps, (hipStream_t)stream))) return rc;
  return post(h, h->maps, p.g, score_thr, iou_thr, boxes, counts, (hipStream_t)stream);
}

int float_sfd_maps(float_sfd_t* h, const void* rgb8, int32_t H, int32_t W, float* maps12, void* stream) {
  int rc;
  if ((rc = check_view("float_sfd_maps", h, H, W))) return rc;
  FH_REQUIRE(rgb8 && maps12, "float_sfd_maps: null argument");
  return forward(h, rgb8, H, W, sfd_plan(H, W).g, maps12, (hipStream_t)stream);
}

int float_sfd_post(float_sfd_t* h, const float* maps12, int32_t H, int32_t W, float score_thr, float iou_thr, float* boxes, int32_t* counts,
                   void* stream) {
  int rc;
  if ((rc = check_view("float_sfd_post", h, H, W))) return rc;
  FH_REQUIRE(maps12 && boxes && counts, "float_sfd_post: null argument");
  return post(h, maps12, sfd_plan(H, W).g, score_thr, iou_thr, boxes, counts, (hipStream_t)stream);
}

int float_sfd_dense(float_sfd_t* h, float* scores_boxes, void* stream) {
  FH_REQUIRE(h && scores_boxes, "float_sfd_dense: null argument");
  FH_REQUIRE(h->last_P > 0, "float_sfd_dense: no float_sfd_detect / float_sfd_post call on this handle yet");
  return fh_copy_d2d(scores_boxes, h->dense, (size_t)h->last_P * 5 * sizeof(float), (hipStream_t)stream);
}

int float_sfd_saturation(float_sfd_t* h, uint64_t* total, int32_t reset, void* stream) {
  FH_REQUIRE(h && total, "null argument to float_sfd_saturation");
  FH_CHECK_HIP(hipStreamSynchronize((hipStream_t)stream));
  unsigned long long v = 0;
  FH_CHECK_HIP(hipMemcpy(&v, h->sat, sizeof(v), hipMemcpyDeviceToHost));
  *total = v;
  if (reset) {  // on the caller's stream: ordered against the launches that add to the counter there
    FH_CHECK_HIP(hipMemsetAsync(h->sat, 0, sizeof(v), (hipStream_t)stream));
    FH_CHECK_HIP(hipStreamSynchronize((hipStream_t)stream));
  }
  return FLOAT_OK;
}

}  // extern "C"
