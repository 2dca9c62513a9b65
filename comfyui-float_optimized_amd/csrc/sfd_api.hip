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
constexpr int kSfdMinSide = 16, kSfdMaxSide = 4096, kSfdMaxCand = 2048, kSfdMaxViews = 64;

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
  DevicePool pool;  // weights, the range counter
  DevicePool ws;    // the workspace below: sized by create for one view of max_h x max_w, grown by float_sfd_reserve_batch only
  size_t cap_act = 0, cap_norm = 0, cap_head = 0, cap_pos = 0;  // elements of bufA / bufB, bufN; pixels of headraw; positions of maps / dense
  int res_n = 0, res_h = 0, res_w = 0;                          // float_sfd_reserve_batch: views and view size the batched calls accept
  float *w0 = nullptr, *b0 = nullptr;  // conv1_1: [ky][kx][c_bgr][64], [64]
  SConv trunk[kNTrunk];
  SConv head[kSfdLevels];
  float* normw[3] = {nullptr, nullptr, nullptr};
  void *bufA = nullptr, *bufB = nullptr, *bufN = nullptr;  // T::elem: ping-pong activations, the L2-normalised map
  float *headraw = nullptr, *maps = nullptr, *dense = nullptr;
  int last_P = 0;  // positions per view of the last detect / post (float_sfd_dense, float_sfd_dense_batch)
  int last_n = 0;  // its views
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

// The workspace for n views of H x W: every term of sfd_plan(H, W) times n, never below what the handle has.  create and
// float_sfd_reserve_batch are the only callers; the run-time calls check the capacity and refuse.
int ensure_workspace(float_sfd* h, int n, int H, int W) {
  const SfdPlan p = sfd_plan(H, W);
  const size_t act = (size_t)n * p.max_act, norm = (size_t)n * p.max_norm, head = (size_t)n * p.max_head,
               pos = (size_t)n * p.g.pos0[kSfdLevels];
  if (act <= h->cap_act && norm <= h->cap_norm && head <= h->cap_head && pos <= h->cap_pos) return FLOAT_OK;
  // the new buffers first: a failed allocation (64 large views) leaves the handle as it was, single-view calls included
  const size_t a = std::max(act, h->cap_act), nn = std::max(norm, h->cap_norm), hd = std::max(head, h->cap_head),
               ps = std::max(pos, h->cap_pos);
  const size_t esz = h->cfg.dtype == FLOAT_DT_FP32 ? 4 : 2;  // bytes per activation element
  DevicePool nw;
  void *bufA = nullptr, *bufB = nullptr, *bufN = nullptr;
  float *headraw = nullptr, *maps = nullptr, *dense = nullptr;
  int rc = 0;
  auto AE = [&](void** dst, size_t cnt) {
    unsigned char* b = nullptr;
    if (!rc) rc = nw.alloc(&b, cnt * esz, true);
    *dst = b;
  };
  AE(&bufA, a);
  AE(&bufB, a);
  AE(&bufN, nn);
  if (!rc) rc = nw.alloc(&headraw, hd * kSfdHeadC, true);
  if (!rc) rc = nw.alloc(&maps, ps * 6, true);
  if (!rc) rc = nw.alloc(&dense, ps * 5, true);
  if (rc) {
    nw.release();
    return rc;
  }
  if (h->cap_act) {  // earlier calls, on any stream, may still use the old buffers
    const hipError_t e = hipDeviceSynchronize();
    if (e != hipSuccess) {
      nw.release();
      fh_set_error("hipDeviceSynchronize failed: %s", hipGetErrorString(e));
      return FLOAT_E_HIP;
    }
  }
  h->ws.release();
  h->ws = nw;
  h->bufA = bufA, h->bufB = bufB, h->bufN = bufN;
  h->headraw = headraw, h->maps = maps, h->dense = dense;
  h->cap_act = a, h->cap_norm = nn, h->cap_head = hd, h->cap_pos = ps;
  h->last_P = h->last_n = 0;  // the dense rows went with the old buffers
  return FLOAT_OK;
}

template <class T>
int create_impl(float_sfd* h, const TensorTable& tt) {
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
  if ((rc = ensure_workspace(h, 1, h->cfg.max_h, h->cfg.max_w)) || (rc = h->pool.alloc(&h->sat, 1, true))) return rc;
  (void)hipFuncSetAttribute(reinterpret_cast<const void*>(sfd_select_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, kSfdMaxCand * 32);
  (void)hipGetLastError();
  return FLOAT_OK;
}

template <class T>
int launch_conv(const SConv& L, const void* X, int n, int Hi, int Wi, void* Y, float* Yf32, int relu, hipStream_t st, unsigned long long* sat) {
  SfdConvArgs g;
  memset(&g, 0, sizeof(g));
  g.X = X;
  g.W = L.W;
  g.Y = Y;
  g.Yf32 = Yf32;
  g.bias = L.bias;
  g.n = n;
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
  const int mb = (n * npix + 63) / 64;  // n <= 64 views of at most 4096 x 4096 pixels: at most 2^30
  if (L.cout % 64 == 0) hipLaunchKernelGGL((sfd_conv_kernel<T, 4>), dim3(mb, L.cout / 64), dim3(256), 0, st, g);
  else hipLaunchKernelGGL((sfd_conv_kernel<T, 1>), dim3(mb, L.cout / 16), dim3(256), 0, st, g);
  FH_CHECK_HIP(hipGetLastError());
  return FLOAT_OK;
}

// the network on n stacked views: per view the 12 maps (per level conf [2][npix], loc [4][npix], at float offset 6 * pos0[level])
// into maps_out + view * 6 P
template <class T>
int forward_impl(float_sfd* h, const unsigned char* rgb8, int n, int H, int W, const SfdGeom& geo, float* maps_out, hipStream_t st) {
  typedef typename T::elem E;
  int rc;
  void *cur = h->bufA, *oth = h->bufB;
  int hh = H, ww = W;
  {
    const size_t tot = (size_t)n * H * W * 8;
    hipLaunchKernelGGL((sfd_first_kernel<T>), dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, st, rgb8, h->w0, h->b0,
                       reinterpret_cast<E*>(cur), n, H, W, h->sat);
  }
  for (int i = 0; i < kNTrunk; ++i) {
    const TrunkDef& L = kTrunk[i];
    if ((rc = launch_conv<T>(h->trunk[i], cur, n, hh, ww, oth, nullptr, 1, st, h->sat))) return rc;
    std::swap(cur, oth);
    hh = (hh + 2 * L.pad - L.k) / L.stride + 1;
    ww = (ww + 2 * L.pad - L.k) / L.stride + 1;
    const int npix = hh * ww;
    if (L.level >= 0 && npix > 0) {
      const void* feat = cur;
      if (L.level < 3) {
        hipLaunchKernelGGL((sfd_l2norm_kernel<T>), dim3((unsigned)((n * npix + 3) / 4)), dim3(256), 0, st, reinterpret_cast<const E*>(cur),
                           h->normw[L.level], reinterpret_cast<E*>(h->bufN), n * npix, L.cout, h->sat);
        feat = h->bufN;
      }
      if ((rc = launch_conv<T>(h->head[L.level], feat, n, hh, ww, nullptr, h->headraw, 0, st, h->sat))) return rc;
      float* conf = maps_out + (size_t)6 * geo.pos0[L.level];
      hipLaunchKernelGGL(sfd_maps_kernel, dim3((unsigned)((n * npix + 255) / 256)), dim3(256), 0, st, h->headraw, conf,
                         conf + (size_t)2 * npix, n, (size_t)6 * geo.pos0[kSfdLevels], npix, kHeadConf[L.level]);
    }
    if (L.pool) {
      const size_t tot = (size_t)n * (hh / 2) * (ww / 2) * (L.cout / 8);
      if (tot)
        hipLaunchKernelGGL((sfd_pool_kernel<T>), dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, st, reinterpret_cast<const E*>(cur),
                           reinterpret_cast<E*>(oth), n, hh, ww, L.cout, h->sat);
      std::swap(cur, oth);
      hh /= 2;
      ww /= 2;
    }
  }
  FH_CHECK_HIP(hipGetLastError());
  return FLOAT_OK;
}

int forward(float_sfd* h, const void* rgb8, int n, int H, int W, const SfdGeom& geo, float* maps_out, hipStream_t st) {
  const unsigned char* p = reinterpret_cast<const unsigned char*>(rgb8);
  if (h->cfg.dtype == FLOAT_DT_FP32) return forward_impl<FP32>(h, p, n, H, W, geo, maps_out, st);
  return h->cfg.dtype == FLOAT_DT_BF16 ? forward_impl<BF16>(h, p, n, H, W, geo, maps_out, st)
                                       : forward_impl<FP16>(h, p, n, H, W, geo, maps_out, st);
}

// maps (n, 6 P) -> dense (n, P, 5) in the handle, boxes (n, max_boxes, 5), counts (n, 2): one decode launch, one select launch
// with a workgroup per view
int post(float_sfd* h, const float* maps, int n, const SfdGeom& geo, float score_thr, float iou_thr, float* boxes, int32_t* counts,
         hipStream_t st) {
  const int P = geo.pos0[kSfdLevels];
  hipLaunchKernelGGL(sfd_decode_kernel, dim3((unsigned)((P + 255) / 256), n), dim3(256), 0, st, maps, geo, h->dense);
  hipLaunchKernelGGL(sfd_select_kernel, dim3(n), dim3(256), (size_t)h->cfg.max_candidates * 32, st, h->dense, P, score_thr, iou_thr,
                     h->cfg.max_candidates, h->cfg.max_boxes, boxes, counts);
  FH_CHECK_HIP(hipGetLastError());
  h->last_P = P;
  h->last_n = n;
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

// ... and every batched entry point: n within the reservation, the view within the reserved size
int check_batch(const char* fn, const float_sfd* h, int n, int H, int W) {
  int rc;
  FH_REQUIRE(n >= 1 && n <= kSfdMaxViews, "%s: n = %d views, a call takes 1 ... %d", fn, n, kSfdMaxViews);
  if ((rc = check_view(fn, h, H, W))) return rc;
  FH_REQUIRE(n <= h->res_n, "%s: n = %d views exceed the %d reserved: call float_sfd_reserve_batch first (run-time calls do not allocate)", fn,
             n, h->res_n);
  FH_REQUIRE(H <= h->res_h && W <= h->res_w,
             "%s: a %d x %d view (H x W) is beyond the reserved %d x %d: call float_sfd_reserve_batch first (run-time calls do not allocate)", fn,
             H, W, h->res_h, h->res_w);
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
  h->ws.release();
  delete h;
}

int float_sfd_detect(float_sfd_t* h, const void* rgb8, int32_t H, int32_t W, float score_thr, float iou_thr, float* boxes, int32_t* counts,
                     void* stream) {
  int rc;
  if ((rc = check_view("float_sfd_detect", h, H, W))) return rc;
  FH_REQUIRE(rgb8 && boxes && counts, "float_sfd_detect: null argument");
  const SfdPlan p = sfd_plan(H, W);
  if ((rc = forward(h, rgb8, 1, H, W, p.g, h->maps, (hipStream_t)stream))) return rc;
  return post(h, h->maps, 1, p.g, score_thr, iou_thr, boxes, counts, (hipStream_t)stream);
}

int float_sfd_maps(float_sfd_t* h, const void* rgb8, int32_t H, int32_t W, float* maps12, void* stream) {
  int rc;
  if ((rc = check_view("float_sfd_maps", h, H, W))) return rc;
  FH_REQUIRE(rgb8 && maps12, "float_sfd_maps: null argument");
  return forward(h, rgb8, 1, H, W, sfd_plan(H, W).g, maps12, (hipStream_t)stream);
}

int float_sfd_post(float_sfd_t* h, const float* maps12, int32_t H, int32_t W, float score_thr, float iou_thr, float* boxes, int32_t* counts,
                   void* stream) {
  int rc;
  if ((rc = check_view("float_sfd_post", h, H, W))) return rc;
  FH_REQUIRE(maps12 && boxes && counts, "float_sfd_post: null argument");
  return post(h, maps12, 1, sfd_plan(H, W).g, score_thr, iou_thr, boxes, counts, (hipStream_t)stream);
}

int float_sfd_dense(float_sfd_t* h, float* scores_boxes, void* stream) {
  FH_REQUIRE(h && scores_boxes, "float_sfd_dense: null argument");
  FH_REQUIRE(h->last_P > 0, "float_sfd_dense: no float_sfd_detect / float_sfd_post call on this handle yet");
  return fh_copy_d2d(scores_boxes, h->dense, (size_t)h->last_P * 5 * sizeof(float), (hipStream_t)stream);
}

int float_sfd_reserve_batch(float_sfd_t* h, int32_t n, int32_t H, int32_t W) {
  int rc;
  FH_REQUIRE(n >= 1 && n <= kSfdMaxViews, "float_sfd_reserve_batch: n = %d views, a call takes 1 ... %d", n, kSfdMaxViews);
  if ((rc = check_view("float_sfd_reserve_batch", h, H, W))) return rc;
  const int rn = std::max(n, h->res_n), rh = std::max(H, h->res_h), rw = std::max(W, h->res_w);
  if ((rc = ensure_workspace(h, rn, rh, rw))) return rc;  // allocates, and synchronises the device, only where it has to grow
  h->res_n = rn;
  h->res_h = rh;
  h->res_w = rw;
  return FLOAT_OK;
}

int float_sfd_maps_batch(float_sfd_t* h, const void* rgb8, int32_t n, int32_t H, int32_t W, float* maps12, void* stream) {
  int rc;
  if ((rc = check_batch("float_sfd_maps_batch", h, n, H, W))) return rc;
  FH_REQUIRE(rgb8 && maps12, "float_sfd_maps_batch: null argument (rgb8, maps12)");
  return forward(h, rgb8, n, H, W, sfd_plan(H, W).g, maps12, (hipStream_t)stream);
}

int float_sfd_post_batch(float_sfd_t* h, const float* maps12, int32_t n, int32_t H, int32_t W, float score_thr, float iou_thr, float* boxes,
                         int32_t* counts, void* stream) {
  int rc;
  if ((rc = check_batch("float_sfd_post_batch", h, n, H, W))) return rc;
  FH_REQUIRE(maps12 && boxes && counts, "float_sfd_post_batch: null argument (maps12, boxes, counts)");
  return post(h, maps12, n, sfd_plan(H, W).g, score_thr, iou_thr, boxes, counts, (hipStream_t)stream);
}

int float_sfd_detect_batch(float_sfd_t* h, const void* rgb8, int32_t n, int32_t H, int32_t W, float score_thr, float iou_thr, float* boxes,
                           int32_t* counts, void* stream) {
  int rc;
  if ((rc = check_batch("float_sfd_detect_batch", h, n, H, W))) return rc;
  FH_REQUIRE(rgb8 && boxes && counts, "float_sfd_detect_batch: null argument (rgb8, boxes, counts)");
  const SfdPlan p = sfd_plan(H, W);
  if ((rc = forward(h, rgb8, n, H, W, p.g, h->maps, (hipStream_t)stream))) return rc;
  return post(h, h->maps, n, p.g, score_thr, iou_thr, boxes, counts, (hipStream_t)stream);
}

int float_sfd_dense_batch(float_sfd_t* h, float* scores_boxes, void* stream) {
  FH_REQUIRE(h && scores_boxes, "float_sfd_dense_batch: null argument (handle, scores_boxes)");
  FH_REQUIRE(h->last_P > 0, "float_sfd_dense_batch: no detect / post call on this handle since its workspace was sized");
  return fh_copy_d2d(scores_boxes, h->dense, (size_t)h->last_n * h->last_P * 5 * sizeof(float), (hipStream_t)stream);
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
