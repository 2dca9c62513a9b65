// Host-side checkpoint handling of the decoder operator: validation of the state dict's tensors and FIR buffers, and the
// packing of StyledConv / ToFlow / ToRGB weights into the layouts of dec_kernels.hpp.  Included by dec_api.hip only.
#pragma once
#include <math.h>

#include "common.hpp"

namespace {

struct Styled {  // one StyledConv (styledecoder.py:302-325)
  int cin = 0, cout = 0;
  bool up = false;
  void* W = nullptr;      // T::elem; plain: [9][Cout][Cin]; up: four parity classes, [4+2+2+1][Cout][Cin]
  float* WsqT = nullptr;  // [Cin][Cout] sum over taps of W^2 (fp32)
  float* abias = nullptr; // [Cout] FusedLeakyReLU bias
  int style_off = 0, demod_off = 0;
  // up: 1-D taps of the Blur behind the transposed conv (styledecoder.py:209-213: make_kernel(k) * 4, applied by upfirdn2d as a
  // true convolution): fir[b] = weight of z[X - 1 + b] in output X = 2 k[3 - b] / sum(k); {0.25, 0.75, 0.75, 0.25} for [1,3,3,1]
  float fir[4] = {0.25f, 0.75f, 0.75f, 0.25f};
};

struct Level {  // ToFlow + ToRGB of one resolution
  int R = 0, C = 0;
  float *wflow = nullptr, *bflow = nullptr, *wrgb = nullptr, *b1 = nullptr, *b2 = nullptr;
  float* lin = nullptr;  // [R] np.linspace(-1, 1, R) as float32
  int style_off = 0;
  void* feat = nullptr;  // [R][R][C] T::elem
  float* grgb = nullptr;  // [R][R][4]: ToRGB's conv of `feat` (dec_feat_rgb_kernel, refreshed whenever the features are set)
  float upk_flow[8], upk_rgb[8];  // per-axis taps of the two Upsamples (upsample_taps)
};

int ilog2(int v) {
  int l = 0;
  while ((1 << l) < v) ++l;
  return l;
}

const float_tensor_t* need(const TensorTable& tt, const std::string& k, int64_t numel) {
  const float_tensor_t* t = tt.find(k);
  if (!t) {
    fh_set_error("missing checkpoint tensor '%s'", k.c_str());
    return nullptr;
  }
  if (numel >= 0 && TensorTable::numel(t) != numel) {
    fh_set_error("tensor '%s' has %lld elements, expected %lld", k.c_str(), (long long)TensorTable::numel(t), (long long)numel);
    return nullptr;
  }
  return t;
}

template <class T>
int upload_elem(DevicePool* pool, const std::vector<float>& src, void** dst) {
  typedef typename T::elem E;
  std::vector<E> tmp(src.size());
  for (size_t i = 0; i < src.size(); ++i) tmp[i] = T::host_from_float(src[i]);
  E* d = nullptr;
  int rc = pool->alloc(&d, tmp.size(), false);
  if (rc) return rc;
  *dst = d;
  FH_CHECK_HIP(hipMemcpy(d, tmp.data(), tmp.size() * sizeof(E), hipMemcpyHostToDevice));
  return FLOAT_OK;
}

template <class T>
int alloc_elem(DevicePool* pool, void** dst, size_t count) {
  typename T::elem* d = nullptr;
  int rc = pool->alloc(&d, count, true);
  *dst = d;
  return rc;
}

int upload32(DevicePool* pool, const std::vector<float>& src, float** dst) {
  int rc = pool->alloc(dst, src.size(), false);
  if (rc) return rc;
  FH_CHECK_HIP(hipMemcpy(*dst, src.data(), src.size() * sizeof(float), hipMemcpyHostToDevice));
  return FLOAT_OK;
}

// Parity classes of conv_transpose2d(stride 2, 3x3): output row u = 2m + pu receives kernel rows
// ky with 2y + ky = u: pu = 0 -> (ky=0, y=m), (ky=2, y=m-1); pu = 1 -> (ky=1, y=m).
struct ClassTaps {
  int n;
  int ky[4], kx[4], dy[4], dx[4];
};
ClassTaps class_taps(int pu, int pv) {
  ClassTaps c;
  c.n = 0;
  // taps listed with ascending input offset (dy = -1 first), the order dec_conv16_kernel enumerates
  const int kys[2][2] = {{2, 0}, {1, -1}}, dys[2][2] = {{-1, 0}, {0, 0}};
  for (int a = 0; a < 2; ++a) {
    if (kys[pu][a] < 0) continue;
    for (int b = 0; b < 2; ++b) {
      if (kys[pv][b] < 0) continue;
      c.ky[c.n] = kys[pu][a];
      c.dy[c.n] = dys[pu][a];
      c.kx[c.n] = kys[pv][b];
      c.dx[c.n] = dys[pv][b];
      ++c.n;
    }
  }
  return c;
}

// 1-D taps of an up-sampling FIR (the Blur behind a transposed conv, styledecoder.py:209-213).  What the reference ends up
// with: Synthesis(blur_kernel=...) builds make_kernel(k) * 4 = outer(k, k) * 4 / sum(k)^2 as a registered BUFFER, and the strict
// load_state_dict (nodes_vadv_loader.py:632) then overwrites it with the checkpoint's `<conv>.blur.kernel` - so the checkpoint's
// buffer wins when it is there, the loader's widget (`blur_kernel`, optional tensor of 4 taps) only when it is not, [1,3,3,1]
// otherwise.  upfirdn2d convolves (correlates with the flipped kernel, styledecoder.py:28-29): fir[b] = weight of z[X - 1 + b]
// in output X.  A buffer must be a 4 x 4 outer product a (x) a (what make_kernel produces); anything else is refused.
int blur_taps(const TensorTable& tt, const std::string& buffer_key, float fir[4]) {
  const float_tensor_t* wk = tt.find("blur_kernel");
  if (wk && TensorTable::numel(wk) != 4) {
    fh_set_error("blur_kernel has %lld taps; the HIP decoder implements 4-tap kernels", (long long)TensorTable::numel(wk));
    return FLOAT_E_INVALID;
  }
  if (const float_tensor_t* kb = tt.find(buffer_key)) {
    if (TensorTable::numel(kb) != 16 || kb->ndim != 2 || kb->shape[0] != 4) {
      fh_set_error("'%s' is not a 4 x 4 kernel; the HIP decoder implements 4-tap blur kernels", buffer_key.c_str());
      return FLOAT_E_INVALID;
    }
    double r[4] = {0, 0, 0, 0}, S = 0, amax = 0;
    for (int i = 0; i < 4; ++i)
      for (int j = 0; j < 4; ++j) {
        r[i] += kb->data[i * 4 + j];
        S += kb->data[i * 4 + j];
        amax = std::max(amax, (double)fabsf(kb->data[i * 4 + j]));
      }
    if (!(S > 1e-12)) {
      fh_set_error("'%s' does not have a positive sum", buffer_key.c_str());
      return FLOAT_E_INVALID;
    }
    double a[4];
    for (int i = 0; i < 4; ++i) a[i] = r[i] / sqrt(S);  // K = a (x) a  =>  row sums = a_i * sum(a), S = sum(a)^2
    for (int i = 0; i < 4; ++i)
      for (int j = 0; j < 4; ++j)
        if (fabs(kb->data[i * 4 + j] - a[i] * a[j]) > 1e-5 * amax) {
          fh_set_error("'%s' is not an outer product k (x) k (make_kernel's form); other blur kernels are not implemented", buffer_key.c_str());
          return FLOAT_E_INVALID;
        }
    for (int b = 0; b < 4; ++b) fir[b] = (float)a[3 - b];
    return FLOAT_OK;
  }
  if (wk) {
    double sum = 0;
    for (int b = 0; b < 4; ++b) sum += wk->data[b];
    if (!(fabs(sum) > 1e-12)) {
      fh_set_error("blur_kernel sums to zero");
      return FLOAT_E_INVALID;
    }
    for (int b = 0; b < 4; ++b) fir[b] = (float)(2.0 * wk->data[3 - b] / sum);
  }
  return FLOAT_OK;
}

// The Upsample of ToRGB / ToFlow (styledecoder.py:373,394) is built with its default [1,3,3,1] whatever the loader's widget says
// (:489-491): make_kernel(k) * 4 as a registered 4 x 4 BUFFER `upsample.kernel`, which the strict load (nodes_vadv_loader.py:632)
// overwrites with the checkpoint's.  dec_flow_kernel applies it per axis: the buffer must be a rank-1 4 x 4 matrix K = ky (x) kx
// (every make_kernel of a 1-D kernel is; a x b with different factors passes too); taps = {ky[4], kx[4]}.  No buffer in the
// state: (1, 3, 3, 1) / 4 per axis.  Another size (the Upsample's padding belongs to 4 taps) or a rank > 1 kernel is refused.
int upsample_taps(const TensorTable& tt, const std::string& key, float taps[8]) {
  static const float dflt[4] = {0.25f, 0.75f, 0.75f, 0.25f};
  for (int i = 0; i < 8; ++i) taps[i] = dflt[i & 3];
  const float_tensor_t* kb = tt.find(key);
  if (!kb) return FLOAT_OK;
  if (TensorTable::numel(kb) != 16 || kb->ndim != 2 || kb->shape[0] != 4) {
    fh_set_error("'%s' is not a 4 x 4 kernel; ToRGB / ToFlow up-sampling kernels of other sizes are not implemented", key.c_str());
    return FLOAT_E_INVALID;
  }
  double r[4] = {0, 0, 0, 0}, c[4] = {0, 0, 0, 0}, S = 0, amax = 0;
  for (int i = 0; i < 4; ++i)
    for (int j = 0; j < 4; ++j) {
      const double v = kb->data[i * 4 + j];
      r[i] += v, c[j] += v, S += v;
      amax = std::max(amax, fabs(v));
    }
  if (!(S > 1e-12)) {
    fh_set_error("'%s' sums to %.3g: the per-axis split K = ky (x) kx of the flow kernel needs a positive sum (INTEGRATION.md, "
                 "'FIR buffers'); such an up-sampling kernel is not implemented", key.c_str(), S);
    return FLOAT_E_INVALID;
  }
  // K_ij = u_i v_j  =>  row sums u_i sum(v), column sums v_j sum(u), S = sum(u) sum(v): K_ij = r_i c_j / S
  const double rs = sqrt(S);
  double resid = 0.0;
  for (int i = 0; i < 4; ++i)
    for (int j = 0; j < 4; ++j) resid = std::max(resid, fabs(kb->data[i * 4 + j] - r[i] * c[j] / S));
  if (resid > 1e-5 * amax) {
    fh_set_error("'%s' is not a rank-1 kernel ky (x) kx (make_kernel's form): max |K - r c^T / sum| = %.3g against the limit 1e-5 * max|K| "
                 "= %.3g; other up-sampling kernels are not implemented (INTEGRATION.md, 'FIR buffers')", key.c_str(), resid, 1e-5 * amax);
    return FLOAT_E_INVALID;
  }
  for (int i = 0; i < 4; ++i) {
    taps[i] = (float)(r[i] / rs);
    taps[4 + i] = (float)(c[i] / rs);
  }
  return FLOAT_OK;
}

template <class T>
int pack_styled(DevicePool* pool, const TensorTable& tt, const std::string& p, int cin, int cout, bool up, Styled* s,
                std::vector<float>* WmT_host, std::vector<float>* bm_host, int style_dim) {
  s->cin = cin;
  s->cout = cout;
  s->up = up;
  const float_tensor_t* w = need(tt, p + ".conv.weight", (int64_t)cout * cin * 9);
  const float_tensor_t* mw = need(tt, p + ".conv.modulation.weight", (int64_t)cin * style_dim);
  const float_tensor_t* mb = need(tt, p + ".conv.modulation.bias", cin);
  const float_tensor_t* ab = need(tt, p + ".activate.bias", cout);
  if (!w || !mw || !mb || !ab) return FLOAT_E_MISSING;
  if (up) {
    int rc = blur_taps(tt, p + ".conv.blur.kernel", s->fir);
    if (rc) return rc;
  }
  const float scale = 1.0f / sqrtf((float)(cin * 9));  // styledecoder.py:223-224
  std::vector<float> packed((size_t)9 * cout * cin);
  auto W = [&](int o, int i, int ky, int kx) { return w->data[(((size_t)o * cin + i) * 3 + ky) * 3 + kx] * scale; };
  if (!up) {
    for (int ky = 0; ky < 3; ++ky)
      for (int kx = 0; kx < 3; ++kx)
        for (int o = 0; o < cout; ++o)
          for (int i = 0; i < cin; ++i) packed[(((size_t)(ky * 3 + kx)) * cout + o) * cin + i] = W(o, i, ky, kx);
  } else {
    size_t t0 = 0;
    for (int pu = 0; pu < 2; ++pu)
      for (int pv = 0; pv < 2; ++pv) {
        const ClassTaps c = class_taps(pu, pv);
        for (int t = 0; t < c.n; ++t, ++t0)
          for (int o = 0; o < cout; ++o)
            for (int i = 0; i < cin; ++i) packed[(t0 * cout + o) * cin + i] = W(o, i, c.ky[t], c.kx[t]);
      }
  }
  int rc;
  if ((rc = upload_elem<T>(pool, packed, &s->W))) return rc;
  std::vector<float> wsq((size_t)cin * cout, 0.f);
  for (int o = 0; o < cout; ++o)
    for (int i = 0; i < cin; ++i) {
      double a = 0;
      for (int k = 0; k < 9; ++k) {
        const double v = w->data[((size_t)o * cin + i) * 9 + k];
        a += v * v;
      }
      wsq[(size_t)i * cout + o] = (float)a;
    }
  if ((rc = upload32(pool, wsq, &s->WsqT))) return rc;
  if ((rc = upload32(pool, std::vector<float>(ab->data, ab->data + cout), &s->abias))) return rc;
  s->style_off = (int)bm_host->size();
  for (int i = 0; i < cin; ++i) bm_host->push_back(mb->data[i]);
  WmT_host->insert(WmT_host->end(), mw->data, mw->data + (size_t)cin * style_dim);  // [cin][style_dim], transposed later
  return FLOAT_OK;
}

// ToFlow `pf` + ToRGB `pr` of the R x R level with C channels: the 1x1 weights scaled by 1/sqrt(C), the three biases, the
// sampling grid's axis, both Upsamples' taps; ToFlow's modulation rows are appended to the shared table like pack_styled's.
// L->feat and L->grgb stay with the caller.
int pack_level(DevicePool* pool, const TensorTable& tt, const std::string& pf, const std::string& pr, int R, int C, Level* L,
               std::vector<float>* wm_rows, std::vector<float>* bm_host, int style_dim) {
  L->R = R, L->C = C;
  const float_tensor_t* fw = need(tt, pf + ".conv.weight", 3 * C);
  const float_tensor_t* fmw = need(tt, pf + ".conv.modulation.weight", (int64_t)C * style_dim);
  const float_tensor_t* fmb = need(tt, pf + ".conv.modulation.bias", C);
  const float_tensor_t* fb = need(tt, pf + ".bias", 3);
  const float_tensor_t* rw = need(tt, pr + ".conv.0.weight", 3 * C);
  const float_tensor_t* rb1 = need(tt, pr + ".conv.1.bias", 3);
  const float_tensor_t* rb2 = need(tt, pr + ".bias", 3);
  if (!fw || !fmw || !fmb || !fb || !rw || !rb1 || !rb2) return FLOAT_E_MISSING;
  int rc;
  if ((rc = upsample_taps(tt, pf + ".upsample.kernel", L->upk_flow)) || (rc = upsample_taps(tt, pr + ".upsample.kernel", L->upk_rgb))) return rc;
  const float sc = 1.0f / sqrtf((float)C);  // 1x1: fan_in = C (styledecoder.py:134,223)
  std::vector<float> a(3 * C), b(3 * C);
  for (int i = 0; i < 3 * C; ++i) {
    a[i] = fw->data[i] * sc;
    b[i] = rw->data[i] * sc;
  }
  if ((rc = upload32(pool, a, &L->wflow))) return rc;
  if ((rc = upload32(pool, b, &L->wrgb))) return rc;
  if ((rc = upload32(pool, std::vector<float>(fb->data, fb->data + 3), &L->bflow))) return rc;
  if ((rc = upload32(pool, std::vector<float>(rb1->data, rb1->data + 3), &L->b1))) return rc;
  if ((rc = upload32(pool, std::vector<float>(rb2->data, rb2->data + 3), &L->b2))) return rc;
  L->style_off = (int)bm_host->size();
  for (int i = 0; i < C; ++i) bm_host->push_back(fmb->data[i]);
  wm_rows->insert(wm_rows->end(), fmw->data, fmw->data + (size_t)C * style_dim);
  // np.linspace(-1, 1, R): start + i*step in float64, last element forced to stop, cast to f32
  std::vector<float> lin(R);
  const double step = 2.0 / (double)(R - 1);
  for (int i = 0; i < R; ++i) lin[i] = (float)(-1.0 + (double)i * step);
  lin[R - 1] = 1.0f;
  return upload32(pool, lin, &L->lin);
}

// The shared modulation table on the device: every EqualLinear's rows ([Stot][style_dim], as pack_styled / pack_level
// appended them) k-major, and their biases.
int upload_mod_table(DevicePool* pool, const std::vector<float>& wm_rows, const std::vector<float>& bm_host, int style_dim,
                     float** WmT, float** bm) {
  const size_t Stot = bm_host.size();
  std::vector<float> wmT((size_t)style_dim * Stot);
  for (size_t j = 0; j < Stot; ++j)
    for (int k = 0; k < style_dim; ++k) wmT[(size_t)k * Stot + j] = wm_rows[j * style_dim + k];
  int rc;
  if ((rc = upload32(pool, wmT, WmT))) return rc;
  return upload32(pool, bm_host, bm);
}

}  // namespace
