// C-ABI entry points of the decoder operator (include/float_hip.h): the handle and its workspace, the per-batch launch chain
// of Synthesis.forward (reference styledecoder.py:497-534) and the unit operators.  Checkpoint handling: dec_pack.hpp;
// launchers and the ride-along copy scheduler: dec_launch.hpp.
#include <math.h>
#include <stdlib.h>

#include "dec_kernels.hpp"
#include "dec_launch.hpp"

constexpr int kStyleCap = 256;

struct float_dec {
  float_dec_cfg_t cfg;
  DevicePool pool;
  int n_levels = 0, Stot = 0, Dtot = 0;
  std::vector<Styled> convs;  // [0] = conv1, [1 + i] = convs.i
  std::vector<Level> levels;
  float* WmT = nullptr;   // [style_dim][Stot] every modulation EqualLinear, k-major
  float* bm = nullptr;    // [Stot]
  float* cin_hwc = nullptr;  // ConstantInput as [4][4][512]
  bool feats_set = false;
  float* dirQ = nullptr;  // [style_dim][motion_dim] of QR(direction.weight + 1e-8) (styledecoder.py:435-436), if present
  int motion_dim = 0;
  // workspace.  Frames go through the decoder in three nested batches:
  //   style batch (<= kStyleCap frames): every style modulation + demod factor in two launches;
  //   low batch   (<= lo_frames): levels up to 32x32, where one frame is only 16..1024 pixels and
  //                               the 512-channel weights dominate, so many frames share a launch;
  //   high batch  (<= max_frames): levels 64..size, where activations are 17 MB per frame.
  int lo_levels = 0, lo_frames = 0;
  float *styles = nullptr, *demod = nullptr, *eps = nullptr;  // eps: [kStyleCap][16] = 1e-8 / (style normaliser)^2
  void *loA = nullptr, *loB = nullptr, *loZ = nullptr, *loX = nullptr;  // T::elem: low phase ping/pong/z + hand-over tensor
  void *hiA = nullptr, *hiB = nullptr, *hiZ = nullptr;
  // last level with <= 64 channels (round 6): ToFlow's conv in conv2's epilogue (dec_conv16_kernel FLOWM) - its per-frame weight
  // fragments and the [max_frames][size][size][4] sums that replace the stored V; FLOAT_DEC_FLOW_EPI=0 keeps dec_flow_kernel there
  void* wfrag = nullptr;
  float* oflow = nullptr;
  // I420 frames of a last level that does not end in dec_flowlast_kernel's I420 form (i420_fused false): [max_frames][size][size][3]
  // 8-bit RGB, which dec_rgb8_to_i420_kernel turns into the caller's planes behind the level
  bool i420_fused = false;
  unsigned char* rgb8 = nullptr;
  FhYuv yuv = fh_yuv_pack(kFhYuvRows[0]);  // the colour matrix of the I420 call that is running (float_dec_frames[_host]_i420 set it)
  unsigned long long* sat = nullptr;  // [kDecSatSites] saturation counters (dec_kernels.hpp), device
  DecTune tune;  // the environment's switches as float_dec_create found them (tuning.hpp)
  float *loFlow[2] = {nullptr, nullptr}, *loRgb[2] = {nullptr, nullptr};
  float *hiFlow[2] = {nullptr, nullptr}, *hiRgb[2] = {nullptr, nullptr};
  RideCopy ride;  // float_dec_frames_host, ride-along mode (dec_launch.hpp)
  std::vector<hipEvent_t> copy_events;  // float_dec_frames_host: one per high batch in flight, recycled across calls
  hipEvent_t join_event = nullptr;
};

namespace {

template <class T>
int create_impl(float_dec* h, const TensorTable& tt) {
  const int size = h->cfg.size, sdim = h->cfg.style_dim;
  const int log_size = ilog2(size);
  // channels by log2(resolution): the reference's table (styledecoder.py:457-467: 512 up to 32 px, then 256 / 128 / 64 / 32 / 16
  // times channel_multiplier) is read off the checkpoint itself - the output channels of every level's convs - so any
  // channel_multiplier loads (the kernels take channel counts in multiples of 32, the flow kernel up to 512)
  int chan[12] = {0, 0, 512, 512, 512, 512, 256, 128, 64, 32, 16, 0};
  {
    const float_tensor_t* c1 = tt.find("conv1.conv.weight");
    if (c1 && c1->ndim == 5) chan[2] = (int)c1->shape[1];
    for (int li = 0; li < log_size - 2; ++li) {
      const float_tensor_t* w = tt.find("convs." + std::to_string(2 * li) + ".conv.weight");
      if (w && w->ndim == 5) chan[li + 3] = (int)w->shape[1];
    }
    for (int l = 2; l <= log_size; ++l)
      FH_REQUIRE(chan[l] >= 32 && chan[l] <= 512 && chan[l] % 32 == 0 && (chan[l] & (chan[l] - 1)) == 0,
                 "decoder level %d px has %d channels: the HIP decoder takes powers of two in [32, 512]", 1 << l, chan[l]);
  }
  h->n_levels = log_size - 2;
  std::vector<float> wm_rows, bm_host;  // rows = modulation outputs, [Stot][sdim]
  int rc;
  h->convs.resize(1 + 2 * h->n_levels);
  if ((rc = pack_styled<T>(&h->pool, tt, "conv1", chan[2], chan[2], false, &h->convs[0], &wm_rows, &bm_host, sdim))) return rc;
  int cin = chan[2];
  for (int li = 0; li < h->n_levels; ++li) {
    const int cout = chan[li + 3];
    if ((rc = pack_styled<T>(&h->pool, tt, "convs." + std::to_string(2 * li), cin, cout, true, &h->convs[1 + 2 * li], &wm_rows,
                             &bm_host, sdim)))
      return rc;
    if ((rc = pack_styled<T>(&h->pool, tt, "convs." + std::to_string(2 * li + 1), cout, cout, false, &h->convs[2 + 2 * li],
                             &wm_rows, &bm_host, sdim)))
      return rc;
    cin = cout;
  }
  int doff = 0;
  for (auto& s : h->convs) {
    s.demod_off = doff;
    doff += s.cout;
  }
  h->Dtot = doff;
  h->levels.resize(h->n_levels);
  for (int li = 0; li < h->n_levels; ++li) {
    Level& L = h->levels[li];
    if ((rc = pack_level(&h->pool, tt, "to_flows." + std::to_string(li), "to_rgbs." + std::to_string(li), 8 << li, chan[li + 3], &L,
                         &wm_rows, &bm_host, sdim)))
      return rc;
    if ((rc = alloc_elem<T>(&h->pool, &L.feat, (size_t)L.R * L.R * L.C))) return rc;
    if ((rc = h->pool.alloc(&L.grgb, (size_t)L.R * L.R * 4, true))) return rc;
  }
  h->Stot = (int)bm_host.size();
  if ((rc = upload_mod_table(&h->pool, wm_rows, bm_host, sdim, &h->WmT, &h->bm))) return rc;
  // ConstantInput (1,512,4,4) -> HWC
  const float_tensor_t* ci = need(tt, "input.input", (int64_t)chan[2] * 16);
  if (!ci) return FLOAT_E_MISSING;
  std::vector<float> hwc((size_t)16 * chan[2]);
  for (int c = 0; c < chan[2]; ++c)
    for (int p = 0; p < 16; ++p) hwc[(size_t)p * chan[2] + c] = ci->data[(size_t)c * 16 + p];
  if ((rc = upload32(&h->pool, hwc, &h->cin_hwc))) return rc;
  // workspace
  h->lo_levels = 0;
  for (int li = 0; li < h->n_levels - 1; ++li)
    if ((8 << li) <= 32) h->lo_levels = li + 1;  // levels 8,16,32 (never the last level)
  h->lo_frames = std::min(128, std::max(h->cfg.max_frames, 8 * h->cfg.max_frames));
  const size_t FH = (size_t)h->cfg.max_frames, FL = (size_t)h->lo_frames;
  size_t act_lo = 16 * (size_t)chan[2], act_hi = 0, x_lo = 0;
  for (int li = 0; li < h->n_levels; ++li) {
    const size_t R = 8u << li;
    const size_t need = std::max((R + 1) * (R + 1) * (size_t)chan[li + 3], (R / 2) * (R / 2) * (size_t)chan[li + 2]);
    if (li < h->lo_levels) {
      act_lo = std::max(act_lo, need);
      x_lo = R * R * (size_t)chan[li + 3];
    } else {
      act_hi = std::max(act_hi, need);
    }
  }
  if ((rc = h->pool.alloc(&h->styles, (size_t)kStyleCap * h->Stot, true))) return rc;
  if ((rc = h->pool.alloc(&h->demod, (size_t)kStyleCap * h->Dtot, true))) return rc;
  if ((rc = h->pool.alloc(&h->eps, (size_t)kStyleCap * 16, true))) return rc;
  if ((rc = h->pool.alloc(&h->sat, (size_t)kDecSatSites, true))) return rc;
  if ((rc = alloc_elem<T>(&h->pool, &h->loA, FL * act_lo))) return rc;
  if ((rc = alloc_elem<T>(&h->pool, &h->loB, FL * act_lo))) return rc;
  if ((rc = alloc_elem<T>(&h->pool, &h->loZ, FL * act_lo))) return rc;
  if ((rc = alloc_elem<T>(&h->pool, &h->loX, FL * std::max(x_lo, (size_t)16 * chan[2])))) return rc;
  if ((rc = alloc_elem<T>(&h->pool, &h->hiA, FH * act_hi))) return rc;
  if ((rc = alloc_elem<T>(&h->pool, &h->hiB, FH * act_hi))) return rc;
  if ((rc = alloc_elem<T>(&h->pool, &h->hiZ, FH * act_hi))) return rc;
  if (h->tune.flow_epi && conv_takes_flow_epi(h->tune, h->convs.back(), size)) {  // run_level's `epi`
    const int cl = h->levels.back().C;
    if ((rc = alloc_elem<T>(&h->pool, &h->wfrag, FH * (size_t)(cl / 32) * (T::is32 ? 1 : 2) * 64 * 8))) return rc;
    if ((rc = h->pool.alloc(&h->oflow, FH * (size_t)size * size * 4, true))) return rc;
  }
  h->i420_fused = h->oflow && h->tune.yuv_fused && flowlast_takes_i420(size) && h->levels.back().C == h->convs.back().cout;
  if (!h->i420_fused && (rc = h->pool.alloc(&h->rgb8, FH * (size_t)size * size * 3, true))) return rc;
  const size_t sk_lo = FL * 32 * 32 * 4, sk_hi = FH * (size_t)size * size * 4;  // flow / rgb pyramids: 4 floats per pixel
  for (int i = 0; i < 2; ++i) {
    if ((rc = h->pool.alloc(&h->loFlow[i], sk_lo, true))) return rc;
    if ((rc = h->pool.alloc(&h->loRgb[i], sk_lo, true))) return rc;
    if ((rc = h->pool.alloc(&h->hiFlow[i], sk_hi, true))) return rc;
    if ((rc = h->pool.alloc(&h->hiRgb[i], sk_hi, true))) return rc;
  }
  return raise_lds_limits<T>(h->tune);
}

// One resolution level for `n` frames: x_in (R/2, scaled by the up-conv's style) -> z -> U -> V ->
// flow/warp/blend/rgb.  U and the next level's input may alias (U is dead once conv2 has run).
template <class T>
int run_level(float_dec* h, int li, int n, const void* x_in, void* Zb, void* U, void* V, void* xnext, const float* styles,
              const float* demod, const float* flow_prev, const float* rgb_prev, float* flow_cur, float* rgb_cur,
              void* final_out, DecOut final_mode, hipStream_t st) {
  const Level& L = h->levels[li];
  const Styled& up = h->convs[1 + 2 * li];
  const Styled& c2 = h->convs[2 + 2 * li];
  const int R = L.R;
  const DecLaunch cx{h->tune, &h->ride, st};
  const Rows styles_c2{styles + c2.style_off, h->Stot};
  int rc;
  if ((rc = launch_upconv<T>(cx, up, R / 2, n, x_in, Zb, U, &U, Rows{demod + up.demod_off, h->Dtot}, styles_c2, h->sat + 1 + 2 * li))) return rc;
  // conv2 (plain 3x3); its unscaled output V feeds ToFlow.  Last level with conv2's whole channel range in one workgroup
  // (conv_takes_flow_epi: 32 or 64 channels, by the same conv_bn launch_conv tiles with; float_dec_create allocated wfrag /
  // oflow on that test): ToFlow's conv rides in conv2's epilogue, V is not stored and dec_flowlast_kernel finishes the frame.
  // Otherwise dec_flow_kernel reads the stored V.  (The WHOLE flow phase in that epilogue was bitwise equal and slower, 30.5-30.9
  // vs 26.2 ms per 250 frames: DESIGN_HISTORY.md.)
  const bool last = (li == h->n_levels - 1);
  const bool epi = last && h->oflow && conv_takes_flow_epi(h->tune, c2, R) && L.C == c2.cout;
  if (epi) {
    typedef typename T::pack8 P8;
    hipLaunchKernelGGL((dec_flowfrag_kernel<T>), dim3(n, c2.cout / 32), dim3(64), 0, st, reinterpret_cast<P8*>(h->wfrag), L.wflow,
                       styles + L.style_off, h->Stot, L.C);
  }
  if ((rc = launch_conv<T>(cx, ConvGeom::same3x3(R), c2, U, V, n, Rows{demod + c2.demod_off, h->Dtot}, Rows{}, h->sat + 2 + 2 * li,
                           epi ? h->wfrag : nullptr, epi ? h->oflow : nullptr)))
    return rc;
  FlowArgs g = flow_args_of(L, styles, h->Stot, n);
  g.x = V;
  g.pflow = flow_prev;
  g.prgb = rgb_prev;
  g.snext = last ? nullptr : styles + h->convs[1 + 2 * (li + 1)].style_off;
  g.xnext = last ? nullptr : xnext;
  g.flow_out = flow_cur;
  g.rgb_out = rgb_cur;
  // I420: in the last-level kernel itself where it has the form for it, else 8-bit RGB into rgb8 and the converter behind it
  const bool via_rgb8 = last && final_mode == kOutI420 && !(epi && h->i420_fused);
  FH_REQUIRE(!via_rgb8 || h->rgb8, "I420 frames: the handle has no 8-bit RGB scratch");
  g.final_out = last ? (via_rgb8 ? h->rgb8 : final_out) : nullptr;
  g.final_mode = last ? (via_rgb8 ? kOutU8 : final_mode) : kOutNone;
  g.yuv = h->yuv;
  g.write_pyr = (!last || h->tune.write_pyr) ? 1 : 0;
  g.sat = h->sat + 16 + li;
  g.oflow = epi ? h->oflow : nullptr;
#ifdef DEC_STAMPS
  if (last) {
    const unsigned long long init[4] = {~0ull, 0ull, ~0ull, 0ull};
    FH_CHECK_HIP(hipMemcpyToSymbolAsync(HIP_SYMBOL(g_dec_stamps), init, sizeof(init), 0, hipMemcpyHostToDevice, st));
  }
#endif
  if ((rc = launch_flow<T>(cx, g))) return rc;
  return via_rgb8 ? launch_rgb8_to_i420(cx, h->rgb8, final_out, n, R, h->yuv) : FLOAT_OK;
}

// Low phase for `n` frames (n <= lo_frames): constant input, conv1, levels 8..32.  Leaves the
// next level's (scaled) input in loX and the flow / rgb pyramids in loFlow[k] / loRgb[k]; returns k.
template <class T>
int run_low(float_dec* h, int n, const float* styles, const float* demod, int* skip_idx, hipStream_t st) {
  int rc;
  const Styled& c1 = h->convs[0];
  const int tot = n * 16 * c1.cin / 4;
  hipLaunchKernelGGL((dec_input_kernel<T>), dim3((tot + 255) / 256), dim3(256), 0, st, reinterpret_cast<typename T::elem*>(h->loB),
                     h->cin_hwc, styles + c1.style_off, h->Stot, n, 16, c1.cin, h->sat + 32);
  void* first_out = h->lo_levels > 0 ? h->loA : h->loX;
  // conv1: plain 3x3 at 4 px, scaled by the first up-conv's style
  if ((rc = launch_conv<T>(DecLaunch{h->tune, nullptr, st}, ConvGeom::same3x3(4), c1, h->loB, first_out, n, Rows{demod + c1.demod_off, h->Dtot},
                           Rows{styles + h->convs[1].style_off, h->Stot}, h->sat + 0)))
    return rc;
  int cur = 0;
  const float *fp = nullptr, *rp = nullptr;
  for (int li = 0; li < h->lo_levels; ++li) {
    void* xnext = (li == h->lo_levels - 1) ? h->loX : h->loA;
    if ((rc = run_level<T>(h, li, n, h->loA, h->loZ, h->loA, h->loB, xnext, styles, demod, fp, rp, h->loFlow[cur], h->loRgb[cur],
                           nullptr, kOutNone, st)))
      return rc;
    fp = h->loFlow[cur];
    rp = h->loRgb[cur];
    cur ^= 1;
  }
  *skip_idx = cur ^ 1;  // buffers holding the last written pyramids (unused when lo_levels == 0)
  return FLOAT_OK;
}

// High phase for `n` frames (n <= max_frames) that sit at frame offset `off` inside the low batch.
template <class T>
int run_high(float_dec* h, int n, int off, const float* styles, const float* demod, int skip_idx, void* out, DecOut final_mode,
             hipStream_t st) {
  int rc;
  const int l0 = h->lo_levels;
  typedef typename T::elem E;
  const void* x_in;
  const float *fp = nullptr, *rp = nullptr;
  if (l0 > 0) {
    const Level& P = h->levels[l0 - 1];
    x_in = reinterpret_cast<const E*>(h->loX) + (size_t)off * P.R * P.R * P.C;
    fp = h->loFlow[skip_idx] + (size_t)off * P.R * P.R * 4;
    rp = h->loRgb[skip_idx] + (size_t)off * P.R * P.R * 4;
  } else {
    x_in = reinterpret_cast<const E*>(h->loX) + (size_t)off * 16 * h->convs[0].cout;
  }
  int cur = 0;
  for (int li = l0; li < h->n_levels; ++li) {
    if ((rc = run_level<T>(h, li, n, x_in, h->hiZ, h->hiA, h->hiB, h->hiA, styles, demod, fp, rp, h->hiFlow[cur], h->hiRgb[cur],
                           out, final_mode, st)))
      return rc;
    x_in = h->hiA;
    fp = h->hiFlow[cur];
    rp = h->hiRgb[cur];
    cur ^= 1;
  }
  return FLOAT_OK;
}

// host != nullptr: every finished high batch is copied to host + (its offset) on `cs` while `st` renders the next one
// (float_dec_frames_host); `st` is made to wait for the last copy before the call returns.  out_v / host_v / host_dev_v hold
// floats, or uint8_t with kOutU8 / kOutI420: every offset and byte count below goes by the bytes of one frame.
template <class T>
int frames_impl(float_dec* h, const float* s_r, const float* r_d, int n_frames, void* out_v, DecOut final_mode, hipStream_t st,
                void* host_v = nullptr, hipStream_t cs = nullptr, void* host_dev_v = nullptr) {
  const int S = h->cfg.size, sdim = h->cfg.style_dim, FH = h->cfg.max_frames, FL = h->lo_frames;
  const size_t fbytes = out_frame_bytes(final_mode, S);
  char *const out = static_cast<char*>(out_v), *const host = static_cast<char*>(host_v), *const host_dev = static_cast<char*>(host_dev_v);
  size_t n_copy = 0;
  const DecTune& tn = h->tune;
  // same-stream hand-over: copy workgroups ride along the next batch's launches unless FLOAT_DEC_COPY=memcpy
  // the copy workgroups store straight through `host`: only when it is device-accessible (pinned / registered) host memory
  // (host_dev = its device-side address); a pageable destination takes the hipMemcpyAsync path, batch by batch, in order
  const bool ride = host_dev && cs == st && !tn.copy_memcpy && (fbytes % 16 == 0) &&
                    ((uintptr_t)host_dev % 16 == 0) && ((uintptr_t)out % 16 == 0);
  h->ride.reset();
  const StyleTable table{h->WmT, h->bm, h->Stot, h->Dtot, h->styles, h->eps, h->demod};
  int rc;
  // Ragged clips put their SHORT piece first at every level (style chunk, low group, high batch): the last batch of the call is
  // then a full one.  A short last batch carried the previous full batch's copy in launches too short for it (its launches took
  // as long as a full batch's) and the short first batch carries nothing.
  auto piece = [](int done, int total, int cap) {
    const int r = total % cap;
    return (done == 0 && r) ? r : std::min(cap, total - done);
  };
  for (int s0 = 0, ns = 0; s0 < n_frames; s0 += ns) {
    ns = piece(s0, n_frames, kStyleCap);
    // every style modulation (22 EqualLinears) and every demod factor for `ns` frames
    if ((rc = launch_styles(table, h->convs.data(), h->convs.size(), r_d + (size_t)s0 * sdim, s_r, sdim, ns, tn.style_norm, h->sat, st))) return rc;
    for (int a0 = 0, na = 0; a0 < ns; a0 += na) {
      na = piece(a0, ns, FL);
      const float* st_a = h->styles + (size_t)a0 * h->Stot;
      const float* dm_a = h->demod + (size_t)a0 * h->Dtot;
      int skip_idx = 0;
      if ((rc = run_low<T>(h, na, st_a, dm_a, &skip_idx, st))) return rc;
      for (int b0 = 0, nb = 0; b0 < na; b0 += nb) {
        nb = piece(b0, na, FH);
        const size_t off = (size_t)(s0 + a0 + b0) * fbytes;
        if (host && ride) h->ride.open_batch(tn, h->levels, h->lo_levels);  // this batch's launches carry the previous one's frames
        rc = run_high<T>(h, nb, b0, st_a + (size_t)b0 * h->Stot, dm_a + (size_t)b0 * h->Dtot, skip_idx, out + off, final_mode, st);
        if (rc) return rc;
        const size_t bytes = (size_t)nb * fbytes;
        if (host && ride) {
          if ((rc = h->ride.hand_over(out + off, host_dev + off, host + off, bytes, st))) return rc;
        } else if (host && cs == st) {  // in-order copy behind the batch's last kernel
          FH_CHECK_HIP(hipMemcpyAsync(host + off, out + off, bytes, hipMemcpyDeviceToHost, st));
        } else if (host) {
          if (n_copy >= h->copy_events.size()) {
            hipEvent_t e;
            FH_CHECK_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
            h->copy_events.push_back(e);
          }
          hipEvent_t e = h->copy_events[n_copy++];
          FH_CHECK_HIP(hipEventRecord(e, st));
          FH_CHECK_HIP(hipStreamWaitEvent(cs, e, 0));
          FH_CHECK_HIP(hipMemcpyAsync(host + off, out + off, bytes, hipMemcpyDeviceToHost, cs));
        }
      }
    }
  }
  if (host && ride && (rc = h->ride.flush(st))) return rc;  // the last batch has no successor to ride along
  if (host && n_copy) {  // join: work queued on `st` after this call sees the frames in host memory
    if (!h->join_event) FH_CHECK_HIP(hipEventCreateWithFlags(&h->join_event, hipEventDisableTiming));
    FH_CHECK_HIP(hipEventRecord(h->join_event, cs));
    FH_CHECK_HIP(hipStreamWaitEvent(st, h->join_event, 0));
  }
  FH_CHECK_HIP(hipGetLastError());
  return FLOAT_OK;
}

// G = ToRGB(features) of every level, after the features changed
template <class T>
int feats_rgb_impl(float_dec* h, hipStream_t st) {
  for (int li = 0; li < h->n_levels; ++li) {
    const Level& L = h->levels[li];
    const int npix = L.R * L.R;
    hipLaunchKernelGGL((dec_feat_rgb_kernel<T>), dim3((npix + 255) / 256), dim3(256), 0, st, L.grgb,
                       reinterpret_cast<const typename T::elem*>(L.feat), L.wrgb, L.C, npix);
  }
  FH_CHECK_HIP(hipGetLastError());
  return FLOAT_OK;
}

template <class T>
int set_feats_impl(float_dec* h, const float* const* feats, hipStream_t st) {
  for (int li = 0; li < h->n_levels; ++li) {
    const Level& L = h->levels[li];
    const int tot = L.C * L.R * L.R / 4;
    hipLaunchKernelGGL((dec_feat_pack_kernel<T>), dim3((tot + 255) / 256), dim3(256), 0, st, reinterpret_cast<typename T::elem*>(L.feat),
                       feats[li], L.C, L.R * L.R, h->sat + 33);
  }
  FH_CHECK_HIP(hipGetLastError());
  return feats_rgb_impl<T>(h, st);
}

// Run `call` with T = the handle's operand type.
#define DEC_DISPATCH(dtype, call)                          \
  ((dtype) == FLOAT_DT_FP32 ? ([&] { typedef FP32 T; return call; })() : ([&] { typedef FP16 T; return call; })())

// One StyledConv / one ToFlow + ToRGB level on caller data (float_dec_debug_*): a private pool, the production launchers.
struct UnitCtx {
  DevicePool pool;
  ~UnitCtx() { pool.release(); }
};

// The modulation table of the rows pack_styled / pack_level left in `wm_rows` / `bm_host`, and room for F frames' styles (and,
// with Dtot output channels to demodulate, eps + demod factors).
int unit_style_table(UnitCtx* u, const std::vector<float>& wm_rows, const std::vector<float>& bm_host, int sdim, int F, int Dtot,
                     StyleTable* t) {
  *t = StyleTable{nullptr, nullptr, (int)bm_host.size(), Dtot, nullptr, nullptr, nullptr};
  int rc;
  if ((rc = upload_mod_table(&u->pool, wm_rows, bm_host, sdim, &t->WmT, &t->bm))) return rc;
  if ((rc = u->pool.alloc(&t->styles, (size_t)F * t->Stot, true))) return rc;
  if (Dtot && ((rc = u->pool.alloc(&t->demod, (size_t)F * Dtot, true)) || (rc = u->pool.alloc(&t->eps, (size_t)F * 16, true)))) return rc;
  return FLOAT_OK;
}

template <class T>
int unit_styled_conv(const float_dec_unit_t* cfg, const TensorTable& tt, const float* x, const float* style, float* out,
                     uint64_t* saturated, int style_norm, hipStream_t st) {
  typedef typename T::elem E;
  const int cin = cfg->cin, cout = cfg->cout, Ri = cfg->res, F = cfg->n_frames, sdim = cfg->style_dim;
  const int Ro = cfg->upsample ? 2 * Ri : Ri;
  UnitCtx u;
  const DecTune tn = DecTune::from_env();  // no handle: the switches as this call finds them
  const DecLaunch cx{tn, nullptr, st};
  int rc;
  if ((rc = raise_lds_limits<T>(tn))) return rc;
  Styled s;
  std::vector<float> wm_rows, bm_host;
  if ((rc = pack_styled<T>(&u.pool, tt, "sc", cin, cout, cfg->upsample != 0, &s, &wm_rows, &bm_host, sdim))) return rc;
  StyleTable t;
  if ((rc = unit_style_table(&u, wm_rows, bm_host, sdim, F, cout, &t))) return rc;
  float* ones = nullptr;
  unsigned long long* sat = nullptr;
  if ((rc = u.pool.alloc(&sat, 1, true))) return rc;
  if ((rc = upload32(&u.pool, std::vector<float>((size_t)F * cout, 1.0f), &ones))) return rc;
  if ((rc = launch_styles(t, &s, 1, style, nullptr, sdim, F, style_norm != 0, nullptr, st))) return rc;
  E *X = nullptr, *Z = nullptr, *U = nullptr;
  const size_t nin = (size_t)F * Ri * Ri * cin, nout = (size_t)F * (Ro + 1) * (Ro + 1) * cout;
  if ((rc = u.pool.alloc(&X, nin, true))) return rc;
  if ((rc = u.pool.alloc(&Z, nout, true))) return rc;
  if ((rc = u.pool.alloc(&U, nout, true))) return rc;
  hipLaunchKernelGGL((dec_dbg_pack_kernel<T>), dim3((unsigned)((nin / 4 + 255) / 256)), dim3(256), 0, st, X, x, t.styles, cin, F, cin,
                     Ri * Ri, sat);
  void* Y = U;
  if (cfg->upsample) {
    if ((rc = launch_upconv<T>(cx, s, Ri, F, X, Z, U, &Y, Rows{t.demod, cout}, Rows{ones, cout}, sat))) return rc;
  } else {
    if ((rc = launch_conv<T>(cx, ConvGeom::same3x3(Ri), s, X, U, F, Rows{t.demod, cout}, Rows{}, sat))) return rc;
  }
  const size_t no = (size_t)F * Ro * Ro * cout;
  hipLaunchKernelGGL((dec_dbg_unpack_kernel<T>), dim3((unsigned)((no + 255) / 256)), dim3(256), 0, st, out, reinterpret_cast<const E*>(Y), F,
                     cout, Ro * Ro);
  FH_CHECK_HIP(hipGetLastError());
  FH_CHECK_HIP(hipStreamSynchronize(st));
  unsigned long long n = 0;
  FH_CHECK_HIP(hipMemcpy(&n, sat, sizeof(n), hipMemcpyDeviceToHost));
  if (saturated) *saturated = n;
  return FLOAT_OK;
}

template <class T>
int unit_flow_level(const float_dec_unit_t* cfg, const TensorTable& tt, const float* x, const float* feat, const float* style,
                    const float* prev_flow, const float* prev_rgb, float* out_flow, float* out_blend, float* out_rgb, hipStream_t st) {
  typedef typename T::elem E;
  const int C = cfg->cin, R = cfg->res, F = cfg->n_frames, sdim = cfg->style_dim, Rp = R / 2;
  UnitCtx u;
  const DecTune tn = DecTune::from_env();
  int rc;
  Level L;
  std::vector<float> wm_rows, bm_host;
  if ((rc = pack_level(&u.pool, tt, "to_flow", "to_rgb", R, C, &L, &wm_rows, &bm_host, sdim))) return rc;
  StyleTable t;
  if ((rc = unit_style_table(&u, wm_rows, bm_host, sdim, F, 0, &t))) return rc;
  launch_style_gemm(t, style, nullptr, sdim, F, st);
  float *ones, *pf = nullptr, *pr = nullptr, *fo, *ro;
  if ((rc = upload32(&u.pool, std::vector<float>((size_t)F * C, 1.0f), &ones))) return rc;
  E *X, *Ft, *XN;
  unsigned long long* sat;
  if ((rc = u.pool.alloc(&sat, 1, true))) return rc;
  if ((rc = u.pool.alloc(&X, (size_t)F * R * R * C, true)) || (rc = u.pool.alloc(&XN, (size_t)F * R * R * C, true))) return rc;
  if ((rc = u.pool.alloc(&Ft, (size_t)R * R * C, true))) return rc;
  if ((rc = u.pool.alloc(&fo, (size_t)F * R * R * 4, true)) || (rc = u.pool.alloc(&ro, (size_t)F * R * R * 4, true))) return rc;
  const size_t nx = (size_t)F * R * R * C;
  hipLaunchKernelGGL((dec_dbg_pack_kernel<T>), dim3((unsigned)((nx / 4 + 255) / 256)), dim3(256), 0, st, X, x, (const float*)nullptr, 0, F,
                     C, R * R, sat);
  hipLaunchKernelGGL((dec_dbg_pack_kernel<T>), dim3((unsigned)(((size_t)R * R * C / 4 + 255) / 256)), dim3(256), 0, st, Ft, feat,
                     (const float*)nullptr, 0, 1, C, R * R, sat);
  if (prev_flow) {
    if ((rc = u.pool.alloc(&pf, (size_t)F * Rp * Rp * 4, true))) return rc;
    hipLaunchKernelGGL(dec_dbg_pyr_kernel, dim3((F * Rp * Rp + 255) / 256), dim3(256), 0, st, pf, prev_flow, F, Rp * Rp, 0);
  }
  if (prev_rgb) {
    if ((rc = u.pool.alloc(&pr, (size_t)F * Rp * Rp * 4, true))) return rc;
    hipLaunchKernelGGL(dec_dbg_pyr_kernel, dim3((F * Rp * Rp + 255) / 256), dim3(256), 0, st, pr, prev_rgb, F, Rp * Rp, 0);
  }
  if ((rc = u.pool.alloc(&L.grgb, (size_t)R * R * 4, true))) return rc;
  hipLaunchKernelGGL((dec_feat_rgb_kernel<T>), dim3((R * R + 255) / 256), dim3(256), 0, st, L.grgb, Ft, L.wrgb, C, R * R);
  L.feat = Ft;
  FlowArgs g = flow_args_of(L, t.styles, C, F);
  g.x = X;
  g.pflow = pf;
  g.prgb = pr;
  g.snext = ones;
  g.xnext = XN;
  g.flow_out = fo;
  g.rgb_out = ro;
  g.write_pyr = 1;
  g.sat = sat;
  if ((rc = launch_flow<T>(DecLaunch{tn, nullptr, st}, g))) return rc;
  if (out_flow) hipLaunchKernelGGL(dec_dbg_pyr_kernel, dim3((F * R * R + 255) / 256), dim3(256), 0, st, out_flow, fo, F, R * R, 1);
  if (out_rgb) hipLaunchKernelGGL(dec_dbg_pyr_kernel, dim3((F * R * R + 255) / 256), dim3(256), 0, st, out_rgb, ro, F, R * R, 1);
  if (out_blend)
    hipLaunchKernelGGL((dec_dbg_unpack_kernel<T>), dim3((unsigned)((nx + 255) / 256)), dim3(256), 0, st, out_blend, XN, F, C, R * R);
  FH_CHECK_HIP(hipGetLastError());
  FH_CHECK_HIP(hipStreamSynchronize(st));
  return FLOAT_OK;
}

}  // namespace

extern "C" {

int float_dec_create(const float_dec_cfg_t* cfg, const float_tensor_t* tensors, int32_t n_tensors, float_dec_t** out) {
  FH_REQUIRE(cfg && tensors && out, "null argument to float_dec_create");
  FH_REQUIRE(cfg->size >= 64 && cfg->size <= 512 && (cfg->size & (cfg->size - 1)) == 0,
             "decoder size must be a power of two in [64, 512] (got %d)", cfg->size);
  FH_REQUIRE(cfg->style_dim > 0 && cfg->style_dim <= 2048, "style_dim %d unsupported", cfg->style_dim);
  FH_REQUIRE(cfg->max_frames >= 1 && cfg->max_frames <= 128, "max_frames must be in [1,128] (got %d)", cfg->max_frames);
  // fp16 operands in production: with bf16 the 512-px frames sat at the 40 dB limit (40.7 dB, max |d| 0.15 on a [0,1] pixel: the
  // flow field positions the bilinear sampling, 8 mantissa bits are too few there); fp16 runs at the same MFMA rate.
  // FLOAT_DT_FP32 is the verification mode: the same launch chain with fp32 activations and weights (1/16 of the MFMA rate).
  FH_REQUIRE(cfg->dtype == FLOAT_DT_FP16 || cfg->dtype == FLOAT_DT_FP32,
             "the decoder supports FLOAT_DT_FP16 operands (and FLOAT_DT_FP32 for verification) only (got dtype %d)", cfg->dtype);
  float_dec* h = new float_dec();
  h->tune = DecTune::from_env();
  h->cfg = *cfg;
  TensorTable tt(tensors, n_tensors);
  int rc = DEC_DISPATCH(cfg->dtype, create_impl<T>(h, tt));
  if (!rc) {
    if (const float_tensor_t* dw = tt.find("direction.weight")) {
      if (dw->ndim == 2 && dw->shape[0] == cfg->style_dim) {
        std::vector<float> Q;
        h->motion_dim = (int)dw->shape[1];
        fh_direction_q(dw->data, cfg->style_dim, h->motion_dim, &Q);
        rc = h->pool.alloc(&h->dirQ, Q.size(), false);
        if (!rc && hipMemcpy(h->dirQ, Q.data(), Q.size() * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) rc = FLOAT_E_HIP;
      }
    }
  }
  if (rc) {
    float_dec_destroy(h);
    return rc;
  }
  *out = h;
  return FLOAT_OK;
}

int float_dec_direction(float_dec_t* h, const float* lam, float* r_s, void* stream) {
  FH_REQUIRE(h && lam && r_s, "null argument to float_dec_direction");
  FH_REQUIRE(h->dirQ != nullptr, "the decoder checkpoint has no (style_dim, motion_dim) 'direction.weight'");
  return fh_linear_f32(lam, h->dirQ, nullptr, 1.0f, r_s, h->cfg.style_dim, h->motion_dim, (hipStream_t)stream);
}

void float_dec_destroy(float_dec_t* h) {
  if (!h) return;
  for (hipEvent_t e : h->copy_events) (void)hipEventDestroy(e);
  if (h->join_event) (void)hipEventDestroy(h->join_event);
  h->pool.release();
  delete h;
}

int float_dec_set_feats(float_dec_t* h, const float* const* feats, int32_t n_feats, void* stream) {
  FH_REQUIRE(h && feats, "null argument to float_dec_set_feats");
  FH_REQUIRE(n_feats == h->n_levels, "expected %d feature maps (8..%d), got %d", h->n_levels, h->cfg.size, n_feats);
  for (int i = 0; i < n_feats; ++i) FH_REQUIRE(feats[i] != nullptr, "feats[%d] is null", i);
  hipStream_t st = (hipStream_t)stream;
  int rc = DEC_DISPATCH(h->cfg.dtype, set_feats_impl<T>(h, feats, st));
  if (!rc) h->feats_set = true;
  return rc;
}

int float_dec_set_feats16(float_dec_t* h, const void* const* feats16, int32_t n_feats, int32_t dtype, void* stream) {
  FH_REQUIRE(h && feats16, "null argument to float_dec_set_feats16");
  FH_REQUIRE(n_feats == h->n_levels, "expected %d feature maps (8..%d), got %d", h->n_levels, h->cfg.size, n_feats);
  FH_REQUIRE(dtype == h->cfg.dtype, "feature dtype %d differs from the decoder's (%d)", dtype, h->cfg.dtype);
  for (int i = 0; i < n_feats; ++i) FH_REQUIRE(feats16[i] != nullptr, "feats16[%d] is null", i);
  hipStream_t st = (hipStream_t)stream;
  const size_t eb = dtype == FLOAT_DT_FP32 ? 4 : 2;
  for (int li = 0; li < h->n_levels; ++li) {
    const Level& L = h->levels[li];
    int rc = fh_copy_d2d(L.feat, feats16[li], (size_t)L.R * L.R * L.C * eb, st);
    if (rc) return rc;
  }
  int rc = DEC_DISPATCH(h->cfg.dtype, feats_rgb_impl<T>(h, st));
  if (rc) return rc;
  h->feats_set = true;
  return FLOAT_OK;
}

// What every float_dec_frames* entry point `fn` checks before it decodes (`ptrs`: its pointer arguments are all there)
static int dec_check_run(float_dec_t* h, bool ptrs, int32_t n_frames, const void* out, DecOut mode, const char* fn) {
  const char* sfx = mode == kOutU8 ? "_u8" : mode == kOutI420 ? "_i420" : "";
  FH_REQUIRE(h && ptrs, "null argument to %s%s", fn, sfx);
  FH_REQUIRE(h->feats_set, "float_dec_set_feats must be called before decoding");
  FH_REQUIRE(n_frames >= 1, "n_frames must be >= 1 (got %d)", n_frames);
  FH_REQUIRE((mode != kOutU8 && mode != kOutI420) || (uintptr_t)out % 4 == 0,
             "%s%s: the output must be 4-byte aligned (the last-level kernel stores dwords)", fn, sfx);
  return FLOAT_OK;
}

static int dec_run(float_dec_t* h, const float* s_r, const float* r_d, int32_t n_frames, void* out, DecOut mode, void* stream) {
  if (int rc = dec_check_run(h, s_r && r_d && out, n_frames, out, mode, "float_dec_frames")) return rc;
  hipStream_t st = (hipStream_t)stream;
  return DEC_DISPATCH(h->cfg.dtype, frames_impl<T>(h, s_r, r_d, n_frames, out, mode, st));
}

int float_dec_frames(float_dec_t* h, const float* s_r, const float* r_d, int32_t n_frames, float* out_hwc, void* stream) {
  return dec_run(h, s_r, r_d, n_frames, out_hwc, kOutHWC, stream);
}

// float_dec_frames_host (float) and float_dec_frames_host_u8 (uint8_t)
static int dec_run_host(float_dec_t* h, const float* s_r, const float* r_d, int32_t n_frames, void* out_hwc, void* host_hwc, DecOut mode,
                        void* stream, void* copy_stream) {
  if (int rc = dec_check_run(h, s_r && r_d && out_hwc && host_hwc, n_frames, out_hwc, mode, "float_dec_frames_host")) return rc;
  hipStream_t st = (hipStream_t)stream, cs = copy_stream ? (hipStream_t)copy_stream : st;
  // Is host_hwc memory a kernel may store through?  Only pinned (hipHostMalloc) or registered (hipHostRegister) host memory
  // has a device-side address; for anything else - pageable memory - the frames go by hipMemcpyAsync behind each batch.
  void* host_dev = nullptr;
  {
    hipPointerAttribute_t at;
    memset(&at, 0, sizeof(at));
    if (hipPointerGetAttributes(&at, host_hwc) == hipSuccess && at.type == hipMemoryTypeHost && at.devicePointer)
      host_dev = at.devicePointer;
    else
      (void)hipGetLastError();  // "invalid value" for pageable memory: not an error of this call
  }
  return DEC_DISPATCH(h->cfg.dtype, frames_impl<T>(h, s_r, r_d, n_frames, out_hwc, mode, st, host_hwc, cs, host_dev));
}

int float_dec_frames_host(float_dec_t* h, const float* s_r, const float* r_d, int32_t n_frames, float* out_hwc, float* host_hwc,
                          void* stream, void* copy_stream) {
  return dec_run_host(h, s_r, r_d, n_frames, out_hwc, host_hwc, kOutHWC, stream, copy_stream);
}

int float_dec_frames_u8(float_dec_t* h, const float* s_r, const float* r_d, int32_t n_frames, uint8_t* out_hwc, void* stream) {
  return dec_run(h, s_r, r_d, n_frames, out_hwc, kOutU8, stream);
}

int float_dec_frames_host_u8(float_dec_t* h, const float* s_r, const float* r_d, int32_t n_frames, uint8_t* out_hwc, uint8_t* host_hwc,
                             void* stream, void* copy_stream) {
  return dec_run_host(h, s_r, r_d, n_frames, out_hwc, host_hwc, kOutU8, stream, copy_stream);
}

// The colour matrix of the I420 calls (common.hpp: kFhYuvRows; 0 / 2 / 4 / 6 = BT.601 / BT.709, limited / full range): an unknown
// id is refused before anything else is looked at.  The table rides in the kernels' arguments (FlowArgs::yuv, and the converter's
// last argument), six dwords that the scalar unit unpacks - not a template parameter: dec_flowlast_kernel's I420 instantiation
// stays one per operand type at 56 VGPRs (64 -> 70 SGPRs), dec_rgb8_to_i420_kernel at 50 (51).  MI355X, yuvbench.py --matrix 6
// (20 interleaved repetitions): decode + hand-over of 250 frames 20.13 (id 0) / 20.07 ms (id 6) fused and 20.28 / 20.27 ms through
// the converter, against 20.08 and 20.25 ms for the constants in the instructions (the commit before; spreads 0.07 ... 0.26 ms).
#define DEC_REQUIRE_MATRIX(fn, matrix, t) \
  FH_REQUIRE(fh_yuv_of((matrix), &(t)), fn ": matrix %d unknown (" FH_YUV_IDS ")", (int)(matrix))

int float_dec_frames_i420(float_dec_t* h, const float* s_r, const float* r_d, int32_t n_frames, int32_t matrix, uint8_t* out,
                          void* stream) {
  FhYuv t;
  FH_REQUIRE(h && s_r && r_d && out, "null argument to float_dec_frames_i420");
  DEC_REQUIRE_MATRIX("float_dec_frames_i420", matrix, t);
  h->yuv = t;
  return dec_run(h, s_r, r_d, n_frames, out, kOutI420, stream);
}

int float_dec_frames_host_i420(float_dec_t* h, const float* s_r, const float* r_d, int32_t n_frames, int32_t matrix, uint8_t* out,
                               uint8_t* host, void* stream, void* copy_stream) {
  FhYuv t;
  FH_REQUIRE(h && s_r && r_d && out && host, "null argument to float_dec_frames_host_i420");
  DEC_REQUIRE_MATRIX("float_dec_frames_host_i420", matrix, t);
  h->yuv = t;
  return dec_run_host(h, s_r, r_d, n_frames, out, host, kOutI420, stream, copy_stream);
}

int float_dec_saturation(float_dec_t* h, uint64_t* total, uint64_t* per_site, int32_t reset, void* stream) {
  FH_REQUIRE(h && total, "null argument to float_dec_saturation");
  hipStream_t st = (hipStream_t)stream;
  unsigned long long host[kDecSatSites];
  FH_CHECK_HIP(hipStreamSynchronize(st));
  FH_CHECK_HIP(hipMemcpy(host, h->sat, sizeof(host), hipMemcpyDeviceToHost));
  uint64_t sum = 0;
  for (int i = 0; i < kDecSatSites; ++i) {
    sum += host[i];
    if (per_site) per_site[i] = host[i];
  }
  *total = sum;
  if (reset) {  // on the caller's stream: ordered against the launches that add to the counters there
    FH_CHECK_HIP(hipMemsetAsync(h->sat, 0, sizeof(host), st));
    FH_CHECK_HIP(hipStreamSynchronize(st));
  }
  return FLOAT_OK;
}

int float_dec_debug_styled_conv(const float_dec_unit_t* u, const float_tensor_t* tensors, int32_t n_tensors, const float* x,
                                const float* style, float* out, uint64_t* saturated, void* stream) {
  FH_REQUIRE(u && tensors && x && style && out, "null argument to float_dec_debug_styled_conv");
  FH_REQUIRE(u->dtype == FLOAT_DT_FP16 || u->dtype == FLOAT_DT_FP32, "unit op: dtype %d unsupported", u->dtype);
  FH_REQUIRE(u->cin % 32 == 0 && u->cout % 32 == 0 && u->cin > 0 && u->cout > 0, "unit op: channels must be multiples of 32");
  FH_REQUIRE(u->res >= 4 && (u->res & (u->res - 1)) == 0 && u->res <= 512, "unit op: resolution must be a power of two in [4, 512]");
  FH_REQUIRE(u->n_frames >= 1 && u->style_dim >= 1 && u->style_dim <= 2048, "unit op: bad batch / style_dim");
  TensorTable tt(tensors, n_tensors);
  return DEC_DISPATCH(u->dtype, unit_styled_conv<T>(u, tt, x, style, out, saturated, (u->flags & 1) ? 0 : 1, (hipStream_t)stream));
}

int float_dec_debug_flow_level(const float_dec_unit_t* u, const float_tensor_t* tensors, int32_t n_tensors, const float* x,
                               const float* feat, const float* style, const float* prev_flow, const float* prev_rgb, float* out_flow,
                               float* out_blend, float* out_rgb, void* stream) {
  FH_REQUIRE(u && tensors && x && feat && style, "null argument to float_dec_debug_flow_level");
  FH_REQUIRE(u->dtype == FLOAT_DT_FP16 || u->dtype == FLOAT_DT_FP32, "unit op: dtype %d unsupported", u->dtype);
  FH_REQUIRE(u->cin >= 32 && u->cin <= 512 && (u->cin & (u->cin - 1)) == 0, "unit op: channels must be a power of two in [32, 512]");
  FH_REQUIRE(u->res >= 8 && (u->res & (u->res - 1)) == 0 && u->res <= 512, "unit op: resolution must be a power of two in [8, 512]");
  FH_REQUIRE(u->n_frames >= 1 && u->style_dim >= 1 && u->style_dim <= 2048, "unit op: bad batch / style_dim");
  TensorTable tt(tensors, n_tensors);
  return DEC_DISPATCH(u->dtype, unit_flow_level<T>(u, tt, x, feat, style, prev_flow, prev_rgb, out_flow, out_blend, out_rgb, (hipStream_t)stream));
}

#ifdef DEC_PHASES
int float_dec_debug_phases(unsigned long long* out16, int reset) {
  static unsigned long long all[64 * 16];
  FH_CHECK_HIP(hipDeviceSynchronize());
  FH_CHECK_HIP(hipMemcpyFromSymbol(all, HIP_SYMBOL(g_dec_phase), sizeof(all)));
  for (int i = 0; i < 16; ++i) {
    out16[i] = 0;
    for (int r = 0; r < 64; ++r) out16[i] += all[r * 16 + i];
  }
  if (reset) {
    memset(all, 0, sizeof(all));
    FH_CHECK_HIP(hipMemcpyToSymbol(HIP_SYMBOL(g_dec_phase), all, sizeof(all)));
  }
  return FLOAT_OK;
}
#endif

#ifdef DEC_STAMPS
int float_dec_debug_stamps(unsigned long long* out4) {
  FH_CHECK_HIP(hipDeviceSynchronize());
  FH_CHECK_HIP(hipMemcpyFromSymbol(out4, HIP_SYMBOL(g_dec_stamps), 4 * sizeof(unsigned long long)));
  return FLOAT_OK;
}
#endif

int float_dec_feat_shape(float_dec_t* h, int32_t i, int32_t* channels, int32_t* resolution) {
  FH_REQUIRE(h && channels && resolution, "null argument to float_dec_feat_shape");
  FH_REQUIRE(i >= 0 && i < h->n_levels, "feature index %d out of range (the decoder takes %d maps)", i, h->n_levels);
  *channels = h->levels[i].C;
  *resolution = h->levels[i].R;
  return FLOAT_OK;
}

int float_dec_frames_raw(float_dec_t* h, const float* s_r, const float* r_d, int32_t n_frames, float* out_chw, void* stream) {
  return dec_run(h, s_r, r_d, n_frames, out_chw, kOutRawCHW, stream);
}

}  // extern "C"
