// C-ABI entry points of the FMT operator (include/float_hip.h): the handle, the evaluation chain and its hipGraph cache, the
// incremental sampler and the GEMM service.  Packing and launchers: fmt_weights.hpp, fmt_launch.hpp.
#include <math.h>
#include <stdlib.h>

#include "fmt_gemm.hpp"
#include "fmt_kernels.hpp"
#include "fmt_rb_kernels.hpp"
#include "fmt_big_kernels.hpp"
#include "fmt_launch.hpp"

namespace {

struct Blk {
  Lin qkv, proj, fc1, fc2;
};

constexpr int kMaxTok = 80;      // tokens per window (n_prev + n_cur); the workspace is sized for a 4-way CFG batch of them (320 rows)
constexpr int kMaxSteps = 1024;  // FloatAdvancedParameters.nfe max is 1000 (nodes_adv.py:184-190)

}  // namespace

struct float_fmt {
  float_fmt_cfg_t cfg;
  DevicePool pool;
  int D, ntok, Mpad, Kc, Ntot, Kx;
  int Bmax = 1;  // clips per launch chain the workspace is sized for (float_fmt_cfg_t::max_batch)
  Lin x_embed, t0, t2, c_embed, adaln_all, final_lin;
  std::vector<Blk> blk;
  float* pos = nullptr;
  float* freqs = nullptr;
  // workspace
  u16 *cond16, *sc16, *h16, *hfin16, *qkv16, *att16, *hid16, *xin16, *tsin16, *th16;
  float *ccond, *xres, *xcur, *temb, *vout;
  unsigned long long* sat = nullptr;  // range counter of every 16-bit activation store of the handle's launches (float_fmt_saturation)
  float* slab = nullptr;  // [8][Mpad][D] split-K partial sums (EPI_PARTIAL)
  float *wa_c, *we_c, *prev_x, *prev_wa, *prev_we, *x0_c;
  float* wr_c = nullptr;   // [clip][dim_w]: wr of a ragged job in slot order
  int method = 0;          // FLOAT_ODE_*
  FmtTune tune;            // the environment's switches as float_fmt_create found them (tuning.hpp)
  int n_cu = 0;            // compute units of the device (big_shape_ok, launch_big4)
  float* kbuf = nullptr;   // [4][kMaxTok][dim_w] stage velocities of the Runge-Kutta solvers
  // Modulations of up to kScSteps evaluations of a window, [step][Mmod][Ntot] fp32: c = t_emb + c_embedder(wr, wa, we) does not
  // depend on x (FMT.py:333-335, 163-166), so every adaLN projection of those evaluations is ONE GEMM per window.
  float* modall = nullptr;
  int Mmod = 0;
  size_t mod_zs = 0;  // floats between two evaluations' modulations in modall, as the last run_mod_all laid them out
  // hipGraph cache for the per-window chain: one entry per chain SETTING (nfe, bc, we_len, method, scales, priority), least
  // recently used setting evicted; an entry holds one executable per stack height (clips in the chain) it has met, so the
  // shrinking stack of a ragged job stays inside its entry and never evicts
  struct GraphKey {
    int nfe, bc, we_len, method;
    int prio;  // priority of the stream the graph is launched on (run_mod_all picks its kernel by it)
    float a, r, e;
    bool operator==(const GraphKey& o) const { return memcmp(this, &o, sizeof(GraphKey)) == 0; }
  };
  struct GraphEntry {
    GraphKey key;
    hipGraphExec_t exec[kFmtMaxClips + 1];  // by nclip; nullptr = not captured yet
    uint64_t used;
  };
  std::vector<GraphEntry> graphs;
  uint64_t graph_clock = 0;
  hipStream_t cap_stream = nullptr;
  int cap_prio = 0;  // while capturing: the priority of the stream the graph will be launched on
  // state of an incremental sample (float_fmt_sample_begin / _next)
  struct {
    const float *wr, *wa, *we, *noise;
    float* r_d;
    int T, we_len, nfe, include_r, next, n_chunks, B;
    int first = 0, total = 0;                                  // first window of the job / windows of the whole clip
    const float *hist_x = nullptr, *hist_wa = nullptr, *hist_we = nullptr;  // history of window `first` (nullptr: zeros)
    float a, r, e;
    std::vector<float> ts;
    bool active = false;
    // ragged job (float_fmt_sample_begin_ragged): per-clip pointers and lengths in SLOT order - window count descending,
    // stable - so that the clips active in window k are the first n_active(k) slots
    bool ragged = false;
    FmtClipTab<const float*> rg_wr, rg_wa, rg_we, rg_noise;
    FmtClipTab<float*> rg_rd;
    int rg_win[kFmtMaxClips];  // windows per slot, non-increasing
  } job;
};

namespace {

// Stream-ordered device copies as kernel launches (see fmt_copy_kernel: memcpy / memset nodes of a caller's capture did not
// replay reproducibly).
int dev_copy2d(float* dst, size_t dpitch, const float* src, size_t spitch, int width, int rows, hipStream_t s) {
  if (width <= 0 || rows <= 0) return FLOAT_OK;
  hipLaunchKernelGGL(fmt_copy_kernel, dim3((unsigned)(((size_t)rows * width + 255) / 256)), dim3(256), 0, s, dst, dpitch, src, spitch, width, rows);
  FH_CHECK_HIP(hipGetLastError());
  return FLOAT_OK;
}
int dev_copy(float* dst, const float* src, size_t n, hipStream_t s) { return dev_copy2d(dst, n, src, n, (int)n, 1, s); }
int dev_zero(float* dst, size_t n, hipStream_t s) { return dev_copy2d(dst, n, nullptr, n, (int)n, 1, s); }
int copy_or_zero(float* dst, const float* src, size_t n, hipStream_t s) { return src ? dev_copy(dst, src, n, s) : dev_zero(dst, n, s); }

// What the launchers of fmt_launch.hpp see of the handle, for launches on stream `s`
FmtLaunch launch_ctx(const float_fmt* h, hipStream_t s) {
  return FmtLaunch{h->tune, s, h->sat, h->xres, h->slab, h->h16, h->qkv16, h->att16, h->D, h->ntok, h->Ntot, h->Mpad, h->cfg.heads,
                   h->cfg.attn_window};
}


// Modulation half of the evaluations [e0, e0 + n) of a window: depends only on t and the window's conditions, NOT on x
// (c = t_emb + c_embedder([wr, wa, we]), FMT.py:333-335; adaLN_modulation = Linear(SiLU(c)), FMT.py:163-166, 187-190), so it is
// taken out of the Euler step:
//   sc[z]     = silu(t_emb[e0 + z] + c_cond)                          one launch, blockIdx.y = z
//   modall[z] = sc[z] @ W_adaLN_all^T + b   (Mmod x Ntot fp32 per z)  ONE GEMM launch of n row batches against the 105 MB of
//                                                                     weights (every block's adaLN projection + the head's)
// The step chain then reads its 37 MB slab and no longer streams those weights, which leaves the 208 MB of block weights
// alone in the 256 MB Infinity Cache.  FLOAT_FMT_HOIST=0 launches the same kernel once per evaluation (n = 1) instead
// (bitwise the same numbers; the A/B switch of the measurement).
constexpr int kScSteps = 64;  // evaluations per modulation batch; longer grids run in batches of this many

static int stream_priority(hipStream_t s) {
  int prio = 0;
  if (hipStreamGetPriority(s, &prio) != hipSuccess) {
    (void)hipGetLastError();
    prio = 0;
  }
  return prio;
}

template <class T>
int run_mod_all(float_fmt* h, int M, int e0, int n, hipStream_t s) {
  const int D = h->D;
  const FmtTune& tn = h->tune;
  FH_REQUIRE(n >= 1 && n <= kScSteps, "modulation batch of %d evaluations (max %d)", n, kScSteps);
  // dense rows for the persistent kernel (row z * M + r of one packed image), else one padded image per evaluation
  // Not on a stream of non-default priority: with the chain on a HIGH-priority stream beside a decoder on a second stream
  // (FLOAT_AMD_OVERLAP=prio) every window after the first came out wrong, and only with this kernel in the chain (round 6:
  // tools/probes/overlap_check.py; the kernel alone passes the same stress in tools/probes/gemm_big_lab.hip, cause not found -
  // DESIGN.md section 7).  fmt_gemm_dma_kernel gives the same numbers bit for bit.
  const int prio = (s == h->cap_stream && s) ? h->cap_prio : stream_priority(s);
  const bool big = !T::is32 && tn.wide && prio == 0 && big_shape_ok(tn, n * M, h->adaln_all.N, h->adaln_all.K, h->n_cu);
  hipLaunchKernelGGL((fmt_silu_c_kernel<T>), dim3((M * D / 8 + 255) / 256, n), dim3(256), 0, s, h->sc16, h->temb + (size_t)e0 * D,
                     h->ccond, M, D, (size_t)h->Mpad * D, big ? M : 0, h->sat);
  h->mod_zs = big ? (size_t)M * h->Ntot : (size_t)h->Mmod * h->Ntot;
  if constexpr (!T::is32) {
    if (big) return launch_big4<T>(h->sc16, h->adaln_all, h->modall, n * M, h->Ntot, h->n_cu, s);
  }
  GemmArgs g = base_args(h->sc16, h->adaln_all, M);
  g.sat = h->sat, g.out_f32 = h->modall, g.ldo = h->Ntot, g.zcount = n;
  const bool dma = (tn.wide_variant == 6 || tn.wide_variant == 7) && (M + 15) / 16 > 4 && dma_shape_ok(g, 320);
  g.zgroup = tn.zgroup > 0 ? tn.zgroup : (dma ? 2 : 4);
  g.a_zstride = (size_t)h->Mpad * D;
  g.o_zstride = (size_t)h->Mmod * h->Ntot;
  if constexpr (!T::is32) {
    if (tn.wide && g.N % 128 == 0 && g.K % 128 == 0) return launch_wide<T>(g, tn.wide_variant, s);
  }
  for (int z = 0; z < n; ++z) {  // shapes the wide kernel does not tile: the generic GEMM, one batch at a time
    GemmArgs gz = g;
    gz.A = g.A + (size_t)z * g.a_zstride * (sizeof(typename T::elem) / sizeof(u16));
    gz.out_f32 = g.out_f32 + (size_t)z * g.o_zstride;
    gz.zcount = 0;
    int rc = run_gemm<T, EPI_F32>(tn, gz, s);
    if (rc) return rc;
  }
  return FLOAT_OK;
}

bool split_ok(int ks, const Lin& L) { return (ks == 1 || ks == 2 || ks == 4) && L.K % (128 * ks) == 0; }

// Attention, then attn.proj of block B on the M rows of qkv16, by the first that applies: the row-blocked tile (stacked clips),
// a split-K proj, the proj GEMM with gate * residual in its epilogue.  *pend: the reduction left to LN2 by the first two
// (`gate` = gate_msa).
template <class T>
int run_proj(const FmtLaunch& cx, const Blk& B, int M, const float* gate, const RbPlan& rb, PendingRed* pend) {
  const FmtTune& tn = cx.tn;
  const int ks = rb.shape >= 0 ? rb.ksplit : (split_ok(tn.proj_split, B.proj) ? tn.proj_split : 0);
  int rc;
  launch_attn<T>(cx, M, (!ks && (tn.touch & 2)) ? &B.proj : nullptr);
  GemmArgs g = base_args(cx.att16, B.proj, M);
  if (rb.shape >= 0) {
    to_slab(g, cx.slab, cx.Mpad, ks);
    rc = launch_rbs<T, EPI_PARTIAL>(g, rb.shape, cx.s);
  } else if (ks) {
    rc = run_gemm_partial<T>(cx, g, ks);
  } else {
    g.sat = cx.sat, g.out_f32 = cx.xres, g.ldo = cx.D;
    g.gate = gate, g.ldg = cx.Ntot;
    if (tn.touch & 16) g.touch = make_touch(tn, B.fc1, M, 0, gemm_lanes_per_xcd(tn, M, g.N, g.K), 2);
    rc = run_gemm<T, EPI_GATE_RES>(tn, g, cx.s, false, &tn.plan_layer[RB_PROJ]);
  }
  if (!rc && ks) *pend = pending_red(cx.slab, cx.Mpad, cx.D, B.proj.b, gate, ks);
  return rc;
}

// mlp.fc2 of block B on the M rows of hid16, likewise: the row-blocked tile, a split-K GEMM (whose workgroups touch the weights
// of `after`, the GEMM behind the next LayerNorm, under touch bit 32), or gate * residual in the epilogue (`gate` = gate_mlp).
template <class T>
int run_fc2(const FmtLaunch& cx, const Blk& B, const u16* hid16, int M, const float* gate, const RbPlan& rb, const Lin& after,
            int after_nt, PendingRed* pend) {
  const FmtTune& tn = cx.tn;
  const int ks = rb.shape >= 0 ? rb.ksplit : (split_ok(tn.fc2_split, B.fc2) ? tn.fc2_split : 0);
  GemmArgs g = base_args(hid16, B.fc2, M);
  int rc;
  if (rb.shape >= 0) {
    to_slab(g, cx.slab, cx.Mpad, ks);
    rc = launch_rbs<T, EPI_PARTIAL>(g, rb.shape, cx.s);
  } else if (ks) {
    g.sat = cx.sat;
    if (tn.touch & 32) g.touch = make_touch(tn, after, M, 0, gemm_lanes_per_xcd(tn, M, g.N * ks, g.K / ks), 2, after_nt);
    rc = run_gemm_partial<T>(cx, g, ks, &tn.plan_layer[RB_FC2]);
  } else {
    g.sat = cx.sat, g.out_f32 = cx.xres, g.ldo = cx.D;
    g.gate = gate, g.ldg = cx.Ntot;
    rc = run_gemm<T, EPI_GATE_RES>(tn, g, cx.s);
  }
  if (!rc && ks) *pend = pending_red(cx.slab, cx.Mpad, cx.D, B.fc2.b, gate, ks);
  return rc;
}

// Block chain of an evaluation on the rows staged in the workspace, using the modulations in modbuf.
// euler: update xcur/xin16 with dt, else write vout.
template <class T>
int run_blocks(float_fmt* h, int nclip, int bc, const float* modbuf, bool euler, float dt, float a, float r, float e, hipStream_t s,
               float* vout_to = nullptr) {
  const float_fmt_cfg_t& c = h->cfg;
  const FmtTune& tn = h->tune;
  const FmtLaunch cx = launch_ctx(h, s);
  const int D = h->D, ntok = h->ntok, M = nclip * bc * ntok;
  int rc;
  // x_embedder + pos_embed; the CFG rows share x, so 60 rows are computed and broadcast
  {
    GemmArgs g = base_args(h->xin16, h->x_embed, nclip * ntok);
    g.sat = h->sat, g.out_f32 = h->xres, g.ldo = D;
    g.pos = h->pos, g.bc = bc, g.ntok = ntok;
    if ((rc = run_gemm<T, EPI_XEMBED>(tn, g, s))) return rc;
  }
  PendingRed pend;  // residual update left to the next LayerNorm launch
  // stacked clips: the row-blocked LDS-DMA tile (fmt_rb_kernels.hpp); its launches carry no touch descriptors; the LayerNorm in
  // front of qkv / fc1 pulls the first stages of their weights into the XCDs' L2s (make_touch_rb)
  RbPlan rb_qkv, rb_proj, rb_fc1, rb_fc2;
  if constexpr (!T::is32) {
    rb_qkv = pick_rb(tn, RB_QKV, M), rb_proj = pick_rb(tn, RB_PROJ, M), rb_fc1 = pick_rb(tn, RB_FC1, M), rb_fc2 = pick_rb(tn, RB_FC2, M);
  }
  for (int b = 0; b < c.depth; ++b) {
    const float* mod = modbuf + (size_t)b * 6 * D;  // shift_msa, scale_msa, gate_msa, shift_mlp, scale_mlp, gate_mlp
    const Blk& B = h->blk[b];
    const bool last = b + 1 == c.depth;
    if ((rc = launch_lnmod<T>(cx, M, mod, mod + D, &pend, &B.qkv, nullptr, 0, 128, rb_qkv.shape))) return rc;
    {
      GemmArgs g = base_args(h->h16, B.qkv, M);
      g.sat = h->sat, g.out16 = h->qkv16, g.ldo16 = 3 * D;
      if ((tn.touch & 8) && !split_ok(tn.proj_split, B.proj)) g.touch = make_touch(tn, B.proj, M, 0, gemm_lanes_per_xcd(tn, M, g.N, g.K), 2);
      if (rb_qkv.shape >= 0) rc = launch_rbs<T, EPI_T16>(g, rb_qkv.shape, s);
      else rc = run_gemm<T, EPI_T16>(tn, g, s, false, &tn.plan_layer[RB_QKV]);
      if (rc) return rc;
    }
    if ((rc = run_proj<T>(cx, B, M, mod + 2 * D, rb_proj, &pend))) return rc;
    if ((rc = launch_lnmod<T>(cx, M, mod + 3 * D, mod + 4 * D, &pend, &B.fc1, nullptr, 0, 64, rb_fc1.shape))) return rc;
    {
      GemmArgs g = base_args(h->h16, B.fc1, M);
      g.sat = h->sat, g.out16 = h->hid16, g.ldo16 = B.fc2.K / 32;  // packed for fc2
      if ((tn.touch & 4) && rb_fc2.shape < 0)
        g.touch = make_touch(tn, B.fc2, M, split_ok(tn.fc2_split, B.fc2) ? tn.fc2_split : 0, gemm_lanes_per_xcd(tn, M, g.N, g.K), 2);
      if (rb_fc1.shape >= 0) rc = launch_rbs<T, EPI_GELU_P16>(g, rb_fc1.shape, s);
      else rc = run_gemm<T, EPI_GELU_P16>(tn, g, s, false, &tn.plan_layer[RB_FC1]);
      if (rc) return rc;
    }
    // fc2's workgroups touch the next block's qkv, or the head GEMM (which runs 16-column workgroups)
    if ((rc = run_fc2<T>(cx, B, h->hid16, M, mod + 5 * D, rb_fc2, last ? h->final_lin : h->blk[b + 1].qkv, last ? 1 : 0, &pend))) return rc;
  }
  {
    const float* mod = modbuf + (size_t)c.depth * 6 * D;  // shift, scale (FMT.py:196)
    // head: token-blocked rows (every CFG row of 16 tokens in one workgroup: 4 x 32 workgroups of bc row tiles) unless the
    // CFG batch is not one of the combine's shapes; then all rows per workgroup (32 workgroups)
    const bool tokblk = (!tn.no_tokblk || nclip > 1) && (bc == 1 || bc == 3 || bc == 4) && h->final_lin.K % 256 == 0;
    FH_REQUIRE(tokblk || nclip == 1, "batched sampling needs the token-blocked head GEMM");
    const int nblk = (ntok + 15) / 16, seqs = nclip * bc;
    if ((rc = launch_lnmod<T>(cx, M, mod, mod + D, &pend, nullptr, tokblk ? h->hfin16 : nullptr, tokblk ? seqs * 16 : 0))) return rc;
    GemmArgs g = base_args(tokblk ? h->hfin16 : h->h16, h->final_lin, tokblk ? nblk * seqs * 16 : M);
    g.sat = h->sat, g.tokblk = tokblk ? 1 : 0;
    g.nclip = nclip, g.bc = bc, g.ntok = ntok, g.n_prev = c.n_prev;
    g.a_cfg = a, g.r_cfg = r, g.e_cfg = e, g.dt = dt;
    if (euler) g.xcur = h->xcur, g.xin16 = h->xin16, g.ldx = h->Kx / 32;
    else g.vout = vout_to ? vout_to : h->vout;
    // token-blocked: a workgroup = the bc row tiles of one (token block, clip) pair; row blocks = token blocks x clips
    if (tokblk) rc = launch_gemm<T, EPI_CFG>(g, bc, 1, 8, s);
    else rc = run_gemm<T, EPI_CFG>(tn, g, s, true);
    if (rc) return rc;
  }
  FH_CHECK_HIP(hipGetLastError());
  return FLOAT_OK;
}

// torch.linspace(0, 1, n) in fp32: symmetric evaluation around the midpoint.
void linspace01(int n, std::vector<float>* ts) {
  ts->resize(n);
  if (n == 1) {
    (*ts)[0] = 0.f;
    return;
  }
  const float step = 1.0f / (float)(n - 1);
  const int half = n / 2;
  for (int i = 0; i < n; ++i) (*ts)[i] = (i < half) ? (0.f + step * (float)i) : (1.0f - step * (float)(n - 1 - i));
}

// t-embedding MLP (FMT.py:128-131) for every evaluation time of a window, rows = evaluations.  The times are formed on the
// device (fmt_tsin_kernel) from (nfe, stage offsets), so no host buffer is read by the stream: the call can be captured.
struct TimeSpec {
  float t;        // nfe == 0: the one explicit time of float_fmt_eval
  int nfe, stages;
  float c[4];     // stage offsets of the Runge-Kutta scheme (Euler: {0})
};
template <class T>
int prepare_time(float_fmt* h, const TimeSpec& ts, int n, hipStream_t s) {
  int rc;
  hipLaunchKernelGGL((fmt_tsin_kernel<T>), dim3(n), dim3(256), 0, s, h->tsin16, h->freqs, n, ts.t, ts.nfe, ts.stages, ts.c[0],
                     ts.c[1], ts.c[2], ts.c[3]);
  GemmArgs g = base_args(h->tsin16, h->t0, n);
  g.sat = h->sat, g.out16 = h->th16, g.ldo16 = h->t2.K / 32;
  if ((rc = launch_gemm<T, EPI_SILU_P16>(g, 4, 1, T::is32 ? 4 : pick_nw(g.K, 0), s))) return rc;
  GemmArgs g2 = base_args(h->th16, h->t2, n);
  g2.sat = h->sat, g2.out_f32 = h->temb, g2.ldo = h->D;
  if ((rc = launch_gemm<T, EPI_F32>(g2, 4, 1, T::is32 ? 4 : pick_nw(g2.K, 0), s))) return rc;
  return FLOAT_OK;
}

struct CfgMode {
  int bc;
  unsigned wr_mask, wa_mask, we_mask;
  int nclip = 1;  // clips stacked along the rows
};

CfgMode cfg_mode(float a, float r, float e, int include_r) {
  if (a == 1.0f && r == 1.0f && e == 1.0f) return {1, 1u, 1u, 1u, 1};  // FMT.py:346,400-401
  if (!include_r) return {3, 0b111u, 0b110u, 0b010u, 1};                // [null_wa,wa,wa] [null_we,we,null_we]
  return {4, 0b1110u, 0b1100u, 0b0100u, 1};                             // FMT.py:382-384
}

// Stage the conditions of one window (device pointers) and compute c_cond = c_embedder([wr,wa,we]).
template <class T>
int stage_window(float_fmt* h, const CfgMode& m, const float* x0, const float* wa, const float* wr, const float* we,
                 int we_len, const float* prev_x, const float* prev_wa, const float* prev_we, hipStream_t s) {
  const float_fmt_cfg_t& c = h->cfg;
  const int M = m.nclip * m.bc * h->ntok;
  hipLaunchKernelGGL((fmt_build_cond_kernel<T>), dim3(M), dim3(256), 0, s, h->cond16, h->Kc, m.bc, h->ntok, c.n_prev,
                     c.dim_w, c.dim_a, c.dim_e, wr, wa, prev_wa, we, we_len, prev_we, m.wr_mask, m.wa_mask, m.we_mask, h->sat);
  GemmArgs g = base_args(h->cond16, h->c_embed, M);
  g.sat = h->sat, g.out_f32 = h->ccond, g.ldo = h->D;
  int rc;
  if ((rc = run_gemm<T, EPI_F32>(h->tune, g, s))) return rc;
  const int n = m.nclip * h->ntok * c.dim_w;
  hipLaunchKernelGGL((fmt_init_x_kernel<T>), dim3((n + 255) / 256), dim3(256), 0, s, h->xcur, h->xin16, h->Kx / 32, x0, prev_x,
                     c.n_prev, c.n_cur, c.dim_w, m.nclip, h->sat);
  FH_CHECK_HIP(hipGetLastError());
  return FLOAT_OK;
}

// only the all-rows-per-workgroup head (FLOAT_FMT_NO_TOKBLK, a debugging aid) is limited to 15 row tiles
int check_cfg_rows(const float_fmt* h, const CfgMode& m) {
  FH_REQUIRE(!h->tune.no_tokblk || m.bc * h->ntok <= 240,
             "%d-way CFG of %d tokens is %d rows; the all-rows CFG epilogue GEMM holds at most 240 (15 row tiles)", m.bc, h->ntok,
             m.bc * h->ntok);
  return FLOAT_OK;
}

int check_common(float_fmt* h, const void* we, int we_len, const void* prev_we) {
  FH_REQUIRE(h != nullptr, "null FMT handle");
  FH_REQUIRE(we_len == 1 || we_len == h->cfg.n_cur,
             "Dynamic emotion latent `we` time dimension (%d) does not match audio latent `wa` time dimension (%d).",
             we_len, h->cfg.n_cur);
  FH_REQUIRE(!(we_len > 1 && prev_we == nullptr),
             "`we` is dynamic (T>1), but prev_we was not provided with prev_x/prev_wa.");
  (void)we;
  return FLOAT_OK;
}

// Fixed-grid explicit Runge-Kutta schemes of torchdiffeq's solver list (reference src/nodes/__init__.py:15-23):
// stage times t0 + c_j dt, stage inputs y0 + dt sum_m a[j][m] k_m, update dt sum_j b_j k_j.  torchdiffeq is not
// installed where this is built, so these are its published rules (midpoint; "rk4" = the 3/8-rule
// rk4_alt_step_func; heun2 / heun3 Butcher tableaux) - parity with the package itself is unpinned.
struct Tableau {
  int s;
  float c[4], a[4][3], b[4];
};
const Tableau& tableau(int method) {
  static const Tableau T[5] = {
      {1, {0.f}, {{0.f}}, {1.f}},                                                                        // euler
      {2, {0.f, 0.5f}, {{0.f}, {0.5f}}, {0.f, 1.f}},                                                     // midpoint
      {4, {0.f, 1.f / 3, 2.f / 3, 1.f}, {{0.f}, {1.f / 3}, {-1.f / 3, 1.f}, {1.f, -1.f, 1.f}}, {0.125f, 0.375f, 0.375f, 0.125f}},  // rk4 (3/8)
      {2, {0.f, 1.f}, {{0.f}, {1.f}}, {0.5f, 0.5f}},                                                     // heun2
      {3, {0.f, 1.f / 3, 2.f / 3}, {{0.f}, {1.f / 3}, {0.f, 2.f / 3}}, {0.25f, 0.f, 0.75f}},             // heun3
  };
  return T[method];
}

// evaluation times of a window: Euler -> the grid itself; RK -> t_i + c_j (t_{i+1} - t_i), step-major
TimeSpec time_spec(int method, int nfe) {
  const Tableau& tb = tableau(method);
  TimeSpec ts{};
  ts.nfe = nfe;
  ts.stages = tb.s;
  for (int j = 0; j < 4; ++j) ts.c[j] = tb.c[j];
  return ts;
}
int n_evals(int method, int nfe) { return (nfe - 1) * tableau(method).s; }

// The evaluations of one window, eager and single-stream (this is also what gets captured into the window's hipGraph and
// the profiling path).  Modulations come in batches of up to kScSteps evaluations (run_mod_all); FLOAT_FMT_HOIST=0 makes the
// batch one evaluation long.
template <class T>
int run_window_steps(float_fmt* h, const CfgMode& m, int nfe, const std::vector<float>& ts, float a, float r, float e,
                     hipStream_t s) {
  const Tableau& tb = tableau(h->method);
  const float_fmt_cfg_t& c = h->cfg;
  const size_t kstride = (size_t)h->Bmax * kMaxTok * c.dim_w;  // one stage's velocities: [clip][ntok][dim_w]
  const int n = m.nclip * c.n_cur * c.dim_w, rows = m.nclip * m.bc * h->ntok;
  const int nev = n_evals(h->method, nfe), batch = h->tune.hoist ? kScSteps : 1;
  const bool euler = h->method == FLOAT_ODE_EULER;
  int rc;
  for (int ev = 0; ev < nev; ++ev) {
    const int i = ev / tb.s, j = ev - i * tb.s, z = ev % batch;
    const float dt = ts[i + 1] - ts[i];
    if (z == 0 && (rc = run_mod_all<T>(h, rows, ev, std::min(batch, nev - ev), s))) return rc;
    const float* mod = h->modall + (size_t)z * h->mod_zs;  // the layout run_mod_all chose for this batch
    if (euler) {
      if ((rc = run_blocks<T>(h, m.nclip, m.bc, mod, true, dt, a, r, e, s))) return rc;
      continue;
    }
    // fixed-grid explicit Runge-Kutta: stage j evaluates at y0 + dt sum_m a[j][m] k_m, the update is dt sum_j b_j k_j
    if (j > 0) {
      hipLaunchKernelGGL((fmt_rk_combine_kernel<T>), dim3((n + 255) / 256), dim3(256), 0, s, h->xcur, h->kbuf, kstride, j,
                         dt * tb.a[j][0], dt * tb.a[j][1], dt * tb.a[j][2], 0.f, 0, h->xin16, h->Kx / 32, c.n_prev, c.n_cur,
                         c.dim_w, m.nclip, h->sat);
    }
    if ((rc = run_blocks<T>(h, m.nclip, m.bc, mod, false, 0.f, a, r, e, s, h->kbuf + (size_t)j * kstride))) return rc;
    if (j == tb.s - 1) {
      hipLaunchKernelGGL((fmt_rk_combine_kernel<T>), dim3((n + 255) / 256), dim3(256), 0, s, h->xcur, h->kbuf, kstride, tb.s,
                         dt * tb.b[0], dt * tb.b[1], dt * tb.b[2], dt * tb.b[3], 1, h->xin16, h->Kx / 32, c.n_prev, c.n_cur,
                         c.dim_w, m.nclip, h->sat);
    }
  }
  FH_CHECK_HIP(hipGetLastError());
  return FLOAT_OK;
}

// Same chain, replayed from a cached hipGraph (all pointers are workspace-internal, so the graph is reusable across windows
// and clips for a given (nfe, method, cfg mode, scales) and stack height).  The cache holds kMaxGraphs SETTINGS; the least
// recently used one is destroyed, with the graphs of all its stack heights, when a new setting arrives (a caller sweeping a
// CFG scale would otherwise keep a ~3000-node graph per value).  The stack height is not part of the key: a ragged job on a
// max_batch = 16 handle presents up to 16 heights of ONE setting, which live in one entry (6.5 ms of capture and about 1 MB
// each at 50 evaluations), so no number of heights evicts - only a ninth setting does.
constexpr size_t kMaxGraphs = 8;
void destroy_graphs(float_fmt::GraphEntry& g) {
  for (hipGraphExec_t& e : g.exec)
    if (e) {
      (void)hipGraphExecDestroy(e);
      e = nullptr;
    }
}
template <class T>
int run_window_steps_graph(float_fmt* h, const CfgMode& m, int we_len, int nfe, const std::vector<float>& ts, float a,
                           float r, float e, hipStream_t s) {
  float_fmt::GraphKey key;
  memset(&key, 0, sizeof(key));
  key.nfe = nfe;
  key.method = h->method;
  key.bc = m.bc;
  key.we_len = we_len;
  key.a = a;
  key.r = r;
  key.e = e;
  key.prio = stream_priority(s);
  FH_REQUIRE(m.nclip >= 1 && m.nclip <= kFmtMaxClips, "chain of %d clips (max %d)", m.nclip, kFmtMaxClips);
  float_fmt::GraphEntry* hit = nullptr;
  for (auto& g : h->graphs)
    if (g.key == key) hit = &g;
  if (!hit || !hit->exec[m.nclip]) {
    if (!h->cap_stream) FH_CHECK_HIP(hipStreamCreateWithFlags(&h->cap_stream, hipStreamNonBlocking));
    hipGraph_t graph = nullptr;
    h->cap_prio = key.prio;
    FH_CHECK_HIP(hipStreamBeginCapture(h->cap_stream, hipStreamCaptureModeThreadLocal));
    int rc = run_window_steps<T>(h, m, nfe, ts, a, r, e, h->cap_stream);
    hipError_t ce = hipStreamEndCapture(h->cap_stream, &graph);
    if (rc) {
      if (graph) (void)hipGraphDestroy(graph);
      return rc;
    }
    FH_CHECK_HIP(ce);
    hipGraphExec_t exec = nullptr;
    FH_CHECK_HIP(hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0));
    (void)hipGraphDestroy(graph);
    if (!hit) {
      if (h->graphs.size() >= kMaxGraphs) {
        size_t lru = 0;
        for (size_t i = 1; i < h->graphs.size(); ++i)
          if (h->graphs[i].used < h->graphs[lru].used) lru = i;
        // an executable that is still queued must not be destroyed under it - and it may be queued on ANOTHER stream than `s`
        // (the window sampler and the overlapped pipeline run the chain on side streams): eviction is rare (a ninth distinct
        // chain setting), so wait for the whole device
        hipError_t se = hipDeviceSynchronize();
        if (se != hipSuccess) {
          (void)hipGraphExecDestroy(exec);
          FH_CHECK_HIP(se);
        }
        destroy_graphs(h->graphs[lru]);
        h->graphs.erase(h->graphs.begin() + lru);
      }
      float_fmt::GraphEntry fresh;
      memset(&fresh, 0, sizeof(fresh));
      fresh.key = key;
      h->graphs.push_back(fresh);
      hit = &h->graphs.back();
    }
    hit->exec[m.nclip] = exec;
  }
  hit->used = ++h->graph_clock;
  FH_CHECK_HIP(hipGraphLaunch(hit->exec[m.nclip], s));
  return FLOAT_OK;
}

template <class T>
int window_impl(float_fmt* h, const float* x0, const float* wa, const float* wr, const float* we, int we_len,
                const float* prev_x, const float* prev_wa, const float* prev_we, int nfe, const std::vector<float>& ts,
                float a, float r, float e, int include_r, hipStream_t s, int nclip = 1) {
  CfgMode m = cfg_mode(a, r, e, include_r);
  m.nclip = nclip;
  int rc = check_cfg_rows(h, m);
  if (rc) return rc;
  if ((rc = stage_window<T>(h, m, x0, wa, wr, we, we_len, prev_x, prev_wa, prev_we, s))) return rc;
  if (nfe <= 1) return FLOAT_OK;  // a one-point grid has no evaluation: the sample is x0 (FLOAT.py:188,247-248)
  // A caller that is itself capturing `s` gets the chain launched straight into its capture (a graph cannot be launched or
  // captured from inside another capture); so does the profiling pass, whose events need eager launches.
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(s, &cs) != hipSuccess) {
    (void)hipGetLastError();
    cs = hipStreamCaptureStatusNone;
  }
  if (h->cfg.use_graph && !g_fh_profiling && cs == hipStreamCaptureStatusNone)
    return run_window_steps_graph<T>(h, m, we_len, nfe, ts, a, r, e, s);
  return run_window_steps<T>(h, m, nfe, ts, a, r, e, s);
}

template <class T>
int eval_impl(float_fmt* h, float t, const float* x, const float* wa, const float* wr, const float* we, int we_len,
              const float* prev_x, const float* prev_wa, const float* prev_we, float a, float r, float e, int include_r,
              float* out, hipStream_t s) {
  TimeSpec tsp{};
  tsp.t = t;
  int rc = prepare_time<T>(h, tsp, 1, s);
  if (rc) return rc;
  const CfgMode m = cfg_mode(a, r, e, include_r);
  if ((rc = check_cfg_rows(h, m))) return rc;
  if ((rc = stage_window<T>(h, m, x, wa, wr, we, we_len, prev_x, prev_wa, prev_we, s))) return rc;
  if ((rc = run_mod_all<T>(h, m.bc * h->ntok, 0, 1, s))) return rc;
  if ((rc = run_blocks<T>(h, 1, m.bc, h->modall, false, 0.f, a, r, e, s))) return rc;
  return dev_copy(out, h->vout, (size_t)h->ntok * h->cfg.dim_w, s);
}

// One window of the auto-regressive loop (FLOAT.py:214-251; nodes_adv.py:605-688).
template <class T>
int sample_window(float_fmt* h, int k, hipStream_t s) {
  const float_fmt_cfg_t& c = h->cfg;
  auto& J = h->job;
  const int L = c.n_cur, P = c.n_prev, Tn = J.T, B = J.B;
  const bool dynamic = J.we_len > 1;
  int rc;
  auto blocks = [](int n) { return dim3((n + 255) / 256); };
  if (k == J.first) {
    if ((rc = prepare_time<T>(h, time_spec(h->method, J.nfe), std::max(1, n_evals(h->method, J.nfe)), s))) return rc;
    // chunk 0 starts from zero history (FLOAT.py:217-219, nodes_adv.py:591-593); a job that starts at a later window
    // (float_fmt_sample_begin_range) from the history its caller hands over, or from zeros too
    if ((rc = copy_or_zero(h->prev_x, J.hist_x, (size_t)B * P * c.dim_w, s))) return rc;
    if ((rc = copy_or_zero(h->prev_wa, J.hist_wa, (size_t)B * P * c.dim_a, s))) return rc;
    if ((rc = copy_or_zero(h->prev_we, J.hist_we, (size_t)B * P * c.dim_e, s))) return rc;
  } else if (P > 0) {
    // AR hand-off: last P frames of the previous final sample / (padded) wa window / we window, per clip
    hipLaunchKernelGGL(fmt_tail_kernel, blocks(B * P * c.dim_w), dim3(256), 0, s, h->prev_x, h->xcur, P, L, c.dim_w, B);
    hipLaunchKernelGGL(fmt_tail_kernel, blocks(B * P * c.dim_a), dim3(256), 0, s, h->prev_wa, h->wa_c, P, L, c.dim_a, B);
    if (dynamic) hipLaunchKernelGGL(fmt_tail_kernel, blocks(B * P * c.dim_e), dim3(256), 0, s, h->prev_we, h->we_c, P, L, c.dim_e, B);
  }
  hipLaunchKernelGGL(fmt_slice_pad_kernel, blocks(B * L * c.dim_a), dim3(256), 0, s, h->wa_c, J.wa, k * L, Tn, L, c.dim_a, B);
  if (dynamic) hipLaunchKernelGGL(fmt_slice_pad_kernel, blocks(B * L * c.dim_e), dim3(256), 0, s, h->we_c, J.we, k * L, Tn, L, c.dim_e, B);
  // x0 is copied into the workspace so the window chain only ever sees handle-owned pointers; noise is (windows, clips, L, dim_w)
  if ((rc = dev_copy(h->x0_c, J.noise + (size_t)k * B * L * c.dim_w, (size_t)B * L * c.dim_w, s))) return rc;
  rc = window_impl<T>(h, h->x0_c, h->wa_c, J.wr, dynamic ? h->we_c : J.we, dynamic ? L : 1, h->prev_x, h->prev_wa,
                      dynamic ? h->prev_we : nullptr, J.nfe, J.ts, J.a, J.r, J.e, J.include_r, s, B);
  if (rc) return rc;
  const int rows = (k == J.total - 1) ? (Tn - k * L) : L;  // trim to T (FLOAT.py:252)
  return dev_copy2d(J.r_d + (size_t)k * L * c.dim_w, (size_t)Tn * c.dim_w, h->xcur, (size_t)L * c.dim_w, rows * c.dim_w, B, s);
}

// One window of a ragged job: the clips that still have a window k are the first `nact` slots, and the chain runs on them alone.
// A clip that has left the stack keeps its rows of the workspace, unread.  The staging is one launch per tensor whatever the
// clip count: the per-clip pointers and lengths are kernel arguments (FmtClipTab).
template <class T>
int sample_window_ragged(float_fmt* h, int k, hipStream_t s) {
  const float_fmt_cfg_t& c = h->cfg;
  auto& J = h->job;
  const int L = c.n_cur, P = c.n_prev;
  const bool dynamic = J.we_len > 1;
  int nact = 0;
  while (nact < J.B && J.rg_win[nact] > k) ++nact;
  int rc;
  auto blocks = [](int n) { return dim3((n + 255) / 256); };
  auto grid = [nact](int n) { return dim3((n + 255) / 256, nact); };
  if (k == 0) {
    if ((rc = prepare_time<T>(h, time_spec(h->method, J.nfe), std::max(1, n_evals(h->method, J.nfe)), s))) return rc;
    if ((rc = dev_zero(h->prev_x, (size_t)nact * P * c.dim_w, s))) return rc;
    if ((rc = dev_zero(h->prev_wa, (size_t)nact * P * c.dim_a, s))) return rc;
    if ((rc = dev_zero(h->prev_we, (size_t)nact * P * c.dim_e, s))) return rc;
    // the slot order holds for the whole job: wr and a static we are staged once
    hipLaunchKernelGGL(fmt_gather_pad_kernel, grid(c.dim_w), dim3(256), 0, s, h->wr_c, J.rg_wr, 0, 1, c.dim_w);
    if (!dynamic) hipLaunchKernelGGL(fmt_gather_pad_kernel, grid(c.dim_e), dim3(256), 0, s, h->we_c, J.rg_we, 0, 1, c.dim_e);
  } else if (P > 0) {
    hipLaunchKernelGGL(fmt_tail_kernel, blocks(nact * P * c.dim_w), dim3(256), 0, s, h->prev_x, h->xcur, P, L, c.dim_w, nact);
    hipLaunchKernelGGL(fmt_tail_kernel, blocks(nact * P * c.dim_a), dim3(256), 0, s, h->prev_wa, h->wa_c, P, L, c.dim_a, nact);
    if (dynamic) hipLaunchKernelGGL(fmt_tail_kernel, blocks(nact * P * c.dim_e), dim3(256), 0, s, h->prev_we, h->we_c, P, L, c.dim_e, nact);
  }
  hipLaunchKernelGGL(fmt_gather_pad_kernel, grid(L * c.dim_a), dim3(256), 0, s, h->wa_c, J.rg_wa, k * L, L, c.dim_a);
  if (dynamic) hipLaunchKernelGGL(fmt_gather_pad_kernel, grid(L * c.dim_e), dim3(256), 0, s, h->we_c, J.rg_we, k * L, L, c.dim_e);
  hipLaunchKernelGGL(fmt_gather_pad_kernel, grid(L * c.dim_w), dim3(256), 0, s, h->x0_c, J.rg_noise, k * L, L, c.dim_w);
  FH_CHECK_HIP(hipGetLastError());
  rc = window_impl<T>(h, h->x0_c, h->wa_c, h->wr_c, h->we_c, dynamic ? L : 1, h->prev_x, h->prev_wa,
                      dynamic ? h->prev_we : nullptr, J.nfe, J.ts, J.a, J.r, J.e, J.include_r, s, nact);
  if (rc) return rc;
  hipLaunchKernelGGL(fmt_scatter_trim_kernel, grid(L * c.dim_w), dim3(256), 0, s, J.rg_rd, h->xcur, k * L, L, c.dim_w);
  FH_CHECK_HIP(hipGetLastError());
  return FLOAT_OK;
}

template <class T>
int create_impl(float_fmt* h, const TensorTable& tt) {
  const float_fmt_cfg_t& c = h->cfg;
  const int D = c.dim_h;
  int rc;
  prime_kernels<T>();
  auto pack = [&](const std::vector<std::string>& names, int N_each, int K, Lin* out) {
    return pack_linear_pool<T>(h->tune, &h->pool, tt, names, N_each, K, out);
  };
  if ((rc = pack({"x_embedder.proj"}, D, c.dim_w, &h->x_embed))) return rc;
  if ((rc = pack({"t_embedder.mlp.0"}, D, 256, &h->t0))) return rc;
  if ((rc = pack({"t_embedder.mlp.2"}, D, D, &h->t2))) return rc;
  if ((rc = pack({"c_embedder"}, D, c.dim_w + c.dim_a + c.dim_e, &h->c_embed))) return rc;
  h->blk.resize(c.depth);
  std::vector<std::string> ada;
  for (int b = 0; b < c.depth; ++b) {
    const std::string p = "blocks." + std::to_string(b) + ".";
    if ((rc = pack({p + "attn.qkv"}, 3 * D, D, &h->blk[b].qkv))) return rc;
    if ((rc = pack({p + "attn.proj"}, D, D, &h->blk[b].proj))) return rc;
    if ((rc = pack({p + "mlp.fc1"}, c.mlp_hidden, D, &h->blk[b].fc1))) return rc;
    if ((rc = pack({p + "mlp.fc2"}, D, c.mlp_hidden, &h->blk[b].fc2))) return rc;
    ada.push_back(p + "adaLN_modulation.1");
  }
  if ((rc = pack(ada, 6 * D, D, &h->adaln_all))) return rc;
  // the head's adaLN (2D outputs) rides at the end of the same fused projection
  Lin tail;
  if ((rc = pack(std::vector<std::string>{"decoder.adaLN_modulation.1"}, 2 * D, D, &tail))) return rc;
  if ((rc = concat_linear_rows<T>(&h->pool, h->adaln_all, tail, &h->adaln_all))) return rc;
  if ((rc = pack({"decoder.linear"}, c.dim_w, D, &h->final_lin))) return rc;
  return FLOAT_OK;
}

}  // namespace


// ---------------------------------------------------------------- GEMM service (fmt_gemm.hpp)
int fmt_pack_linear(const FmtTune& tn, DevicePool* pool, int dtype, const TensorTable& tt, const std::vector<std::string>& names,
                    int N_each, int K, FmtLin* out) {
  FH_REQUIRE(dtype == FLOAT_DT_BF16 || dtype == FLOAT_DT_FP16 || dtype == FLOAT_DT_FP32, "the GEMM service: unknown dtype %d", dtype);
  return fmt_by_dtype(dtype, [&](auto t) { return pack_linear_pool<decltype(t)>(tn, pool, tt, names, N_each, K, out); });
}

int fmt_pack_linear_raw(const FmtTune& tn, DevicePool* pool, int dtype, const float* w, const float* b, int N, int K, FmtLin* out) {
  std::vector<float> zeros;
  if (!b) {
    zeros.assign(N, 0.f);
    b = zeros.data();
  }
  float_tensor_t t[2];
  memset(t, 0, sizeof(t));
  t[0].name = "raw.weight";
  t[0].data = w;
  t[0].ndim = 2;
  t[0].shape[0] = N;
  t[0].shape[1] = K;
  t[1].name = "raw.bias";
  t[1].data = b;
  t[1].ndim = 1;
  t[1].shape[0] = N;
  TensorTable tt(t, 2);
  return fmt_pack_linear(tn, pool, dtype, tt, {"raw"}, N, K, out);
}

GemmArgs fmt_gemm_args(const u16* A, const FmtLin& L, int M) { return base_args(A, L, M); }

void fmt_gemm_prime(int dtype) {
  fmt_by_dtype(dtype, [](auto t) { prime_kernels<decltype(t)>(); });
}

template <class T>
static int gemm_run_t(const FmtTune& tn, int epi, const GemmArgs& g, hipStream_t s) {
  switch (epi) {
    case EPI_F32: return run_gemm<T, EPI_F32>(tn, g, s);
    case EPI_T16: return run_gemm<T, EPI_T16>(tn, g, s);
    case EPI_SILU_P16: return run_gemm<T, EPI_SILU_P16>(tn, g, s);
    case EPI_GELU_P16: return run_gemm<T, EPI_GELU_P16>(tn, g, s);
    case EPI_GELUERF_P16: return run_gemm<T, EPI_GELUERF_P16>(tn, g, s);
    default: fh_set_error("fmt_gemm_run: epilogue %d is not exported", epi); return FLOAT_E_INVALID;
  }
}

int fmt_gemm_run(const FmtTune& tn, int dtype, int epi, GemmArgs g, hipStream_t s) {
  return fmt_by_dtype(dtype, [&](auto t) { return gemm_run_t<decltype(t)>(tn, epi, g, s); });
}

template <class T>
static int debug_impl(float_fmt* h, int what, const float* in, float* out, hipStream_t s) {
  const int D = h->D, ntok = h->ntok;
  if (what == 0) {
    return dev_copy(out, h->pos, (size_t)ntok * D, s);
  }
  if (what == 3 || what == 4) {
    // the K-split exchange of fmt_gemm_kernel on ONE workgroup's tile: 48 rows x 64 (what = 3) or 16 (what = 4) columns, K = 1024
    // over 8 waves (4 in the fp32 mode), zero bias: with 8 waves the straight-line form of the body (the 16-column tile through
    // attn.proj's epilogue, which carries it).  in = [A (48, 1024) | W (N, 1024)] fp32 rows.
    FH_REQUIRE(in != nullptr, "float_fmt_debug: request %d needs an input", what);
    constexpr int Mt = 48, Kt = 1024;
    const int Nt = what == 3 ? 64 : 16;
    std::vector<float> host((size_t)(Mt + Nt) * Kt);
    FH_CHECK_HIP(hipStreamSynchronize(s));
    FH_CHECK_HIP(hipMemcpy(host.data(), in, host.size() * sizeof(float), hipMemcpyDeviceToHost));
    struct Scratch : DevicePool {
      ~Scratch() { release(); }
    } pool;
    Lin a, w;  // A packs like a weight: the operand layout is the same for both
    int rc;
    if ((rc = fmt_pack_linear_raw(h->tune, &pool, h->cfg.dtype, host.data(), nullptr, Mt, Kt, &a))) return rc;
    if ((rc = fmt_pack_linear_raw(h->tune, &pool, h->cfg.dtype, host.data() + (size_t)Mt * Kt, nullptr, Nt, Kt, &w))) return rc;
    GemmArgs g = base_args(a.W, w, Mt);
    g.out_f32 = out, g.ldo = Nt;
    if (what == 3) {
      if ((rc = launch_gemm<T, EPI_F32>(g, 3, 4, T::is32 ? 4 : 8, s))) return rc;
    } else {
      // the 16-column tile as the chain runs it (attn.proj): out = 0 + 1 * (sum + 0), the sum itself
      float* ones = nullptr;
      if ((rc = pool.alloc(&ones, (size_t)Mt * Nt, false))) return rc;
      const std::vector<float> one((size_t)Mt * Nt, 1.f);
      FH_CHECK_HIP(hipMemcpy(ones, one.data(), one.size() * sizeof(float), hipMemcpyHostToDevice));
      FH_CHECK_HIP(hipMemsetAsync(out, 0, (size_t)Mt * Nt * sizeof(float), s));
      g.gate = ones, g.ldg = Nt;
      if ((rc = launch_gemm<T, EPI_GATE_RES>(g, 3, 1, T::is32 ? 4 : 8, s))) return rc;
    }
    FH_CHECK_HIP(hipStreamSynchronize(s));
    return FLOAT_OK;
  }
  if (what == 5) {  // in (64, 64) -> out (64, 5, 2, 64): fmt_xlane_probe_kernel
    FH_REQUIRE(in != nullptr, "float_fmt_debug: request %d needs an input", what);
    hipLaunchKernelGGL(fmt_xlane_probe_kernel, dim3(kXlaneProbeVecs), dim3(64), 0, s, in, out);
    FH_CHECK_HIP(hipGetLastError());
    return FLOAT_OK;
  }
  FH_REQUIRE(what == 1 && in != nullptr, "float_fmt_debug: unknown request %d (or null input)", what);
  const int n = ntok * 3 * D;
  hipLaunchKernelGGL((fmt_dbg_to16_kernel<T>), dim3((n + 255) / 256), dim3(256), 0, s, h->qkv16, in, n);
  launch_attn<T>(launch_ctx(h, s), ntok, nullptr);
  hipLaunchKernelGGL((fmt_dbg_unpack_kernel<T>), dim3((ntok * D + 255) / 256), dim3(256), 0, s, out, h->att16, ntok, D);
  FH_CHECK_HIP(hipGetLastError());
  return FLOAT_OK;
}

// the windows of the job float_fmt_sample_begin set up, one after the other
static int drain_job(float_fmt_t* h, void* stream) {
  int32_t left = 1;
  while (left > 0)
    if (int rc = float_fmt_sample_next(h, stream, nullptr, &left)) return rc;
  return FLOAT_OK;
}

extern "C" {

int float_fmt_create(const float_fmt_cfg_t* cfg, const float_tensor_t* tensors, int32_t n_tensors, float_fmt_t** out) {
  FH_REQUIRE(cfg && tensors && out, "null argument to float_fmt_create");
  FH_REQUIRE(cfg->dim_h % 256 == 0 && cfg->dim_h / 256 <= 8 && ((cfg->dim_h / 256) & (cfg->dim_h / 256 - 1)) == 0,
             "dim_h=%d unsupported", cfg->dim_h);
  FH_REQUIRE(cfg->dim_h / cfg->heads == 128, "head_dim must be 128 (dim_h=%d heads=%d)", cfg->dim_h, cfg->heads);
  FH_REQUIRE(cfg->dim_w % 128 == 0 && cfg->mlp_hidden % 128 == 0, "dim_w / mlp_hidden must be multiples of 128");
  FH_REQUIRE(cfg->n_prev + cfg->n_cur <= kMaxTok, "at most %d tokens per window (got %d)", kMaxTok, cfg->n_prev + cfg->n_cur);
  FH_REQUIRE(cfg->n_prev >= 0 && cfg->n_prev <= cfg->n_cur, "n_prev must be in [0, n_cur]");
  FH_REQUIRE(cfg->dtype == FLOAT_DT_BF16 || cfg->dtype == FLOAT_DT_FP16 || cfg->dtype == FLOAT_DT_FP32, "unknown dtype %d", cfg->dtype);
  FH_REQUIRE(cfg->max_batch >= 0 && cfg->max_batch <= 16, "max_batch must be in [0, 16] (got %d)", cfg->max_batch);
  float_fmt* h = new float_fmt();
  h->tune = FmtTune::from_env();
  h->cfg = *cfg;
  h->D = cfg->dim_h;
  h->ntok = cfg->n_prev + cfg->n_cur;
  // rows of every activation buffer: the 4-way CFG batch plus the row tiles a row-blocked tiling reads past it (row blocks
  // are 3-6 tiles; their operand loads are not guarded, the rows are zero and their results are dropped)
  h->Bmax = cfg->max_batch > 0 ? cfg->max_batch : 1;
  h->Mpad = 16 * ((h->Bmax * 4 * h->ntok + 15) / 16 + 12);  // + the row tiles a 192-row block reads past the last row
  h->Kc = round_up(cfg->dim_w + cfg->dim_a + cfg->dim_e, 128);
  h->Kx = round_up(cfg->dim_w, 128);
  {
    int dev = 0, ncu = 0;
    if (hipGetDevice(&dev) == hipSuccess && hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess) h->n_cu = ncu;
    else (void)hipGetLastError();
  }
  h->Ntot = cfg->depth * 6 * h->D + 2 * h->D;
  TensorTable tt(tensors, n_tensors);
  int rc = fmt_by_dtype(cfg->dtype, [&](auto t) { return create_impl<decltype(t)>(h, tt); });
  const int D = h->D, Mp = h->Mpad;
  const size_t esz = cfg->dtype == FLOAT_DT_FP32 ? 2 : 1;  // u16 slots per operand element
  auto A = [&](auto** p, size_t n) {
    // operand buffers (typed u16*) hold 4-byte elements in the fp32 mode
    if (!rc) rc = h->pool.alloc(p, std::is_same<std::remove_reference_t<decltype(**p)>, u16>::value ? n * esz : n, true);
  };
  A(&h->pos, (size_t)kMaxTok * D);
  A(&h->freqs, 128);
  A(&h->cond16, (size_t)Mp * h->Kc);
  A(&h->sc16, (size_t)kScSteps * Mp * D + (size_t)12 * 16 * D);  // + the row tiles a 192-row block reads past the last batch
  A(&h->h16, (size_t)Mp * D);
  A(&h->hfin16, (size_t)h->Bmax * 64 * ((kMaxTok + 15) / 16) * D);  // token-blocked rows of the head GEMM, clips x 4 CFG rows x 16 tokens per block
  A(&h->qkv16, (size_t)Mp * 3 * D);
  A(&h->att16, (size_t)Mp * D);
  A(&h->hid16, (size_t)Mp * cfg->mlp_hidden);
  A(&h->xin16, (size_t)(h->Bmax * kMaxTok + 6 * 16) * h->Kx);  // + the row tiles a row-blocked tiling reads past the last token (zero)
  A(&h->tsin16, (size_t)kMaxSteps * 256);
  A(&h->th16, (size_t)kMaxSteps * D);
  A(&h->ccond, (size_t)Mp * D);
  // modulations of a batch of evaluations (run_mod_all): never zero-filled or read before written, up to 3.1 GB at the
  // default shape (64 x 240 x 51 200 fp32) of the 288 GB
  h->Mmod = 16 * ((h->Bmax * 4 * h->ntok + 15) / 16);
  if (!rc) rc = h->pool.alloc(&h->modall, (size_t)kScSteps * h->Mmod * h->Ntot, false);
  A(&h->kbuf, (size_t)4 * h->Bmax * kMaxTok * cfg->dim_w);
  A(&h->xres, (size_t)Mp * D);
  A(&h->slab, (size_t)8 * Mp * D);
  A(&h->sat, 1);
  A(&h->xcur, (size_t)h->Bmax * cfg->n_cur * cfg->dim_w);
  A(&h->temb, (size_t)kMaxSteps * D);
  A(&h->vout, (size_t)h->Bmax * kMaxTok * cfg->dim_w);
  A(&h->wa_c, (size_t)h->Bmax * cfg->n_cur * cfg->dim_a);
  A(&h->we_c, (size_t)h->Bmax * cfg->n_cur * cfg->dim_e);
  A(&h->x0_c, (size_t)h->Bmax * cfg->n_cur * cfg->dim_w);
  A(&h->wr_c, (size_t)h->Bmax * cfg->dim_w);
  A(&h->prev_x, (size_t)h->Bmax * cfg->n_cur * cfg->dim_w);
  A(&h->prev_wa, (size_t)h->Bmax * cfg->n_cur * cfg->dim_a);
  A(&h->prev_we, (size_t)h->Bmax * cfg->n_cur * cfg->dim_e);
  if (!rc) {
    // pos_embed: from the checkpoint when present, else regenerated like the VA loader does
    // (nodes_vadv_loader.py:822-840): sin on even, cos on odd feature indices (FMT.py:29-37).
    std::vector<float> pos((size_t)h->ntok * D);
    const float_tensor_t* pe = tt.find("pos_embed");
    if (pe && TensorTable::numel(pe) == (int64_t)h->ntok * D) {
      memcpy(pos.data(), pe->data, pos.size() * sizeof(float));
    } else {
      for (int p = 0; p < h->ntok; ++p)
        for (int j = 0; j < D; ++j) {
          const float ang = (float)((double)p / pow(10000.0, 2.0 * (double)(j / 2) / (double)D));
          pos[(size_t)p * D + j] = (j & 1) ? cosf(ang) : sinf(ang);
        }
    }
    std::vector<float> fr(128);
    for (int k = 0; k < 128; ++k) fr[k] = expf(-logf(10000.0f) * (float)k / 128.0f);
    if (hipMemcpy(h->pos, pos.data(), pos.size() * sizeof(float), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(h->freqs, fr.data(), fr.size() * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) {
      fh_set_error("hipMemcpy of FMT tables failed");
      rc = FLOAT_E_HIP;
    }
  }
  if (rc) {
    float_fmt_destroy(h);
    return rc;
  }
  *out = h;
  return FLOAT_OK;
}

void float_fmt_destroy(float_fmt_t* h) {
  if (!h) return;
  for (auto& g : h->graphs) destroy_graphs(g);
  if (h->cap_stream) (void)hipStreamDestroy(h->cap_stream);
  h->pool.release();
  delete h;
}

int float_fmt_eval(float_fmt_t* h, float t, const float* x, const float* wa, const float* wr, const float* we,
                   int32_t we_len, const float* prev_x, const float* prev_wa, const float* prev_we, float a_cfg,
                   float r_cfg, float e_cfg, int32_t include_r_cfg, float* out, void* stream) {
  int rc = check_common(h, we, we_len, prev_we);
  if (rc) return rc;
  FH_REQUIRE(x && wa && wr && we && prev_x && prev_wa && out, "null tensor argument to float_fmt_eval");
  hipStream_t s = (hipStream_t)stream;
  return fmt_by_dtype(h->cfg.dtype, [&](auto tag) {
    return eval_impl<decltype(tag)>(h, t, x, wa, wr, we, we_len, prev_x, prev_wa, prev_we, a_cfg, r_cfg, e_cfg, include_r_cfg, out, s);
  });
}

int float_fmt_sample_chunk(float_fmt_t* h, const float* x0, const float* wa, const float* wr, const float* we,
                           int32_t we_len, const float* prev_x, const float* prev_wa, const float* prev_we, int32_t nfe,
                           float a_cfg, float r_cfg, float e_cfg, int32_t include_r_cfg, float* out, void* stream) {
  int rc = check_common(h, we, we_len, prev_we);
  if (rc) return rc;
  FH_REQUIRE(x0 && wa && wr && we && prev_x && prev_wa && out, "null tensor argument to float_fmt_sample_chunk");
  FH_REQUIRE(nfe >= 1 && n_evals(h->method, nfe) < kMaxSteps, "nfe=%d: too many evaluations (max %d)", nfe, kMaxSteps);
  hipStream_t s = (hipStream_t)stream;
  std::vector<float> ts;
  linspace01(nfe, &ts);
  const float_fmt_cfg_t& c = h->cfg;
  // stage caller tensors into handle-owned buffers (the graph path needs stable addresses)
  if ((rc = dev_copy(h->x0_c, x0, (size_t)c.n_cur * c.dim_w, s))) return rc;
  if ((rc = dev_copy(h->wa_c, wa, (size_t)c.n_cur * c.dim_a, s))) return rc;
  if ((rc = dev_copy(h->prev_x, prev_x, (size_t)c.n_prev * c.dim_w, s))) return rc;
  if ((rc = dev_copy(h->prev_wa, prev_wa, (size_t)c.n_prev * c.dim_a, s))) return rc;
  if (we_len > 1) {
    if ((rc = dev_copy(h->we_c, we, (size_t)c.n_cur * c.dim_e, s))) return rc;
    if ((rc = dev_copy(h->prev_we, prev_we, (size_t)c.n_prev * c.dim_e, s))) return rc;
  }
  const float* we_p = we_len > 1 ? h->we_c : we;
  const float* pwe_p = we_len > 1 ? h->prev_we : nullptr;
  const TimeSpec tsp = time_spec(h->method, nfe);
  const int nev = std::max(1, n_evals(h->method, nfe));
  rc = fmt_by_dtype(c.dtype, [&](auto t) {
    typedef decltype(t) T;
    if (int prc = prepare_time<T>(h, tsp, nev, s)) return prc;
    return window_impl<T>(h, h->x0_c, h->wa_c, wr, we_p, we_len, h->prev_x, h->prev_wa, pwe_p, nfe, ts, a_cfg, r_cfg, e_cfg,
                          include_r_cfg, s);
  });
  if (rc) return rc;
  return dev_copy(out, h->xcur, (size_t)c.n_cur * c.dim_w, s);
}

int float_fmt_debug(float_fmt_t* h, int32_t what, const float* in, float* out, void* stream) {
  FH_REQUIRE(h != nullptr && out != nullptr, "null argument to float_fmt_debug");
  return fmt_by_dtype(h->cfg.dtype, [&](auto t) { return debug_impl<decltype(t)>(h, what, in, out, (hipStream_t)stream); });
}

int float_fmt_saturation(float_fmt_t* h, uint64_t* total, int32_t reset, void* stream) {
  FH_REQUIRE(h && total, "null argument to float_fmt_saturation");
  FH_CHECK_HIP(hipStreamSynchronize((hipStream_t)stream));
  unsigned long long v = 0;
  FH_CHECK_HIP(hipMemcpy(&v, h->sat, sizeof(v), hipMemcpyDeviceToHost));
  *total = v;
  if (reset) {  // on the caller's stream: ordered against the launches that add to the counter there (not the NULL stream's memset)
    FH_CHECK_HIP(hipMemsetAsync(h->sat, 0, sizeof(v), (hipStream_t)stream));
    FH_CHECK_HIP(hipStreamSynchronize((hipStream_t)stream));
  }
  return FLOAT_OK;
}

int float_fmt_set_method(float_fmt_t* h, int32_t method) {
  FH_REQUIRE(h != nullptr, "null FMT handle");
  FH_REQUIRE(method >= FLOAT_ODE_EULER && method <= FLOAT_ODE_HEUN3, "unknown ODE method %d", method);
  h->method = method;
  return FLOAT_OK;
}

int float_fmt_sample_begin(float_fmt_t* h, const float* wr, const float* wa, int32_t T, const float* we, int32_t we_len,
                           const float* noise, int32_t nfe, float a_cfg, float r_cfg, float e_cfg, int32_t include_r_cfg,
                           float* r_d) {
  FH_REQUIRE(h != nullptr, "null FMT handle");
  FH_REQUIRE(wr && wa && we && noise && r_d, "null tensor argument to float_fmt_sample");
  FH_REQUIRE(T >= 1, "T must be >= 1 (got %d)", T);
  FH_REQUIRE(we_len == 1 || we_len == T,
             "Dynamic emotion latent `we` time dimension (%d) does not match audio latent `wa` time dimension (%d).",
             we_len, T);
  FH_REQUIRE(nfe >= 1 && n_evals(h->method, nfe) < kMaxSteps, "nfe=%d: too many evaluations (max %d)", nfe, kMaxSteps);
  auto& J = h->job;
  J.wr = wr;
  J.wa = wa;
  J.we = we;
  J.noise = noise;
  J.r_d = r_d;
  J.T = T;
  J.we_len = we_len;
  J.nfe = nfe;
  J.include_r = include_r_cfg;
  J.a = a_cfg;
  J.r = r_cfg;
  J.e = e_cfg;
  J.B = 1;
  J.ragged = false;
  J.next = 0;
  J.n_chunks = (T + h->cfg.n_cur - 1) / h->cfg.n_cur;
  J.first = 0;
  J.total = J.n_chunks;
  J.hist_x = J.hist_wa = J.hist_we = nullptr;
  linspace01(nfe, &J.ts);
  J.active = true;
  return FLOAT_OK;
}

int float_fmt_sample_begin_range(float_fmt_t* h, const float* wr, const float* wa, int32_t T, const float* we, int32_t we_len,
                                 const float* noise, int32_t nfe, float a_cfg, float r_cfg, float e_cfg, int32_t include_r_cfg,
                                 float* r_d, int32_t first_window, int32_t end_window, const float* hist_x, const float* hist_wa,
                                 const float* hist_we) {
  int rc = float_fmt_sample_begin(h, wr, wa, T, we, we_len, noise, nfe, a_cfg, r_cfg, e_cfg, include_r_cfg, r_d);
  if (rc) return rc;
  auto& J = h->job;
  J.active = false;
  FH_REQUIRE(first_window >= 0 && first_window < end_window && end_window <= J.total,
             "window range [%d, %d) outside the clip's %d windows", first_window, end_window, J.total);
  FH_REQUIRE(we_len == 1 || hist_we != nullptr || hist_x == nullptr,
             "a dynamic-emotion job that starts from a history needs hist_we too");
  J.first = J.next = first_window;
  J.n_chunks = end_window;
  J.hist_x = hist_x;
  J.hist_wa = hist_wa;
  J.hist_we = we_len > 1 ? hist_we : nullptr;
  J.active = true;
  return FLOAT_OK;
}

int float_fmt_sample_next(float_fmt_t* h, void* stream, int32_t* window_done, int32_t* windows_left) {
  FH_REQUIRE(h != nullptr && h->job.active, "float_fmt_sample_next without float_fmt_sample_begin");
  auto& J = h->job;
  hipStream_t s = (hipStream_t)stream;
  const int k = J.next;
  int rc = fmt_by_dtype(h->cfg.dtype, [&](auto t) {
    return J.ragged ? sample_window_ragged<decltype(t)>(h, k, s) : sample_window<decltype(t)>(h, k, s);
  });
  if (rc) {
    J.active = false;
    return rc;
  }
  J.next = k + 1;
  if (window_done) *window_done = k;
  if (windows_left) *windows_left = J.n_chunks - J.next;
  if (J.next >= J.n_chunks) J.active = false;
  return FLOAT_OK;
}

int float_fmt_sample_batch(float_fmt_t* h, int32_t n_clips, const float* wr, const float* wa, int32_t T, const float* we,
                           int32_t we_len, const float* noise, int32_t nfe, float a_cfg, float r_cfg, float e_cfg,
                           int32_t include_r_cfg, float* r_d, void* stream) {
  FH_REQUIRE(h != nullptr, "null FMT handle");
  FH_REQUIRE(n_clips >= 1 && n_clips <= h->Bmax, "batch of %d clips, the handle was created with max_batch = %d", n_clips, h->Bmax);
  int rc = float_fmt_sample_begin(h, wr, wa, T, we, we_len, noise, nfe, a_cfg, r_cfg, e_cfg, include_r_cfg, r_d);
  if (rc) return rc;
  h->job.B = n_clips;
  return drain_job(h, stream);
}

int float_fmt_sample_begin_ragged(float_fmt_t* h, int32_t n_clips, const int32_t* T, const float* const* wr,
                                  const float* const* wa, const float* const* we, int32_t we_dynamic,
                                  const float* const* noise, int32_t nfe, float a_cfg, float r_cfg, float e_cfg,
                                  int32_t include_r_cfg, float* const* r_d) {
  FH_REQUIRE(h != nullptr, "null FMT handle");
  FH_REQUIRE(T && wr && wa && we && noise && r_d, "null array argument to float_fmt_sample_begin_ragged");
  FH_REQUIRE(n_clips >= 1 && n_clips <= h->Bmax, "batch of %d clips, the handle was created with max_batch = %d", n_clips, h->Bmax);
  for (int i = 0; i < n_clips; ++i) {
    FH_REQUIRE(wr[i] && wa[i] && we[i] && noise[i] && r_d[i], "null tensor argument to float_fmt_sample_begin_ragged (clip %d)", i);
    FH_REQUIRE(T[i] >= 1, "T must be >= 1 (got %d for clip %d)", T[i], i);
  }
  FH_REQUIRE(nfe >= 1 && n_evals(h->method, nfe) < kMaxSteps, "nfe=%d: too many evaluations (max %d)", nfe, kMaxSteps);
  auto& J = h->job;
  J.active = false;
  const int L = h->cfg.n_cur;
  // slots by window count, descending and stable: equal lengths keep the caller's order
  int order[kFmtMaxClips];
  for (int i = 0; i < n_clips; ++i) order[i] = i;
  std::stable_sort(order, order + n_clips, [&](int x, int y) { return (T[x] + L - 1) / L > (T[y] + L - 1) / L; });
  memset(&J.rg_wr, 0, sizeof(J.rg_wr));
  memset(&J.rg_wa, 0, sizeof(J.rg_wa));
  memset(&J.rg_we, 0, sizeof(J.rg_we));
  memset(&J.rg_noise, 0, sizeof(J.rg_noise));
  memset(&J.rg_rd, 0, sizeof(J.rg_rd));
  for (int q = 0; q < n_clips; ++q) {
    const int i = order[q], Ti = T[i], win = (Ti + L - 1) / L;
    J.rg_win[q] = win;
    J.rg_wr.p[q] = wr[i], J.rg_wr.T[q] = 1;
    J.rg_wa.p[q] = wa[i], J.rg_wa.T[q] = Ti;
    J.rg_we.p[q] = we[i], J.rg_we.T[q] = we_dynamic ? Ti : 1;
    J.rg_noise.p[q] = noise[i], J.rg_noise.T[q] = win * L;
    J.rg_rd.p[q] = r_d[i], J.rg_rd.T[q] = Ti;
  }
  J.wr = J.wa = J.we = J.noise = nullptr;
  J.r_d = nullptr;
  J.T = 0;
  J.we_len = we_dynamic ? L : 1;  // per window, as the chain sees it
  J.nfe = nfe;
  J.include_r = include_r_cfg;
  J.a = a_cfg;
  J.r = r_cfg;
  J.e = e_cfg;
  J.B = n_clips;
  J.ragged = true;
  J.next = J.first = 0;
  J.n_chunks = J.total = J.rg_win[0];
  J.hist_x = J.hist_wa = J.hist_we = nullptr;
  linspace01(nfe, &J.ts);
  J.active = true;
  return FLOAT_OK;
}

int float_fmt_sample_batch_ragged(float_fmt_t* h, int32_t n_clips, const int32_t* T, const float* const* wr,
                                  const float* const* wa, const float* const* we, int32_t we_dynamic,
                                  const float* const* noise, int32_t nfe, float a_cfg, float r_cfg, float e_cfg,
                                  int32_t include_r_cfg, float* const* r_d, void* stream) {
  int rc = float_fmt_sample_begin_ragged(h, n_clips, T, wr, wa, we, we_dynamic, noise, nfe, a_cfg, r_cfg, e_cfg, include_r_cfg, r_d);
  if (rc) return rc;
  return drain_job(h, stream);
}

int float_fmt_sample(float_fmt_t* h, const float* wr, const float* wa, int32_t T, const float* we, int32_t we_len,
                     const float* noise, int32_t nfe, float a_cfg, float r_cfg, float e_cfg, int32_t include_r_cfg,
                     float* r_d, void* stream) {
  int rc = float_fmt_sample_begin(h, wr, wa, T, we, we_len, noise, nfe, a_cfg, r_cfg, e_cfg, include_r_cfg, r_d);
  if (rc) return rc;
  return drain_job(h, stream);
}

}  // extern "C"
