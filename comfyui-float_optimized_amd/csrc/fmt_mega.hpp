// Host side of the persistent evaluation kernel (fmt_mega_kernel, FLOAT_FMT_MEGA=1; the launch chain measured faster and is the
// default): the stage table of run_blocks' chain for one clip, the barrier words and their watchdog, and the launch.  Needs the
// handle, so fmt_api.hip includes it below struct float_fmt.
#pragma once
#include "fmt_launch.hpp"

namespace {

MegaSync mega_sync_of(const float_fmt* h) {
  unsigned* m = h->mega_sync;
  return MegaSync{m, m + 8 * 32, m + 9 * 32, m + 17 * 32, m + 18 * 32, h->mega_err_host, reinterpret_cast<unsigned long long*>(m + 20 * 32), (unsigned)h->tune.mega_stamp_wg};
}
// The persistent kernel's barrier watchdog, looked at by EVERY FMT call of the handle before it queues new work (the flag is
// host-mapped: no copy, no synchronisation when it is clear): a timeout in an earlier call means that call's results are
// invalid.  This call fails with the message; the device is drained, the cached window graphs (they hold the persistent
// kernel) are destroyed, the barrier words are cleared (their generation counters are out of step for good otherwise) and the
// handle runs the launch chain from here on.
int mega_poll(float_fmt* h) {
  if (!h->mega_err_host || *reinterpret_cast<volatile unsigned*>(h->mega_err_host) == 0u) return FLOAT_OK;
  FH_CHECK_HIP(hipDeviceSynchronize());  // graphs may be queued on other streams than the caller's
  for (auto& gr : h->graphs)
    for (hipGraphExec_t e : gr.exec)
      if (e) (void)hipGraphExecDestroy(e);
  h->graphs.clear();
  if (h->mega_sync) FH_CHECK_HIP(hipMemset(h->mega_sync, 0, (size_t)(32 * 20) * sizeof(unsigned)));
  *reinterpret_cast<volatile unsigned*>(h->mega_err_host) = 0u;
  h->tune.mega = 0;
  h->job.active = false;
  fh_set_error("fmt_mega_kernel: a grid barrier timed out in an earlier call (not all %d workgroups were resident) - the results of "
               "that call are invalid; the handle falls back to the launch chain (FLOAT_FMT_MEGA=0 selects it from the start)", 256);
  return FLOAT_E_HIP;
}
// The chain's shapes this kernel is built for: one clip, 3 CFG rows of 60 tokens (M = 180), dim_h 1024, the default launch
// options - i.e. exactly the tilings run_blocks would pick.  Anything else keeps the launch chain.
template <class T>
bool mega_shape_ok(const float_fmt* h, int nclip, int bc) {
  const FmtTune& tn = h->tune;
  if (T::is32 || !tn.mega || nclip != 1 || bc != 3 || h->D != 1024 || h->cfg.heads != 8 || h->n_cu < kMegaWgs) return false;
  if (attnproj_hpw(tn, h->D, h->cfg.heads) || tn.fc2_split != 4 || tn.proj_split != 0) return false;
  const int M = bc * h->ntok;
  auto is = [](Tiling t, int a, int b, int c) { return t.mtw == a && t.nt == b && t.nw == c; };
  const Blk& B = h->blk[0];
  return (M + 15) / 16 == 12 && (h->ntok + 15) / 16 == 4 && h->x_embed.K % 256 == 0 && h->final_lin.K % 256 == 0 &&
         is(pick_tiling(tn, M, B.qkv.N, B.qkv.K, false), 3, 4, 8) && is(pick_tiling(tn, M, B.proj.N, B.proj.K, false), 3, 1, 8) &&
         is(pick_tiling(tn, M, B.fc1.N, B.fc1.K, false), 3, 4, 8) && is(pick_tiling(tn, M, B.fc2.N * 4, B.fc2.K / 4, false), 3, 4, 8) &&
         B.fc2.K % 512 == 0;
}

template <class T>
int build_mega(float_fmt* h, int bc) {
  float_fmt::MegaPlan& P = h->mega[bc];
  P.tried = 1;
  {
    // every one of the 256 workgroups must be resident at once (a plain launch: nothing else checks it)
    int per_cu = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, reinterpret_cast<const void*>(fmt_mega_kernel<T>), 512, kMegaSmem) != hipSuccess) {
      (void)hipGetLastError();
      per_cu = 0;
    }
    if (per_cu * h->n_cu < kMegaWgs) {
      h->tune.mega = 0;  // the launch chain
      return FLOAT_OK;
    }
  }
  const float_fmt_cfg_t& c = h->cfg;
  const FmtTune& tn = h->tune;
  const int D = h->D, ntok = h->ntok, M = bc * ntok;
  std::vector<MegaStage> st;
  // A operands of the GEMM stages: one buffer per producing stage, written once per launch (see fmt_gemm_body, ldA)
  const size_t esz = sizeof(typename T::elem) / sizeof(u16);
  const size_t n_h = (size_t)h->Mpad * D * esz, n_hid = (size_t)h->Mpad * c.mlp_hidden * esz;
  if (!h->mega_ws) {
    int rc0 = h->pool.alloc(&h->mega_ws, (size_t)c.depth * (3 * n_h + n_hid), true);
    if (rc0) return rc0;
  }
  auto ws_h1 = [&](int b) { return h->mega_ws + (size_t)b * (3 * n_h + n_hid); };
  auto ws_h2 = [&](int b) { return ws_h1(b) + n_h; };
  auto ws_att = [&](int b) { return ws_h1(b) + 2 * n_h; };
  auto ws_hid = [&](int b) { return ws_h1(b) + 3 * n_h; };
  auto gemm_stage = [&](int kind, GemmArgs g, int mtw, int nt) {
    MegaStage m;
    memset(&m, 0, sizeof(m));
    m.kind = kind;
    g.sat = h->sat;
    g.mblk = ((g.M + 15) / 16 + mtw - 1) / mtw;
    if (g.ksplit < 1) g.ksplit = 1;
    fmt_gemm_head(g, nt * 16, kind == MS_FC2);  // fc2 is the chain's EPI_PARTIAL stage
    m.g = g;
    m.nblk = (unsigned)((g.N / (nt * 16)) * g.mblk * g.ksplit);
    return m;
  };
  auto ln_stage = [&](int b_mod, int which, int ks, const float* bias, int gate_col, const Lin* next, int touch_bit, u16* out, int perm) {
    MegaStage m;
    memset(&m, 0, sizeof(m));
    m.kind = MS_LN;
    m.nblk = (unsigned)(((M + 63) / 64) * 64);
    m.shift_off = (long long)b_mod * 6 * D + (long long)which * D;
    m.scale_off = m.shift_off + D;
    m.ks = ks;
    m.red_bias = bias;
    m.red_gate_off = (long long)b_mod * 6 * D + (long long)gate_col * D;
    m.ln_out = out ? out : h->h16;
    m.perm = perm;
    if (next && (tn.touch & (1 | touch_bit))) m.pf = make_touch(tn, *next, M, 0, (m.nblk / 8) * 64, 6);
    return m;
  };
  {  // x_embedder + pos_embed (run_blocks): 8 K-splitting waves here instead of 4 (every stage runs the 512-thread workgroup)
    GemmArgs g = base_args(h->xin16, h->x_embed, ntok);
    g.out_f32 = h->xres;
    g.ldo = D;
    g.pos = h->pos;
    g.bc = bc;
    g.ntok = ntok;
    st.push_back(gemm_stage(MS_XEMBED, g, 4, 1));
  }
  for (int b = 0; b < c.depth; ++b) {
    const Blk& B = h->blk[b];
    // LN1: folds the previous block's fc2 slabs (gate_mlp of block b - 1)
    if (b == 0) st.push_back(ln_stage(b, 0, 0, nullptr, 0, &B.qkv, 128, ws_h1(b), 0));
    else {
      MegaStage m = ln_stage(b, 0, 4, h->blk[b - 1].fc2.b, 0, &B.qkv, 128, ws_h1(b), 0);
      m.red_gate_off = (long long)(b - 1) * 6 * D + 5LL * D;
      st.push_back(m);
    }
    {
      GemmArgs g = base_args(ws_h1(b), B.qkv, M);
      g.out16 = h->qkv16;
      g.ldo16 = 3 * D;
      if (tn.touch & 8) g.touch = make_touch(tn, B.proj, M, 0, gemm_lanes_per_xcd(tn, M, g.N, g.K), 2);
      st.push_back(gemm_stage(MS_QKV, g, 3, 4));
    }
    {
      MegaStage m;
      memset(&m, 0, sizeof(m));
      m.kind = MS_ATTN;
      m.nblk = (unsigned)(c.heads * ((M + 7) / 8));
      if (tn.touch & 2) m.pf = make_touch(tn, B.proj, M, 0, (m.nblk / 8) * 128, 2);
      m.att_out = ws_att(b);
      st.push_back(m);
    }
    {
      GemmArgs g = base_args(ws_att(b), B.proj, M);
      g.out_f32 = h->xres;
      g.ldo = D;
      g.ldg = h->Ntot;
      if (tn.touch & 16) g.touch = make_touch(tn, B.fc1, M, 0, gemm_lanes_per_xcd(tn, M, g.N, g.K), 2);
      MegaStage m = gemm_stage(MS_PROJ, g, 3, 1);
      m.gate_off = (long long)b * 6 * D + 2LL * D;
      st.push_back(m);
    }
    st.push_back(ln_stage(b, 3, 0, nullptr, 0, &B.fc1, 64, ws_h2(b), 0));
    {
      GemmArgs g = base_args(ws_h2(b), B.fc1, M);
      g.out16 = ws_hid(b);
      g.ldo16 = B.fc2.K / 32;
      if (tn.touch & 4) g.touch = make_touch(tn, B.fc2, M, 4, gemm_lanes_per_xcd(tn, M, g.N, g.K), 2);
      st.push_back(gemm_stage(MS_FC1, g, 3, 4));
    }
    {
      GemmArgs g = base_args(ws_hid(b), B.fc2, M);
      to_slab(g, h->slab, h->Mpad, 4);
      if (tn.touch & 32) {
        const unsigned lanes = gemm_lanes_per_xcd(tn, M, g.N * 4, g.K / 4);
        if (b + 1 < c.depth) g.touch = make_touch(tn, h->blk[b + 1].qkv, M, 0, lanes, 2);
        else g.touch = make_touch(tn, h->final_lin, M, 0, lanes, 2, 1);
      }
      st.push_back(gemm_stage(MS_FC2, g, 3, 4));
    }
  }
  {
    const int nblk = (ntok + 15) / 16, seqs = bc;
    MegaStage m = ln_stage(c.depth, 0, 4, h->blk[c.depth - 1].fc2.b, 0, nullptr, 0, h->hfin16, seqs * 16);
    m.red_gate_off = (long long)(c.depth - 1) * 6 * D + 5LL * D;
    st.push_back(m);
    GemmArgs g = base_args(h->hfin16, h->final_lin, nblk * seqs * 16);
    g.tokblk = 1;
    g.nclip = 1;
    g.bc = bc;
    g.ntok = ntok;
    g.n_prev = c.n_prev;
    g.xcur = h->xcur;
    g.xin16 = h->xin16;
    g.ldx = h->Kx / 32;
    st.push_back(gemm_stage(MS_HEAD, g, bc, 1));
  }
  for (const MegaStage& m : st) FH_REQUIRE(m.nblk <= (unsigned)kMegaWgs, "persistent kernel: a stage needs %u workgroups", m.nblk);
  int rc;
  if (!h->mega_sync && (rc = h->pool.alloc(&h->mega_sync, 32 * 20 + 2 * 3 * 64, true))) return rc;  // + stamps of <= 64 stages
  if (!h->mega_err_host) {
    FH_CHECK_HIP(hipHostMalloc(reinterpret_cast<void**>(&h->mega_err_host), 64, hipHostMallocMapped));
    memset(h->mega_err_host, 0, 64);
  }
  if ((rc = h->pool.alloc(&P.dev, st.size(), false))) return rc;
  FH_CHECK_HIP(hipMemcpy(P.dev, st.data(), st.size() * sizeof(MegaStage), hipMemcpyHostToDevice));
  P.nstage = (int)st.size();
  P.bc = bc;
  P.ctx = MegaCtx{h->xres, h->qkv16, h->slab, (size_t)h->Mpad * D, M, D, ntok, h->Ntot, c.attn_window, c.heads, h->sat, fmt_make_div((unsigned)ntok)};
  return FLOAT_OK;
}

template <class T>
int run_mega(float_fmt* h, int bc, const float* modbuf, bool euler, float dt, float a, float r, float e, hipStream_t s, float* vout_to) {
  float_fmt::MegaPlan& P = h->mega[bc];
  MegaDyn d{modbuf, dt, a, r, e, euler ? 1 : 0, vout_to ? vout_to : h->vout};
  fh_launch_prof(0, (fmt_mega_kernel<T>), dim3(kMegaWgs), dim3(512), kMegaSmem, s, P.dev, P.nstage, d, P.ctx, mega_sync_of(h));
  FH_CHECK_HIP(hipGetLastError());
  return FLOAT_OK;
}

// At create (the first evaluation may already run under stream capture, where nothing can be allocated or copied): the stage
// table for `bc` CFG rows when the handle's shapes and switches are the kernel's.
template <class T>
int prepare_mega(float_fmt* h, int bc) {
  if constexpr (T::is32) return FLOAT_OK;
  else return mega_shape_ok<T>(h, 1, bc) ? build_mega<T>(h, bc) : FLOAT_OK;
}

}  // namespace
