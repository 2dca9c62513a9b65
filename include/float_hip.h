/* float_hip.h - C ABI of libfloat_hip.so: the FLOAT hot path on MI355X (gfx950).
 *
 * Two operators replace the two loops of the reference (set-soft/ComfyUI-FLOAT_Optimized):
 *
 *   FMT  - FlowMatchingTransformer.forward_with_cfv and the fixed-grid Euler loop around it
 *          (reference src/nodes/models/float/FMT.py:277-401, FLOAT.py:209-253,
 *          nodes_adv.py:545-694).
 *   DEC  - Synthesis.forward + per-frame post-process
 *          (reference src/nodes/models/float/styledecoder.py:497-534, FLOAT.py:113-169,
 *          nodes_vadv.py:447-464).
 *
 * Conventions
 *   - plain C, no C++/torch types; every function returns 0 on success or a FLOAT_E_* code,
 *     float_last_error() gives the message (thread-local).  No exception crosses the ABI.
 *   - all tensor arguments of the run-time calls are DEVICE pointers to contiguous fp32
 *     (the reference's tensors are fp32 everywhere); `stream` is a hipStream_t passed as void*.
 *     All work is enqueued on that stream; nothing synchronises the device.
 *   - batch size is 1 at this level, exactly like the reference decode loop (FLOAT.py:140);
 *     the host mirror loops over batch items as FloatProcess does (nodes.py:189-209).  The
 *     batched entries are float_fmt_sample_batch (the reference's samplers take a batch) and its
 *     ragged sibling float_fmt_sample_batch_ragged.
 *   - a handle owns its packed weights and a fixed workspace allocated at create time; no
 *     allocation happens inside the run-time calls (float_aud_reserve is the explicit exception).
 *     Every run-time call enqueues kernels only (device-to-device moves included: memcpy / memset
 *     nodes of a caller's stream capture did not replay reproducibly on ROCm 7.2), except
 *     float_dec_frames_host[_u8|_i420], whose last batch goes to the host by hipMemcpyAsync.  Capture by the
 *     caller (hipStreamBeginCapture on `stream`) is tested for the float_fmt_* calls.
 *   - calls on one handle must be serialised by the caller; different handles are independent.
 */
#ifndef FLOAT_HIP_H
#define FLOAT_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Stays 6: float_sfd_reserve_batch / float_sfd_maps_batch / float_sfd_post_batch / float_sfd_detect_batch / float_sfd_dense_batch
 * (the face detector on n stacked views in one pass), float_aud_reserve_segments / float_aud_classify_segments / float_aud_expand_rows (dynamic emotion: all chunks of a
 * clip through one stacked speech-emotion pass), float_img_resample / float_img_resample_work_bytes / float_img_resample_plan / float_img_resample_plan_ints (bicubic and
 * Lanczos resampling of 8-bit frames on the device), float_img_paste_i420 (the pasted frames as planar YUV 4:2:0),
 * float_img_paste (the generated frames back in the source portrait on the device),
 * float_aud_debug (test hook of the audio attention stage), float_jpg_encode / float_jpg_work_bytes (baseline JPEG files from 8-bit frames on the device) and
 * float_jpg_encode_padded / float_jpg_work_bytes_padded (the same for sides that are no multiples of 16),
 * float_img_front / float_img_front_work_bytes (the image front end on the device),
 * float_aud_front / float_aud_front_len / float_aud_front_work_bytes (the audio front end on the device),
 * float_cmp_segments / float_cmp_work_bytes (the precision guard's on-device comparison), float_dec_frames_u8 /
 * float_dec_frames_host_u8 (8-bit frames), float_dec_frames_i420 / float_dec_frames_host_i420 (planar YUV 4:2:0 frames) and
 * float_fmt_sample_begin_ragged / float_fmt_sample_batch_ragged (clips of different
 * lengths in one chain) are purely additive - no existing signature, structure or behaviour changed, so a
 * caller built against the earlier v6 header runs unchanged. */
#define FLOAT_HIP_ABI_VERSION 6

enum {
  FLOAT_OK = 0,
  FLOAT_E_INVALID = 1,   /* bad argument / shape mismatch (ValueError in the host mirror) */
  FLOAT_E_MISSING = 2,   /* a required checkpoint tensor is absent (KeyError) */
  FLOAT_E_HIP = 3,       /* HIP runtime error (RuntimeError) */
  FLOAT_E_NOMEM = 4
};

/* MFMA operand type; accumulation, statistics, softmax, residual stream and ODE state are fp32 in every mode.
 * FLOAT_DT_FP32 (every operator): the verification mode - fp32 operands on v_mfma_f32_16x16x4_f32, the same launch chain and
 * the same kernels with 4-byte elements, held to the reference goldens at 1e-4 (tests/test_fmt_fp32_gpu.py,
 * tests/test_dec_fp32_gpu.py); 1/16 of the 16-bit MFMA rate, no tuned tilings. */
enum { FLOAT_DT_BF16 = 0, FLOAT_DT_FP16 = 1, FLOAT_DT_FP32 = 2 };

/* One checkpoint tensor, named with the reference's state-dict key (prefix stripped):
 * e.g. "blocks.0.attn.qkv.weight" (FMT) or "convs.3.conv.weight" (decoder).  `data` is a HOST
 * pointer to contiguous fp32; it is only read during *_create. */
typedef struct {
  const char* name;
  const float* data;
  int32_t ndim;
  int64_t shape[6];
} float_tensor_t;

/* ---------------------------------------------------------------- FMT ------------- */
/* Shape contract = reference BaseOptions (options/base_options.py:36-45). */
typedef struct {
  int32_t dim_w, dim_a, dim_e, dim_h;
  int32_t depth, heads;
  int32_t mlp_hidden;      /* int(dim_h * mlp_ratio) */
  int32_t n_prev, n_cur;   /* num_prev_frames, int(wav2vec_sec*fps); n_prev + n_cur <= 80 */
  int32_t attn_window;     /* |i-j| <= window is visible (FMT.py:15-19) */
  int32_t dtype;           /* FLOAT_DT_* */
  int32_t use_graph;       /* 0: eager launches; != 0: replay each window's chain from a cached hipGraph (the graphs of at
                              most 8 chain settings per handle - nfe, CFG shape, scales, method, stream priority - least recently
                              used setting evicted, which synchronises the device; one graph per stack height of a setting).  1 and 2 are the same (1 used to put the
                              adaLN GEMM on a parallel branch; that GEMM now runs once per window, not per step). */
  int32_t max_batch;       /* clips float_fmt_sample_batch may stack per launch chain (sizes the workspace: rows = max_batch x 4 CFG
                              rows x tokens; the per-window modulation slab is 64 x rows x (depth * 6 + 2) * dim_h fp32, 3.1 GB per
                              clip at the default shape); 0 = 1 */
} float_fmt_cfg_t;

typedef struct float_fmt float_fmt_t;

int float_fmt_create(const float_fmt_cfg_t* cfg, const float_tensor_t* tensors, int32_t n_tensors,
                     float_fmt_t** out);
void float_fmt_destroy(float_fmt_t* h);

/* Fixed-grid solver of the sampling calls, the reference's TORCHDIFFEQ_FIXED_STEP_SOLVERS list
 * (src/nodes/__init__.py:15-23; options/base_options.py:50).  Default FLOAT_ODE_EULER (fused update in the last
 * GEMM's epilogue); the Runge-Kutta schemes evaluate the field s times per step (2/4/2/3). */
enum { FLOAT_ODE_EULER = 0, FLOAT_ODE_MIDPOINT = 1, FLOAT_ODE_RK4 = 2, FLOAT_ODE_HEUN2 = 3, FLOAT_ODE_HEUN3 = 4 };
int float_fmt_set_method(float_fmt_t* h, int32_t method);

/* Range check of the 16-bit modes of the FMT, encoder and audio operators (no reference counterpart: the reference is fp32).
 * fp16 ends at 65504.  Outside the decoder a 16-bit activation store CLAMPS at +-65504 (a NaN becomes -65504) so that one
 * outlier degrades the result instead of poisoning it - and every such store is COUNTED: each thread keeps the maximum
 * magnitude of the halves it stores and adds 1 to the handle's device counter if one reached the clamp value.  (The ResBlock
 * conv1 of the encoder runs the decoder's conv kernel, which stores inf instead of clamping and counts it the same way.)
 *   total: threads with at least one clamped / non-finite 16-bit store since the handle was created / last reset - zero or not
 *   is what matters.  Synchronises `stream`.  A non-zero total means the result is NOT the reference's within the stated
 *   tolerance: run that checkpoint with dtype FLOAT_DT_FP32 (or bf16 for the FMT / audio operators, whose exponent range is
 *   fp32's).  Always 0 for bf16 and fp32 handles. */
int float_fmt_saturation(float_fmt_t* h, uint64_t* total, int32_t reset, void* stream);

/* forward_with_cfv (FMT.py:342-401), B = 1.
 *   x, wa: (n_cur, dim)   wr: (dim_w)   we: (we_len, dim_e) with we_len 1 (static) or n_cur
 *   prev_x, prev_wa: (n_prev, dim)   prev_we: (n_prev, dim_e) - required iff we_len > 1
 *   out: (n_prev + n_cur, dim_w)
 * All three scales == 1 -> a single conditional pass (FMT.py:400-401); otherwise the 3-row
 * batch [uncond | all | audio-only], or the 4-row batch when include_r_cfg != 0. */
int float_fmt_eval(float_fmt_t* h, float t, const float* x, const float* wa, const float* wr,
                   const float* we, int32_t we_len, const float* prev_x, const float* prev_wa,
                   const float* prev_we, float a_cfg, float r_cfg, float e_cfg, int32_t include_r_cfg,
                   float* out, void* stream);

/* One window of the ODE loop (FLOAT.py:229-248): Euler over linspace(0,1,nfe), i.e. nfe-1
 * evaluations starting from x0 (n_cur, dim_w); out = final sample (n_cur, dim_w). */
int float_fmt_sample_chunk(float_fmt_t* h, const float* x0, const float* wa, const float* wr,
                           const float* we, int32_t we_len, const float* prev_x, const float* prev_wa,
                           const float* prev_we, int32_t nfe, float a_cfg, float r_cfg, float e_cfg,
                           int32_t include_r_cfg, float* out, void* stream);

/* The whole auto-regressive loop (FLOAT.py:209-253; nodes_adv.py:578-694).
 *   wr: (dim_w)   wa: (T, dim_a)   we: (1|T, dim_e)   noise: (ceil(T/n_cur), n_cur, dim_w),
 *   the explicit form of the reference's sequential randn draws (FLOAT.py:215)
 *   r_d: (T, dim_w).  Last window replicate-padded, prev_* handed off on the device. */
int float_fmt_sample(float_fmt_t* h, const float* wr, const float* wa, int32_t T, const float* we,
                     int32_t we_len, const float* noise, int32_t nfe, float a_cfg, float r_cfg,
                     float e_cfg, int32_t include_r_cfg, float* r_d, void* stream);

/* B independent clips of equal length through ONE launch chain (the reference's samplers take a batch: nodes_vadv.py:618-735
 * -> nodes_adv.py:545-694, x0 = randn(B, 50, 512) at FLOAT.py:215): the clips' rows are stacked, so every weight is read once
 * per evaluation for all of them.  Each clip's result is what float_fmt_sample gives for it alone, bit for bit where the
 * GEMM tilings coincide and within rounding otherwise (the tiling depends on the row count).
 *   wr: (B, dim_w)   wa: (B, T, dim_a)   we: (B, we_len, dim_e)   noise: (windows, B, n_cur, dim_w)   r_d: (B, T, dim_w)
 * n_clips <= max_batch of the handle. */
int float_fmt_sample_batch(float_fmt_t* h, int32_t n_clips, const float* wr, const float* wa, int32_t T,
                           const float* we, int32_t we_len, const float* noise, int32_t nfe, float a_cfg,
                           float r_cfg, float e_cfg, int32_t include_r_cfg, float* r_d, void* stream);

/* B independent clips of their OWN lengths T[i] through one stacked chain, window by window: a clip leaves the stack after its
 * last window, so no window is computed for padding and clips need not be grouped by length.  Each clip's result is what
 * float_fmt_sample gives for it alone, within the rounding stated for float_fmt_sample_batch.  No reference counterpart (the
 * reference's batches share one length); the window body is FLOAT.py:214-251 unchanged.
 *   T, wr, wa, we, noise, r_d: HOST arrays of n_clips entries (the convention of float_dec_set_feats), read during _begin only;
 *   the entries are device pointers that must stay valid until the last window has run:
 *     wr[i]: (dim_w)   wa[i]: (T[i], dim_a)   we[i]: (1, dim_e) for every clip, or - we_dynamic != 0 - (T[i], dim_e) for every clip
 *     noise[i]: (ceil(T[i] / n_cur), n_cur, dim_w), the clip's own sequential draws   r_d[i]: (T[i], dim_w)
 * Caller order is arbitrary: the operator orders its slots by window count (descending, stable), so the clips active in
 * window k are a prefix of the stack; with equal lengths the launches are those of float_fmt_sample_batch.  The pointers and
 * lengths reach the staging kernels as by-value kernel arguments: nothing is allocated, uploaded or synchronised, and the calls
 * may be captured like the others.  n_clips <= max_batch of the handle.
 * _begin_ragged records the job; float_fmt_sample_next then enqueues one window per call (windows_left counts down from the
 * longest clip's window count; rows [k*n_cur, min(T[i], (k+1)*n_cur)) of every r_d[i] that has a window k are complete once
 * that stream work is done).  _batch_ragged = _begin_ragged + every window, like float_fmt_sample_batch. */
int float_fmt_sample_begin_ragged(float_fmt_t* h, int32_t n_clips, const int32_t* T, const float* const* wr,
                                  const float* const* wa, const float* const* we, int32_t we_dynamic,
                                  const float* const* noise, int32_t nfe, float a_cfg, float r_cfg, float e_cfg,
                                  int32_t include_r_cfg, float* const* r_d);
int float_fmt_sample_batch_ragged(float_fmt_t* h, int32_t n_clips, const int32_t* T, const float* const* wr,
                                  const float* const* wa, const float* const* we, int32_t we_dynamic,
                                  const float* const* noise, int32_t nfe, float a_cfg, float r_cfg, float e_cfg,
                                  int32_t include_r_cfg, float* const* r_d, void* stream);

/* The same loop one window at a time, so the caller can overlap the decode of window k (on another
 * stream) with the sampling of window k+1: _begin only records the job (pointers must stay valid
 * until the last _next), each _next enqueues ONE window on `stream` and reports its index and how
 * many remain.  r_d rows [k*n_cur, min(T,(k+1)*n_cur)) are complete once that stream work is done. */
int float_fmt_sample_begin(float_fmt_t* h, const float* wr, const float* wa, int32_t T, const float* we,
                           int32_t we_len, const float* noise, int32_t nfe, float a_cfg, float r_cfg,
                           float e_cfg, int32_t include_r_cfg, float* r_d);
int float_fmt_sample_next(float_fmt_t* h, void* stream, int32_t* window_done, int32_t* windows_left);

/* A job over the windows [first_window, end_window) of the clip only, starting from the history the caller hands over: the
 * multi-GPU window shard (a rank samples its range from zero history, receives its predecessor's boundary latents by an RCCL
 * all_gather and re-solves from them).  No reference counterpart (the reference has no distributed code); the window body is
 * FLOAT.py:214-251 unchanged.  Same arguments as float_fmt_sample_begin (full-clip wa / we / noise / r_d pointers), plus
 *   hist_x (n_prev, dim_w), hist_wa (n_prev, dim_a), hist_we (n_prev, dim_e; read only with we_len > 1): the last n_prev rows
 *   of the previous window's sample / padded wa window / we window, or all NULL = zeros, the history of window 0.
 * Only r_d rows of the job's windows are written.  Continue with float_fmt_sample_next (windows_left counts to end_window). */
int float_fmt_sample_begin_range(float_fmt_t* h, const float* wr, const float* wa, int32_t T, const float* we,
                                 int32_t we_len, const float* noise, int32_t nfe, float a_cfg, float r_cfg,
                                 float e_cfg, int32_t include_r_cfg, float* r_d, int32_t first_window,
                                 int32_t end_window, const float* hist_x, const float* hist_wa, const float* hist_we);

/* Stream capture: every float_fmt_* run-time call may be issued while `stream` is being captured by the caller
 * (hipStreamBeginCapture); the chain is then launched straight into that capture instead of replaying the handle's own
 * graph, and no host memory is read by the stream (evaluation times are formed on the device).
 *
 * Test hook for the two tables the model builds instead of loading (FMT.py:15-40, 234-236, 249-250):
 *   what = 0: out (n_prev + n_cur, dim_h) = the positional table the handle adds in x_embedder (the checkpoint's
 *             `pos_embed` when given, else regenerated: nodes_vadv_loader.py:822-840), `in` unused;
 *   what = 1: the attention kernel of the chain on caller data: in (n_prev + n_cur, 3 * dim_h) = [q | k | v] rows of one
 *             CFG row, out (n_prev + n_cur, dim_h) = softmax(q k^T / sqrt(128) + band mask) v per head; with q = k = 0 and
 *             one-hot v rows the output shows which keys each query may see (enc_dec_mask, FMT.py:15-19).
 *   what = 3 / 4: one workgroup of the chain's GEMM on caller data, 48 rows x 64 (3) or 16 (4) columns with K = 1024 split over
 *             its 8 waves (4 in the fp32 mode; the 64-column tile exists for fp16 / bf16 only): in = [A (48, 1024) | W (N, 1024)],
 *             out (48, N) = A W^T in fp32 with no bias.  Wave w multiplies columns w * 1024 / waves .. of A and W, so operands
 *             that are zero outside one wave's columns show that wave's partial sum alone.  Synchronises the stream.
 *   what = 5: the kernels' cross-lane reductions on caller data: in (64, 64) = 64 vectors of one value per lane of a wave,
 *             out (64, 5, 2, 64) = per vector and lane the 64-lane sum, the 64-lane max and the sums over the lane's aligned
 *             group of 16, 8 and 4 lanes, each in the form the kernels use (DPP / lane swaps, index 0) and as the
 *             __shfl_xor butterfly it replaces (index 1): the two must agree bit for bit.
 * in / out are fp32 device pointers. */
int float_fmt_debug(float_fmt_t* h, int32_t what, const float* in, float* out, void* stream);

/* ---------------------------------------------------------------- decoder --------- */
typedef struct {
  int32_t size;        /* output resolution, 64..512 (styledecoder.py:448) */
  int32_t style_dim;   /* 512 */
  int32_t dtype;       /* FLOAT_DT_FP16 (activations / conv weights), or FLOAT_DT_FP32 = the verification mode (the same launch
                          chain with 4-byte activations and weights); bf16 is refused: too few mantissa bits for the warp */
  int32_t max_frames;  /* frames decoded per internal batch (sizes the workspace) */
} float_dec_cfg_t;

typedef struct float_dec float_dec_t;

/* tensors: the Synthesis state dict (prefix `motion_autoencoder.dec.` stripped), reference key names.
 * Blur FIR of the up-sampling StyledConvs (styledecoder.py:209-213): the checkpoint's `convs.N.conv.blur.kernel` buffer where
 * present (what the reference ends up with after its strict load_state_dict, nodes_vadv_loader.py:632), else the optional
 * 1-D tensor `blur_kernel` (the loader's widget: Synthesis(blur_kernel=...), styledecoder.py:448), else [1,3,3,1].  4-tap
 * kernels only, a buffer must be make_kernel's outer product k (x) k.  ToRGB / ToFlow `to_rgbs.N.upsample.kernel` /
 * `to_flows.N.upsample.kernel` buffers (styledecoder.py:373,394: make_kernel([1,3,3,1]) * 4 by construction, the checkpoint's
 * after the strict load): any rank-1 4 x 4 kernel ky (x) kx is applied per level and per module; another size or a kernel of
 * rank > 1 is refused (FLOAT_E_INVALID). */
int float_dec_create(const float_dec_cfg_t* cfg, const float_tensor_t* tensors, int32_t n_tensors,
                     float_dec_t** out);
void float_dec_destroy(float_dec_t* h);

/* Per clip: the encoder's skip features, reference order (encoder.py:220-231):
 * feats[i] = (C_i, R_i, R_i) fp32 NCHW, R_i = 8 << i.  Repacked to NHWC 16-bit in the handle. */
int float_dec_set_feats(float_dec_t* h, const float* const* feats, int32_t n_feats, void* stream);

/* decode_latent_into_processed_images (FLOAT.py:113-169) without the host copy:
 *   s_r: (style_dim)   r_d: (n_frames, style_dim)
 *   out: (n_frames, size, size, 3) fp32 in [0,1] = clamp(rgb,-1,1)*0.5+0.5, HWC. */
int float_dec_frames(float_dec_t* h, const float* s_r, const float* r_d, int32_t n_frames,
                     float* out_hwc, void* stream);

/* The same with the reference's hand-over to host memory (FLOAT.py:139,157-167: frames land in a pre-allocated CPU tensor):
 * frames are rendered into out_hwc (device, n_frames * size * size * 3) and every finished batch of max_frames frames is
 * copied to host_hwc (same layout).
 *   host_hwc: PINNED or REGISTERED host memory (hipHostMalloc / hipHostRegister / torch pin_memory), 16-byte aligned, gets
 *     the fast path: copy workgroups inside the next batch's launches store the frames straight through its device-side
 *     address (hipPointerGetAttributes decides; nothing is assumed).  Pageable memory is accepted too and takes one
 *     hipMemcpyAsync behind each batch on `stream` (staged by the runtime, slower, same bytes).
 *   copy_stream == NULL or == stream: the copies ride along / are queued on `stream` behind each batch (in order).
 *   another stream: the copy of batch i runs there while `stream` renders batch i+1, and `stream` is made to wait for the
 *     last copy before the call returns.  Measured on MI355X / ROCm 7.2 this does NOT pay inside the whole path: the
 *     decode + copy phase drops from 42 to 30 ms per 250 frames, but a device-to-host copy issued on a second stream leaves
 *     the FMT chain that follows 12 ms slower (84.6 -> 97 ms, even after a full device synchronisation), see DESIGN.md.
 * Either way, synchronising `stream` (or an event recorded on it) means the frames are in host memory. */
int float_dec_frames_host(float_dec_t* h, const float* s_r, const float* r_d, int32_t n_frames,
                          float* out_hwc, float* host_hwc, void* stream, void* copy_stream);

/* 8-bit frames: the same two calls with (n_frames, size, size, 3) uint8_t HWC output, quantised on the device by the kernel
 * that forms the frame: with y the value float_dec_frames stores, q = (uint8_t) rintf(y * 255.0f) (round half to even) -
 * bit-identical to rounding the fp32 frames on the host, at a quarter of the device staging, pinned memory and PCIe bytes.
 * out_hwc must be 4-byte aligned (FLOAT_E_INVALID otherwise: the last-level kernel stores packed dwords).  host_hwc follows
 * float_dec_frames_host's contract word for word: pinned and 16-byte aligned takes the copy workgroups, anything else
 * (pageable, misaligned) one hipMemcpyAsync behind each batch; copy_stream as there; synchronising `stream` means the frames are
 * in host memory.  Both work on FLOAT_DT_FP16 and FLOAT_DT_FP32 handles, and calls of either format may alternate on one handle. */
int float_dec_frames_u8(float_dec_t* h, const float* s_r, const float* r_d, int32_t n_frames,
                        uint8_t* out_hwc, void* stream);
int float_dec_frames_host_u8(float_dec_t* h, const float* s_r, const float* r_d, int32_t n_frames,
                             uint8_t* out_hwc, uint8_t* host_hwc, void* stream, void* copy_stream);

/* Planar YUV 4:2:0 frames (I420), converted on the device from the 8-bit samples R8, G8, B8 that float_dec_frames_u8 stores.
 * One frame is 3 * size * size / 2 bytes: the Y plane size x size, then U and V at size/2 x size/2 each, row-major, contiguous.
 * `matrix` selects the conversion.  All four have one form, in int32 with >> an arithmetic shift (floor):
 *   Y  = ((cr R8 + cg G8 + cb B8 + rnd) >> 8) + off                                   per pixel
 *   Mc = (c00 + c01 + c10 + c11 + 2) >> 2                                             per 2 x 2 block and channel c
 *   U, V = ((cr MR + cg MG + cb MB + rnd) >> 8) + off                                 per block
 * with the rows (cr, cg, cb, rnd, off) of
 *   id  name                                Y                     U                          V
 *   0   FLOAT_DEC_MATRIX_BT601_LIMITED      66, 129, 25, 128, 16  -38, -74, 112, 128, 128    112,  -94, -18, 128, 128
 *   2   FLOAT_DEC_MATRIX_BT709_LIMITED      47, 157, 16, 128, 16  -26, -86, 112, 128, 128    112, -102, -10, 128, 128
 *   4   FLOAT_DEC_MATRIX_BT601_FULL         77, 150, 29, 128, 0   -43, -85, 128, 127, 128    128, -107, -21, 127, 128
 *   6   FLOAT_DEC_MATRIX_BT709_FULL         54, 183, 19, 128, 0   -29, -99, 128, 127, 128    128, -116, -12, 127, 128
 * The id is a flag word: bit 1 = BT.709, bit 2 = full range; bit 0 and every higher bit must be 0, so 1, 3, 5, 7, 8, -1 are
 * FLOAT_E_INVALID, refused before anything else is looked at.  Every Y row sums to 220 (limited) or 256 (full) and every chroma
 * row to 0: a grey sample gives exactly U = V = 128.  No clamp is needed: limited range gives Y in [16, 235] and U, V in
 * [16, 240], full range exactly [0, 255] on every plane (the chroma rounding term of 127 keeps pure blue and red at 255).  Each
 * plane is within 1.17 levels of the float64 formulas of BT.601 / BT.709 (Kr, Kb = 0.299, 0.114 / 0.2126, 0.0722).  Id 0 is
 *   Y = ((66 R8 + 129 G8 + 25 B8 + 128) >> 8) + 16,  U = ((-38 MR - 74 MG + 112 MB + 128) >> 8) + 128,
 *   V = ((112 MR - 94 MG - 18 MB + 128) >> 8) + 128
 * (chroma sited at the block centre, Y4M's C420jpeg).  The definition starts from the 8-bit samples, so the bytes are those a
 * caller gets by converting float_dec_frames_u8's frames this way, whichever kernel forms them.  `out` must be 4-byte aligned;
 * `host`, `copy_stream` and what synchronising `stream` means follow float_dec_frames_host_u8's contract word for word (pinned and
 * 16-byte aligned: copy workgroups; anything else: one hipMemcpyAsync behind each batch).  Calls of all three formats may
 * alternate on one handle. */
enum { FLOAT_DEC_MATRIX_BT601_LIMITED = 0 };
enum { FLOAT_DEC_MATRIX_BT709_LIMITED = 2, FLOAT_DEC_MATRIX_BT601_FULL = 4, FLOAT_DEC_MATRIX_BT709_FULL = 6 };
int float_dec_frames_i420(float_dec_t* h, const float* s_r, const float* r_d, int32_t n_frames, int32_t matrix,
                          uint8_t* out, void* stream);
int float_dec_frames_host_i420(float_dec_t* h, const float* s_r, const float* r_d, int32_t n_frames, int32_t matrix,
                               uint8_t* out, uint8_t* host, void* stream, void* copy_stream);

/* Shape (channels, resolution) of skip feature i as float_dec_set_feats reads it: feats[i] must hold
 * channels * resolution * resolution floats.  Lets the caller validate tensors wired from an arbitrary encoder. */
int float_dec_feat_shape(float_dec_t* h, int32_t i, int32_t* channels, int32_t* resolution);

/* Same, but returns the un-clamped NCHW rgb of Synthesis.forward (styledecoder.py:532-534);
 * parity tests use it to look under the clamp. */
int float_dec_frames_raw(float_dec_t* h, const float* s_r, const float* r_d, int32_t n_frames,
                         float* out_chw, void* stream);

/* Range check of the 16-bit mode.  fp16 ends at 65504; the operator keeps what it stores small by construction (every
 * StyledConv's style is divided by its max |s| per frame, the factor goes into the demodulation's epsilon: exact algebra,
 * dec_kernels.hpp) and COUNTS what still did not fit: such a value is stored as inf and poisons what it touches (loud, not a
 * plausible-looking wrong frame); every thread keeps the maximum magnitude of the 16-bit values it stores and adds 1 to its
 * layer's counter per output tile that held an inf / NaN - the count is of (thread, tile) groups of 16..128 values, zero or not
 * is what matters.
 *   total: the sum since the handle was created / last reset;  per_site: NULL or FLOAT_DEC_SAT_SITES counters
 *   ([0..15] output of StyledConv i (0 = conv1, 1 + 2l / 2 + 2l = up-conv / conv of level l), [16 + l] blend of level l,
 *   [32] constant input, [33] skip features, [34] style vectors with a NaN / inf in them, i.e. a non-finite latent).
 *   Synchronises `stream`.  A non-zero total means the frames are NOT the reference's: run that checkpoint with dtype
 *   FLOAT_DT_FP32.  Always 0 in the fp32 mode (except [34]). */
#define FLOAT_DEC_SAT_SITES 40
int float_dec_saturation(float_dec_t* h, uint64_t* total, uint64_t* per_site, int32_t reset, void* stream);

/* Test hooks: ONE op of the decoder on caller data through the production kernels and launchers (what the full chain cannot
 * show: which op is off).  All pointers device fp32; tensors are host fp32 with the reference module's own key names.
 *   float_dec_debug_styled_conv: StyledConv.forward(x, style) (styledecoder.py:302-325, noise weight 0):
 *     leaky_relu(ModulatedConv2d(x, style) + bias) * sqrt(2).  keys `sc.conv.weight` (1,cout,cin,3,3),
 *     `sc.conv.modulation.weight` (cin,style_dim), `sc.conv.modulation.bias` (cin), `sc.activate.bias` (cout); optional
 *     `sc.conv.blur.kernel` (4,4) / `blur_kernel` (4) as in float_dec_create.
 *     x (n_frames,cin,res,res) NCHW, style (n_frames,style_dim), out (n_frames,cout,R',R'), R' = res or 2 res (upsample).
 *     Which kernel runs follows the production rules: plain conv res >= 16 -> dec_conv16_kernel, below -> dec_conv_kernel;
 *     up-conv 2 res >= 64 -> dec_zblur_kernel, res >= 8 -> dec_zconv4_kernel + dec_blur_kernel, res = 4 -> per-class
 *     dec_conv_kernel + dec_blur_kernel.  *saturated = the range counter of the op's 16-bit output stores (float_dec_saturation's rule: a value beyond fp16's range is stored as inf and counted).  flags bit 0: no style normalisation.
 *   float_dec_debug_flow_level: ToFlow (styledecoder.py:399-425) + ToRGB (:368-386) of one level: keys `to_flow.conv.weight`,
 *     `to_flow.conv.modulation.weight|bias`, `to_flow.bias`, `to_rgb.conv.0.weight`, `to_rgb.conv.1.bias`, `to_rgb.bias`.
 *     x (F,C,R,R) the conv output, feat (C,R,R) the skip feature (the reference repeats it over the batch), style (F,style_dim),
 *     prev_flow / prev_rgb (F,3,R/2,R/2) or NULL;  out_flow (F,3,R,R) = ToFlow's `out` before tanh / sigmoid,
 *     out_blend (F,C,R,R) = feat_warp + x (1 - mask), out_rgb (F,3,R,R) = ToRGB(feat_warp, prev_rgb).  Each output optional. */
typedef struct {
  int32_t dtype;      /* FLOAT_DT_FP16 | FLOAT_DT_FP32 */
  int32_t cin, cout;  /* flow level: cin = C, cout unused */
  int32_t res;        /* input resolution */
  int32_t upsample;
  int32_t n_frames;
  int32_t style_dim;
  int32_t flags;
} float_dec_unit_t;
int float_dec_debug_styled_conv(const float_dec_unit_t* u, const float_tensor_t* tensors, int32_t n_tensors, const float* x,
                                const float* style, float* out, uint64_t* saturated, void* stream);
int float_dec_debug_flow_level(const float_dec_unit_t* u, const float_tensor_t* tensors, int32_t n_tensors, const float* x,
                               const float* feat, const float* style, const float* prev_flow, const float* prev_rgb,
                               float* out_flow, float* out_blend, float* out_rgb, void* stream);

/* Direction.forward (styledecoder.py:428-444; FLOAT.py:289-291, nodes_vadv.py:479-533): r_s = lam @ Q^T with
 * Q from the QR of (direction.weight + 1e-8), factorised once at create time.  lam: (motion_dim), r_s: (style_dim). */
int float_dec_direction(float_dec_t* h, const float* lam, float* r_s, void* stream);

/* Same hand-over without the fp32 round trip: feats16[i] = (R_i, R_i, C_i) NHWC device buffers of element type `dtype`
 * (must equal the decoder's: 16-bit, or fp32 in the verification mode), e.g. the ones float_enc_feats16 returns. */
int float_dec_set_feats16(float_dec_t* h, const void* const* feats16, int32_t n_feats, int32_t dtype,
                          void* stream);

/* ---------------------------------------------------------------- encoder --------- */
/* Appearance / motion encoder, once per clip: EncoderApp.forward
 * (reference src/nodes/models/float/encoder.py:203-231), Encoder.fc (encoder.py:242-247) and
 * Direction (styledecoder.py:428-444, QR hoisted to create time), as called by
 * FLOAT.encode_image_into_latent / inference (FLOAT.py:283-291).
 * Checkpoint keys: `net_app.convs.*`, `fc.*` (prefix `motion_autoencoder.enc.` stripped) and,
 * optionally, `direction.weight` (from `motion_autoencoder.dec.`) to get r_s as well.  The Blur buffers of the down-sampling
 * ConvLayers (`net_app.convs.N.conv2.0.kernel`, `net_app.convs.N.skip.0.kernel`, encoder.py:59-75) are applied as the
 * checkpoint holds them (any 4 x 4 values; make_kernel([1,3,3,1]) where the state has none); another size is refused. */
typedef struct {
  int32_t size;        /* input resolution, power of two in [64, 1024] */
  int32_t dim;         /* 512 */
  int32_t dim_motion;  /* 20 */
  int32_t dtype;       /* FLOAT_DT_* of activations / conv weights (FLOAT_DT_FP32 = verification mode, feeds an fp32 decoder);
                          accumulation, s_r, fc are fp32 */
} float_enc_cfg_t;

typedef struct float_enc float_enc_t;

int float_enc_create(const float_enc_cfg_t* cfg, const float_tensor_t* tensors, int32_t n_tensors,
                     float_enc_t** out);
void float_enc_destroy(float_enc_t* h);

/* img: (3, size, size) fp32 NCHW in [-1,1] (generate.py:34-39).  Outputs (device, fp32, each optional):
 *   s_r (dim); lam = Encoder.fc(s_r) (dim_motion); r_s = Direction(lam) (dim; needs direction.weight);
 *   feats[i] (C_i, R_i, R_i) NCHW with R_i = 8 << i, the reference's res[::-1][2:] order
 *   (n_feats <= log2(size) - 2; NULL entries are skipped). */
int float_enc_forward(float_enc_t* h, const float* img, float* s_r, float* lam, float* r_s,
                      float* const* feats, int32_t n_feats, void* stream);

/* The NHWC 16-bit feature maps left in the handle by the last float_enc_forward (valid until the
 * next one), reference order; *n_out = how many were written (<= max_feats). */
int float_enc_saturation(float_enc_t* h, uint64_t* total, int32_t reset, void* stream); /* see float_fmt_saturation */
int float_enc_feats16(float_enc_t* h, const void** feats16, int32_t* channels, int32_t max_feats,
                      int32_t* n_out);
/* Stream-ordered copies of those maps into caller buffers (dst[i]: R_i x R_i x C_i elements of the operator's type, reference
 * order): a batch of portraits (nodes.py:189-209) keeps one set per item and hands it to float_dec_set_feats16 when the item
 * is decoded, instead of encoding the item a second time. */
int float_enc_export_feats16(float_enc_t* h, void* const* dst, int32_t n_feats, void* stream);

/* ---------------------------------------------------------------- audio encoder --- */
/* Audio conditioning, once per clip: AudioEncoder.inference (reference
 * src/nodes/models/float/FLOAT.py:370-375) = Wav2VecModel.forward(input_values, seq_len,
 * output_hidden_states=True) (src/nodes/models/wav2vec2.py:33-98: feature extractor ->
 * linear_interpolation(align_corners=True) to seq_len frames (:184-197) -> feature projection -> encoder),
 * hidden_states[1:] stacked per frame (FLOAT.py:345-352) and audio_projection = Linear -> LayerNorm ->
 * SiLU (FLOAT.py:338-342).  The wav2vec2 arithmetic itself lives in the `transformers` package
 * (requirements.txt:8, not vendored); it is restated from that package's module definitions for the bundled
 * wav2vec2_base config (src/nodes/model_configs/wav2vec2_base/config.json: feat_extract_norm "group",
 * conv_bias false, do_stable_layer_norm false, eager attention without mask).
 * Checkpoint keys: `wav2vec2.*` and `audio_projection.{0,1}.*` (prefix `audio_encoder.` stripped);
 * the positional conv accepts `parametrizations.weight.original0/1`, `weight_g/weight_v` or a plain `weight`. */
typedef struct {
  int32_t n_conv;              /* feature-extractor layers (7) */
  int32_t conv_dim[8], conv_kernel[8], conv_stride[8];
  int32_t hidden, layers, heads, intermediate;   /* 768, 12, 12, 3072 */
  int32_t pos_k, pos_groups;   /* num_conv_pos_embeddings 128, groups 16 */
  int32_t dim_w;               /* 512 */
  int32_t only_last;           /* opt.only_last_features */
  int32_t dtype;               /* FLOAT_DT_* of activations / weights (FLOAT_DT_FP32 = verification mode); statistics and the
                                  residual stream are fp32 */
  float ln_eps;                /* layer_norm_eps 1e-5 */
  /* Architecture switches of the wav2vec2-large family used by the speech-emotion model
   * (src/nodes/model_configs/emotion_ser/config.json): all 0 for wav2vec2-base. */
  int32_t feat_norm_layer;     /* feat_extract_norm == "layer": LayerNorm over channels after every conv */
  int32_t stable_ln;           /* do_stable_layer_norm: pre-LayerNorm encoder layers + one final LayerNorm */
  int32_t conv_bias;           /* feature-extractor convs carry a bias */
  int32_t num_labels;          /* > 0: classification head (float_aud_classify) instead of the audio projection */
} float_aud_cfg_t;

typedef struct float_aud float_aud_t;

int float_aud_create(const float_aud_cfg_t* cfg, const float_tensor_t* tensors, int32_t n_tensors,
                     float_aud_t** out);
void float_aud_destroy(float_aud_t* h);

/* Sizes the workspace for clips of up to n_samples samples and seq_len transformer frames (seq_len <= 0: the feature
 * extractor's own length, as float_aud_classify uses it).  The ONLY call that allocates after create: it synchronises
 * `stream` first when buffers have to grow (earlier work may still read the old ones) and never shrinks.  Not capturable. */
int float_aud_reserve(float_aud_t* h, int32_t n_samples, int32_t seq_len, void* stream);
int float_aud_saturation(float_aud_t* h, uint64_t* total, int32_t reset, void* stream); /* see float_fmt_saturation */

/* a: (n_samples) fp32 device, the normalised 16 kHz waveform already replicate-padded by the caller to a
 * multiple of seq_len * sampling_rate / fps when needed (FLOAT.py:371-373);  wa: (seq_len, dim_w) fp32.
 * Allocation-free: a clip beyond the reserved capacity is refused (FLOAT_E_INVALID) - call float_aud_reserve first. */
int float_aud_inference(float_aud_t* h, const float* a, int32_t n_samples, int32_t seq_len, float* wa,
                        void* stream);

/* Speech-to-emotion (reference Audio2Emotion.predict_emotion, FLOAT.py:378-401, on
 * Wav2Vec2ForSpeechClassification, src/nodes/models/wav2vec2_ser.py:41-118): wav2vec2 encoder on the un-interpolated
 * feature sequence, mean over time, dense -> tanh -> out_proj, softmax.  Handle created with num_labels > 0 and the
 * keys `wav2vec2.*`, `classifier.dense.*`, `classifier.out_proj.*` (prefix `emotion_encoder.wav2vec2_for_emotion.`
 * stripped).  scores: (num_labels) fp32 device. */
int float_aud_classify(float_aud_t* h, const float* a, int32_t n_samples, float* scores, void* stream);

/* Test hook for one stage of the encoder on caller data (additive: the ABI version does not change).
 *   what = 1: the attention launch exactly as float_aud_inference / float_aud_classify dispatch it for this handle (by operand
 *             type and by FLOAT_AUD_ATTN_MFMA as read at create): in (Tn, 3 * hidden) = [q | k | v] rows, rounded to the
 *             operand type; out (Tn, hidden) = softmax(q k^T / 8) v per head of 64, no mask, as the handle stores it.
 * in / out are fp32 device pointers.  Allocation-free: Tn beyond the reserved frames is refused - call float_aud_reserve first.
 *   what = 2: the normalised copy that the last float_aud_classify_segments(FLOAT_AUD_SEG_NORMALIZE) left in the workspace: the
 *             first Tn floats of its dense (n_seg, seg_len) layout -> out.  `in` is not read (NULL allowed). */
int float_aud_debug(float_aud_t* h, int32_t what, const float* in, int32_t Tn, float* out, void* stream);

/* Dynamic emotion: the equal chunks of a clip through the speech-emotion model as ONE launch sequence (the reference's
 * FloatExtractEmotionWithCustomModelDyn.extract_dynamic_emotion, src/nodes/nodes_vadv.py, calls predict_emotion once per
 * 2-s chunk).  The chunks are independent sequences of equal length, so the transformer runs on n_seg x L stacked rows:
 * every GEMM, LayerNorm and GELU launch is row-wise and serves as it is; the positional conv pads at every segment's edges,
 * attention takes one grid plane per segment, and the mean over time and the head run per segment in the same launches.
 * Additive: the ABI version does not change.
 *   a:       device waveform at the model's rate; segment s = the seg_len samples at a + s * seg_stride, seg_stride >= seg_len.
 *            Never written.
 *   flags & FLOAT_AUD_SEG_NORMALIZE: every segment is first brought to zero mean / unit variance on its own,
 *            (x - mean) / sqrt(var + 1e-7) with the biased variance and fp64 statistics: float_aud_front's rule per segment.
 *            The normalised copy lives in the workspace.  Without the flag the segments are used as given.
 *   scores:  (n_seg, num_labels); row s is what float_aud_classify defines for segment s alone.
 *   frames:  NULL, or (T, num_labels): float_aud_expand_rows(scores, n_seg, num_labels, frames, T, scale).
 * Handles with the classification head and feat_norm_layer = 1 only (GroupNorm statistics run over time).  Allocation-free:
 * more than float_aud_reserve_segments reserved is refused (FLOAT_E_INVALID).  Bad arguments (n_seg < 1, seg_stride < seg_len,
 * T < 1 with frames set, a segment below the extractor's receptive field, n_seg x L above the frame limit of one call, a
 * handle of the wrong kind) are refused before any HIP call.
 * float_aud_reserve_segments sizes the workspace of float_aud_reserve(seg_len, n_seg x L) plus the stacked extractor buffers;
 * like float_aud_reserve it is the only allocation, never shrinks, synchronises `stream` when it grows, and is not capturable.
 * float_aud_expand_rows (no handle) is F.interpolate(mode="nearest") along time on the device, n rows -> T rows of c floats:
 *   frames[t] = rows[min((int)floorf((float)t * scale), n - 1)],  scale = (float)n / (float)T computed by the caller on the HOST
 * (torch's fp32 form; the exact integer t * n / T picks another row for some pairs, e.g. (n, T) = (2, 82)); n == 1 repeats
 * the row.  It is its own entry so that a clip with a shorter last chunk (scored by float_aud_classify into row n_seg of the
 * same matrix) is expanded by one launch over all its rows. */
enum { FLOAT_AUD_SEG_NORMALIZE = 1 };
int float_aud_reserve_segments(float_aud_t* h, int32_t n_seg, int32_t seg_len, void* stream);
int float_aud_classify_segments(float_aud_t* h, const float* a, int32_t n_seg, int32_t seg_len, int64_t seg_stride, int32_t flags,
                                float* scores /* (n_seg, num_labels) */, float* frames /* (T, num_labels) or NULL */, int32_t T,
                                float scale, void* stream);
int float_aud_expand_rows(const float* rows, int32_t n, int32_t c, float* frames, int32_t T, float scale, void* stream);

/* ---------------------------------------------------------------- misc ------------ */
int float_hip_abi_version(void);
const char* float_last_error(void);
/* The colour matrix `matrix` of the I420 calls as the kernels use it: table = Y, U, V rows of (cr, cg, cb, rnd, off), 15 values
 * (float_dec_frames_i420 above states them).  FLOAT_E_INVALID for an id that is not 0, 2, 4 or 6.  Host only: no HIP call. */
int float_yuv_matrix(int32_t matrix, int32_t table[15]);
/* A HIP stream restricted to CUs [cu_begin, cu_end) (hipExtStreamCreateWithCUMask).  Used to run the FMT
 * chain and the decoder concurrently on disjoint CU sets (pipeline.generate(overlap="cu")). */
int float_stream_create_cu_range(int32_t cu_begin, int32_t cu_end, void** stream_out);
int float_stream_destroy(void* stream);
/* Average device time (ms) of the kernels launched by the last timed call, by class, measured
 * with hipEvents on the caller's stream when profiling is on.  which: 0 = FMT GEMMs of the step chain (weight-streaming
 * tiling), 1 = decoder convs, 2 = the once-per-window adaLN modulation GEMM of the FMT, 3 = FMT GEMMs of a stacked-clip
 * step chain (row-blocked LDS-DMA tiling, float_fmt_sample_batch).  Returns <0 when profiling is off. */
int float_set_profiling(int32_t on);
double float_profile_ms(int32_t which, int64_t* n_launches);
/* Measured peaks of the current device, printed by bench.py beside the spec-sheet peaks of its roofline objects: streaming
 * read and copy (read + write) bandwidth over 2-GiB buffers in GB/s, dense fp16 MFMA rate with register operands
 * (v_mfma_f32_16x16x32_f16 / _32x32x16_f16) in TFLOP/s, compute-unit count.  Allocates and frees 4 GiB; ~0.1 s; synchronises
 * the NULL stream.  Every pointer optional. */
int float_probe_peaks(float* hbm_read_gbps, float* hbm_copy_gbps, float* mfma16_tflops, float* mfma32_tflops, int32_t* n_cu);

/* ---------------------------------------------------------------- comparison ------ */
/* Segment-wise comparison of two fp32 device buffers, for the fp16 precision guard (pipeline.FloatHotPath.verify_precision; no
 * reference counterpart: the reference is fp32).  a, b: n_seg contiguous segments of seg_len elements each, b the trusted side;
 * a segment is one frame (size * size * 3) or one window of latents (n_cur * dim_w).  Any seg_len; a and b need 4-byte
 * alignment only (a slice of a larger tensor): 16-byte loads on the aligned body of each segment, scalar head and tail.
 *   stats: DEVICE memory, n_seg x 5 doubles, per segment
 *     [0] sum of (a - b)^2 over the finite pairs     [1] sum of b^2 over the finite pairs
 *     [2] max |a - b| over the finite pairs          [3] number of finite pairs with |a - b| > thr
 *     [4] number of pairs where a or b is NaN or infinite (excluded from [0..3])
 *   Differences, squares and sums are formed in fp64 from the first add, so a sum is within seg_len * 2^-53 relative of any
 *   other summation order; counts and the maximum are exact.
 *   work: DEVICE scratch of at least float_cmp_work_bytes(n_seg, seg_len) bytes, 8-byte aligned, no zeroing needed: workgroups
 *   write per-(segment, slice) partials there and a second launch folds the slices of each segment in a fixed order - no
 *   floating-point atomics, two calls on the same inputs give bitwise identical stats.
 * Enqueues two kernels on `stream`; allocates nothing, synchronises nothing.  Bad arguments (NULL pointers, n_seg <= 0,
 * seg_len <= 0, misaligned pointers, work_bytes too small) return FLOAT_E_INVALID before any HIP call.
 * float_cmp_work_bytes returns 0 for n_seg <= 0 or seg_len <= 0. */
int float_cmp_segments(const float* a, const float* b, int32_t n_seg, int64_t seg_len, float thr, double* stats, void* work,
                       size_t work_bytes, void* stream);
size_t float_cmp_work_bytes(int32_t n_seg, int64_t seg_len);

/* ---------------------------------------------------------------- audio front end -- */
/* The raw planar waveform of a node's AUDIO input, already in HBM, -> the mono waveform at rate_out (16 kHz) that
 * float_aud_inference / float_aud_classify read: channel mean, band-limited resampling, zero-mean / unit-variance
 * (host_models.preprocess_audio of the host mirror; the reference: librosa soxr_hq + Wav2Vec2FeatureExtractor, generate.py:69-73).
 * With g = gcd(rate_in, rate_out), up = rate_out / g, down = rate_in / g:
 *     x[j]  = mean over channels of w[c * ch_stride + j], 0 <= j < n_in; 0 elsewhere
 *     n_out = ceil(n_in * up / down)                                  = float_aud_front_len(n_in, rate_in, rate_out)
 *     c     = rolloff * min(1, up / down),   pos_m = m * down / up    (an exact rational)
 *     t     = clamp((j - pos_m) * c, -zeros, +zeros)
 *     y[m]  = sum over j of x[j] * sinc(t) * cos^2(pi t / (2 zeros)) * c
 *   (host_models.resample_sinc_direct is this in fp64).  The filter is evaluated where it is used - no polyphase table - so
 *   any pair of rates is served exactly.  rate_in == rate_out: no filter, y is the mono mix, bitwise (sum of the channels in
 *   order, divided by their number).
 *   flags & FLOAT_AUD_FRONT_NORMALIZE: a = (y - mean(y)) / sqrt(var(y) + 1e-7), biased variance, the statistics in fp64 from
 *   per-tile partials added in a fixed order (no atomics: bitwise repeatable); a constant y gives zeros.  Otherwise a = y.
 *   w: channel c starts at w + c * ch_stride (a time slice of a (C, N) tensor needs no copy); 4-byte alignment.
 *   channels 1..8, zeros 1..32, 0 < rolloff <= 1, both rates 1..2^20, 1 <= n_in <= 2^34, n_out == float_aud_front_len(...)
 *   <= 2^34; a pair of rates whose 256-output tile of input does not fit the LDS (rate_in / rate_out * 256 + 2 zeros / c + 3
 *   samples of 4 bytes in 160000 bytes: every ratio from 1/64 to 64 at the default zeros = 24, rolloff = 0.945 fits) is refused.
 *   work: DEVICE scratch of at least float_aud_front_work_bytes(...) bytes, 8-byte aligned, no zeroing needed.
 * Enqueues one kernel on `stream`, three when normalising (tile partials, their fold, the normalisation); allocates nothing,
 * synchronises nothing; kernel launches only, so a caller may capture it (no test captures it; the one host-side call beside
 * the launches is hipFuncSetAttribute, once the staged tile passes 64 KiB).  An argument outside these rules returns
 * FLOAT_E_INVALID, with a message naming the function and the argument, before any HIP call.  float_aud_front_len and float_aud_front_work_bytes return 0 for an invalid argument. */
enum { FLOAT_AUD_FRONT_NORMALIZE = 1 };
int64_t float_aud_front_len(int64_t n_in, int32_t rate_in, int32_t rate_out);
size_t float_aud_front_work_bytes(int64_t n_in, int32_t rate_in, int32_t rate_out);
int float_aud_front(const float* w, int32_t channels, int64_t ch_stride, int64_t n_in, int32_t rate_in, int32_t rate_out,
                    int32_t zeros, float rolloff, int32_t flags, float* a, int64_t n_out, void* work, size_t work_bytes,
                    void* stream);

/* ---------------------------------------------------------------- image front end -- */
/* The raw (src_h, src_w, channels) fp32 tensor of a node's IMAGE input, already in HBM, -> the model's input: RGBA conversion,
 * a window that may reach outside the image (zero border), area resize, 8-bit rounding, normalisation (the reference:
 * img_tensor_2_np_array -> process_img's crop -> cv2.resize(INTER_AREA) -> / 127.5 - 1, utils/image.py, generate.py:29-39).
 * Everything after the quantiser is integer arithmetic, so the result is bitwise the definition in the host mirror
 * (host_models.image_to_rgb8 + host_models.resize_rgb8).
 *   Quantiser, every channel, alpha included: q = trunc(clip(x * 255.0f, 0, 255)) in fp32; NaN gives 0.
 *   channels == 4, rgba_mode:
 *     FLOAT_IMG_RGBA_DISCARD  the RGB as it is
 *     FLOAT_IMG_RGBA_BLEND    trunc(clip(c * (a / 255.0f) + bkg * (1.0f - a / 255.0f), 0, 255)), every operation rounded to fp32 on its
 *                             own (no fused multiply-add)
 *     FLOAT_IMG_RGBA_REPLACE  the background colour where a == 0
 *   Window: samples rect_x ... rect_x + rect_w - 1 by rect_y ... rect_y + rect_h - 1 in source coordinates; a sample outside the
 *   image is 0 in all three channels.
 *   Scale per axis, a rational P / Q reduced by the gcd: scale_num / scale_den on both axes, or, with 0, 0, rect_w / dst_w and
 *   rect_h / dst_h.  With n the window's extent on the axis, source sample i covers [i Q, (i + 1) Q):
 *     area rule (P >= Q on both axes): destination cell d covers [d P, min((d + 1) P, n Q)); a sample's weight is the integer
 *       length of the overlap; out = sum(v wx wy) / (cell length x * cell length y)
 *     linear rule (P < Q on either axis, then on both): sx = floor(d P / Q), num = (d + 1) P - (sx + 1) Q, f = 0 if num <= 0 else
 *       num mod P; if sx >= n - 1 then sx = n - 1, f = 0; taps (sx, P - f) and (min(sx + 1, n - 1), f); out = sum(v wx wy) / (Px Py)
 *     both rounded half to even by one integer division; 32-bit row sums (at most 255 P), 64-bit totals.
 *   out_mode: FLOAT_IMG_OUT_NCHW_PM1  (3, dst_h, dst_w) fp32, q / 127.5f - 1.0f (division, then subtraction)
 *             FLOAT_IMG_OUT_HWC_U8    (dst_h, dst_w, 3) uint8, q
 *   Source sides 1..16384, destination sides 1..4096, window extents and both terms of a reduced scale 1..32768, |rect_x|, |rect_y|
 *   <= 65536; every destination cell must start inside the window ((dst - 1) P < n Q); background channels 0..255.  img and out
 *   are contiguous; img is 16-byte aligned for 4 channels and 4-byte aligned for 3, an fp32 out 4-byte aligned.
 *   work: DEVICE scratch of at least float_img_front_work_bytes(src_h, src_w, dst_h, dst_w) = src_h * dst_w * 12 bytes, 4-byte
 *   aligned, no zeroing needed: (source row, dst_w, 3) int32 row sums.
 * Enqueues two kernels on `stream` (one when the window misses the image): the first reads every source pixel of the window once
 * and writes the row sums, the second forms the outputs; no atomics, two calls give equal bytes.  Allocates nothing,
 * synchronises nothing; kernel launches only, so a caller may capture it (no test captures it).  An argument outside these rules
 * returns FLOAT_E_INVALID, with a message naming the function and the argument, before any HIP call; float_img_front_work_bytes
 * returns 0 for a side out of range. */
enum { FLOAT_IMG_RGBA_DISCARD = 0, FLOAT_IMG_RGBA_BLEND = 1, FLOAT_IMG_RGBA_REPLACE = 2 };
enum { FLOAT_IMG_OUT_NCHW_PM1 = 0, FLOAT_IMG_OUT_HWC_U8 = 1 };
size_t float_img_front_work_bytes(int32_t src_h, int32_t src_w, int32_t dst_h, int32_t dst_w);
int float_img_front(const float* img, int32_t src_h, int32_t src_w, int32_t channels, int32_t rect_x, int32_t rect_y, int32_t rect_w,
                    int32_t rect_h, int32_t scale_num, int32_t scale_den, int32_t rgba_mode, int32_t bkg_r, int32_t bkg_g, int32_t bkg_b,
                    int32_t out_mode, void* out, int32_t dst_h, int32_t dst_w, void* work, size_t work_bytes, void* stream);

/* ---------------------------------------------------------------- paste back -- */
/* The step after the decoder: n_frames generated 8-bit frames (n_frames, fr_h, fr_w, 3) - the buffer float_dec_frames_u8 writes -
 * back in the 8-bit source portrait src8 (src_h, src_w, 3), both in HBM -> out (n_frames, src_h, src_w, 3) uint8.  Integer
 * arithmetic, bitwise the definition in the host mirror, host_models.paste_rgb8:
 *   box     cells rect_x ... rect_x + rect_w - 1 by rect_y ... rect_y + rect_h - 1 in source coordinates; it may reach outside the
 *           image or miss it.  A pixel outside box & image is the source's.  The parts of a frame that map outside the image are
 *           discarded.
 *   face    the frame resized to rect_h x rect_w by the rule of float_img_front above at the scales fr_w / rect_w and fr_h /
 *           rect_h (area rule when both axes shrink or keep their size, else the linear rule on both), rounded half to even.
 *   alpha   d = the cell's distance to the nearest OPEN side of the box (u, rect_w - 1 - u, v, rect_h - 1 - v); a side is open
 *           only where the box edge lies strictly inside the image (rect_x > 0, rect_x + rect_w < src_w, rect_y > 0, rect_y +
 *           rect_h < src_h).  a = min(255, 255 (d + 1) / (feather + 1)) (integer division); no open side or feather == 0: a = 255.
 *   blend   out = (a face + (255 - a) src + 127) / 255 (integer division: round to nearest, 255 is odd).
 * Limits: source and box sides 1 ... 16384, frame sides 1 ... 1024 (with them every sum of the resize fits 32 bits: S <= 255 *
 * 2^20, positions <= 2^24) or, per axis, the box's own side (the scale of that axis is 1: frames that float_img_resample below
 * already brought to the box's size pass at any size the box may have), feather 0 ... 16384, n_frames >= 1, |rect_x|, |rect_y| <= 2^30.  All three pointers are DEVICE
 * pointers to contiguous HWC bytes of any alignment; out must not overlap the inputs.  An output frame is 3 src_h src_w < 2^31
 * bytes; frame bases are formed in 64 bits, so out may exceed 4 GiB.
 * Enqueues one kernel on `stream` (one per 2^30 workgroups: thousands of frames); no scratch, no atomics, allocates nothing,
 * synchronises nothing, two calls give equal bytes.  An argument outside these rules returns FLOAT_E_INVALID, with a message
 * naming the function and the argument, before any HIP call. */
int float_img_paste(const uint8_t* src8, int32_t src_h, int32_t src_w, const uint8_t* frames8, int32_t n_frames, int32_t fr_h,
                    int32_t fr_w, int32_t rect_x, int32_t rect_y, int32_t rect_w, int32_t rect_h, int32_t feather, uint8_t* out,
                    void* stream);

/* The same pasted frames leaving as planar YUV 4:2:0, pasted and converted in one kernel: out is (n_frames, 3 src_h / 2, src_w)
 * uint8 I420 - per frame the Y plane src_h x src_w, then U and V at src_h / 2 x src_w / 2, row-major, contiguous (ffmpeg's
 * yuv420p) - at 1.5 bytes per pixel instead of 3.  Bitwise host_models.paste_i420 = rgb8_to_i420(paste_rgb8(...)): the pasted
 * 8-bit RGB samples are those of float_img_paste above, and from them
 *   Y  = ((66 R + 129 G + 25 B + 128) >> 8) + 16                 per pixel
 *   Mc = (c00 + c01 + c10 + c11 + 2) >> 2                        per 2 x 2 block and channel c of the PASTED samples
 *   U  = ((-38 MR - 74 MG + 112 MB + 128) >> 8) + 128,  V = ((112 MR - 94 MG - 18 MB + 128) >> 8) + 128
 * in int32 with >> the arithmetic shift.  Chroma is not blended: a block that straddles the box edge or the feather averages
 * pasted and source pixels.  `matrix` selects the conversion: the formulas above are FLOAT_IMG_MATRIX_BT601_LIMITED (0); 2, 4 and
 * 6 take the rows of float_dec_frames_i420's table (BT.709 limited, BT.601 full, BT.709 full range) in the same arithmetic, and
 * any other value is FLOAT_E_INVALID.
 * Limits: those of float_img_paste, and src_h, src_w even and >= 2; any even size is taken (1920 x 1080).  The pointers are DEVICE
 * pointers of any alignment; out must not overlap the inputs.  With src_w % 4 == 0 and out 4-byte aligned the kernel stores dwords
 * of Y and 16-bit pairs of U and V, otherwise bytes; the bytes stored are the same.  A frame is 3 src_h src_w / 2 bytes; frame
 * bases are formed in 64 bits.
 * Enqueues one kernel on `stream` (one per 2^30 workgroups of 512 pixels); no scratch, no atomics, allocates nothing, synchronises
 * nothing, two calls give equal bytes.  An argument outside these rules returns FLOAT_E_INVALID, with a message naming the
 * function and the argument, before any HIP call. */
enum { FLOAT_IMG_MATRIX_BT601_LIMITED = 0 };
enum { FLOAT_IMG_MATRIX_BT709_LIMITED = 2, FLOAT_IMG_MATRIX_BT601_FULL = 4, FLOAT_IMG_MATRIX_BT709_FULL = 6 };
int float_img_paste_i420(const uint8_t* src8, int32_t src_h, int32_t src_w, const uint8_t* frames8, int32_t n_frames, int32_t fr_h,
                         int32_t fr_w, int32_t rect_x, int32_t rect_y, int32_t rect_w, int32_t rect_h, int32_t feather, int32_t matrix,
                         uint8_t* out, void* stream);

/* ---------------------------------------------------------------- bicubic / Lanczos resampling -- */
/* n_frames 8-bit RGB frames (n_frames, fr_h, fr_w, 3) in HBM resampled to box_h x box_w by Pillow's Image.resize rule for 8-bit
 * images (src/libImaging/Resample.c) with the BICUBIC or the LANCZOS filter - of which only the window win_x, win_y, win_w, win_h
 * is formed: out is (n_frames, win_h, win_w, 3) uint8.  Bitwise host_models.resample_rgb8 in the host mirror, and through it
 * Pillow 12.2.0.  It is what gives the paste-back routes a filter with negative lobes: the face of float_img_paste above is
 * enlarged by the linear rule, and a caller who wants it sharper resamples the window of the box that lies in the image here and
 * hands float_img_paste the box-sized result (its resize at equal sizes is the identity).
 *
 * One axis n_in -> n_out, output index xx (float_img_resample_plan; C double and libm's sin, no HIP call, usable without a GPU):
 *     scale = n_in / n_out;  fs = max(scale, 1.0);  support = S * fs  (S = 2 bicubic, 3 lanczos);  ss = 1.0 / fs
 *     ksize = (int)ceil(support) * 2 + 1
 *     center = (xx + 0.5) * scale
 *     xmin = max(0, (int)(center - support + 0.5));  xmax = min(n_in, (int)(center + support + 0.5));  n = xmax - xmin
 *     w[x] = f((x + xmin - center + 0.5) * ss), x = 0 ... n - 1;  ww = their sum in that order;  w[x] /= ww if ww != 0
 *     k[x] = (int)(-0.5 + w[x] * 2^22) if w[x] < 0 else (int)(0.5 + w[x] * 2^22);  k[x] = 0 for n <= x < ksize
 *     bicubic (a = -0.5): |x| < 1: ((a + 2) x - (a + 3)) x x + 1;  |x| < 2: (((x - 5) x + 8) x - 4) a;  else 0
 *     lanczos: -3 <= x < 3: sinc(x) sinc(x / 3), sinc(0) = 1, sinc(x) = sin(pi x) / (pi x);  else 0
 * `table` receives, for each of the `count` indices from `first` on, the 2 + ksize int32 values xmin, n, k[0 ... ksize - 1];
 * float_img_resample_plan_ints is count * (2 + ksize), the least table_ints (0 for arguments the planner refuses).  Refused
 * (FLOAT_E_INVALID): a filter other than the two, a size outside 1 ... 2^30, indices outside 0 ... n_out, ksize > 255 (shrinking by
 * more than about 42 x with Lanczos, 63 x with bicubic), a short table.  Every row satisfies 255 sum|k| + 2^21 < 2^31.
 *
 * On the device (float_img_resample), in int32 and with >> the arithmetic shift, no float anywhere:
 *     one axis   out = clamp((2^21 + sum_{x < n} k[x] in[xmin + x]) >> 22, 0, 255)
 *     two axes   the horizontal pass first, over only the input rows the window's rows reference, rounded to 8 bits into `work`;
 *                then the vertical pass.  A pass whose two sizes are equal (fr_w == box_w, fr_h == box_h) is skipped, as in Pillow;
 *                with both equal the window is copied.
 *   tab_x     DEVICE copy of the table of float_img_resample_plan(fr_w, box_w, filter, win_x, win_w, ...); ignored (may be NULL)
 *             when fr_w == box_w.  tab_y: the same of (fr_h, box_h, filter, win_y, win_h).  The kernels trust xmin and n: a table
 *             that was made for other sizes reads outside the frames.
 *   work      DEVICE scratch of at least float_img_resample_work_bytes(...) bytes (0 for arguments the call refuses), 16-byte
 *             aligned, no zeroing needed.
 * Limits: frame and window sides 1 ... 16384, box sides 1 ... 2^30, the window inside the box, n_frames >= 1.  frames8 and out are
 * DEVICE pointers to contiguous HWC bytes of any alignment and must not overlap.  A lane forms four neighbouring pixels; with
 * win_w % 4 == 0 and out 4-byte aligned it stores them as three dwords, otherwise as bytes; the bytes stored are the same.
 * Enqueues at most two kernels on `stream` (per 65535 frames); no atomics, allocates nothing, synchronises nothing, two calls
 * give equal bytes.  An argument outside these rules returns FLOAT_E_INVALID, with a message naming the function and the
 * argument, before any HIP call. */
enum { FLOAT_IMG_FILTER_BICUBIC = 0, FLOAT_IMG_FILTER_LANCZOS = 1 };
size_t float_img_resample_plan_ints(int32_t n_in, int32_t n_out, int32_t filter, int32_t count);
int float_img_resample_plan(int32_t n_in, int32_t n_out, int32_t filter, int32_t first, int32_t count, int32_t* table,
                            size_t table_ints);
size_t float_img_resample_work_bytes(int32_t n_frames, int32_t fr_h, int32_t fr_w, int32_t box_h, int32_t box_w, int32_t filter,
                                     int32_t win_x, int32_t win_y, int32_t win_w, int32_t win_h);
int float_img_resample(const uint8_t* frames8, int32_t n_frames, int32_t fr_h, int32_t fr_w, int32_t box_h, int32_t box_w,
                       int32_t filter, int32_t win_x, int32_t win_y, int32_t win_w, int32_t win_h, const int32_t* tab_x,
                       const int32_t* tab_y, void* work, size_t work_bytes, uint8_t* out, void* stream);

/* ---------------------------------------------------------------- JPEG encoder -- */
/* n_frames 8-bit RGB frames in HBM - the (n, h, w, 3) buffer float_dec_frames_u8 writes - -> n complete baseline JPEG files
 * (JFIF 1.1, 4:2:0, one interleaved scan, the Huffman tables of ITU-T T.81 Annex K.3), back to back in `out`: file i is
 * out[offsets[i] : offsets[i + 1]].  Every step is integer arithmetic, so the bytes are bitwise the definition in the host mirror,
 * host_models.jpeg_encode_rgb8, which states the colour matrix (full-range BT.601), the 2 x 2 chroma mean, the two DCT passes
 * (M = rint(2^14 A)), the quantiser (Annex K.1 / K.2 scaled by `quality`), the entropy coding and the file layout.
 *   h, w      multiples of 16 in 16 ... 16384; quality 1 ... 100
 *   restart   MCUs per restart interval, 0 ... 65535.  The intervals of a frame are coded in parallel, one workgroup each: one
 *             MCU row (w / 16) is the intended value.  0 writes no restart markers: a frame is then one serial chain coded by ONE
 *             workgroup - supported, bitwise the definition, and slow.
 *   out       DEVICE, out_cap bytes.  offsets: DEVICE, n_frames + 1 int64, 8-byte aligned; ALWAYS complete and exact, also when
 *             offsets[n_frames] > out_cap: then nothing at or beyond out + out_cap is written (what lies below is valid), and the
 *             caller reads offsets[n_frames] and calls again with room.
 *   work      DEVICE scratch of at least float_jpg_work_bytes(n_frames, h, w, restart) bytes, 16-byte aligned, no zeroing needed.
 *             Frames are coded in groups of 16 that share it in stream order: with g = min(n_frames, 16) frames, i intervals per
 *             frame and m MCUs per interval it is g i (12 + 2496 m) bytes rounded up - 12 for an interval's length and place, and a
 *             slot of the provable worst case, 6 blocks x 64 coefficients x 26 bits, doubled by byte stuffing (40.9 MB at 512 x 512).
 *   rgb8      2-byte aligned.
 * The header bytes, the quantiser and the Huffman code tables are built on the host inside the call and passed as kernel
 * arguments.  Enqueues three kernels per group on `stream`; allocates nothing, synchronises nothing, kernel launches only; the
 * only atomics are ORs into an LDS bit buffer, so two calls give equal bytes.  An argument outside these rules (a null pointer,
 * a side that is no multiple of 16, a quality outside 1 ... 100, a short or misaligned work) returns FLOAT_E_INVALID, with a
 * message naming the function and the argument, before any HIP call; float_jpg_work_bytes returns 0 for such sizes. */
size_t float_jpg_work_bytes(int32_t n_frames, int32_t h, int32_t w, int32_t restart);
int float_jpg_encode(const uint8_t* rgb8, int32_t n_frames, int32_t h, int32_t w, int32_t quality, int32_t restart, uint8_t* out, size_t out_cap,
                     int64_t* offsets, void* work, size_t work_bytes, void* stream);

/* float_jpg_encode for frames of ANY size, opt-in: h and w in 1 ... 16384, rgb8 of any alignment; everything else - arguments,
 * checks, messages, the capacity rule of `out` and `offsets` - as above.  The scan codes ceil(h / 16) x ceil(w / 16) whole MCUs
 * and sample (y, x) of that area is the source pixel (min(y, h - 1), min(x, w - 1)): the last row and the last column are
 * replicated into the partial MCUs, on RGB, in front of the colour conversion (so a chroma sample is the (sum + 2) >> 2 of the
 * four clamped pixels); SOF0 carries the true h and w and a decoder crops.  Plain replication, not libjpeg's DC-only dummy
 * blocks.  Bitwise host_models.jpeg_encode_rgb8(..., pad="edge"); one MCU row is restart = ceil(w / 16).  `work` holds
 * float_jpg_work_bytes_padded(n_frames, h, w, restart) bytes: the formula above with the rounded-up MCU grid.
 * With both sides multiples of 16 and rgb8 2-byte aligned the call runs the kernels of float_jpg_encode and writes its bytes;
 * otherwise the first stage reads single bytes at clamped coordinates, never outside a frame's h w 3 bytes.
 * float_jpg_encode and float_jpg_work_bytes themselves refuse such sizes as before. */
size_t float_jpg_work_bytes_padded(int32_t n_frames, int32_t h, int32_t w, int32_t restart);
int float_jpg_encode_padded(const uint8_t* rgb8, int32_t n_frames, int32_t h, int32_t w, int32_t quality, int32_t restart, uint8_t* out,
                            size_t out_cap, int64_t* offsets, void* work, size_t work_bytes, void* stream);

/* ---------------------------------------------------------------- PNG encoder -- */
/* n_frames 8-bit RGB frames in HBM -> n complete PNG files (8 bits, colour type 2, no interlace, one IDAT), LOSSLESS, back to
 * back in `out`: file i is out[offsets[i] : offsets[i + 1]].  Every step is integer arithmetic, so the bytes are bitwise the
 * definition in the host mirror, host_models.png_encode_rgb8:
 *   filter    per row the cheapest of the specification's five (bpp = 3, the row above row 0 is zero) by the sum of
 *             min(v, 256 - v) over the row's filtered bytes; ties go to the smallest type.
 *   bands     the filtered rows (1 + 3 w bytes each) are cut into bands of `band` rows, the last one may be short.  A band is ONE
 *             deflate block with a dynamic-Huffman header, coding literals only - no LZ77 matches - followed by an empty stored
 *             block (zlib's sync flush), so every band is an independent, byte-aligned piece, coded by one workgroup.
 *   tables    the block's code is one of 8 FIXED code-length tables over the 256 byte values and end-of-block, the one with the
 *             fewest bits for the band's histogram (ties: the smallest index).  Tables 0 ... 6 suit residuals of growing spread;
 *             table 7 is flat (8 bits; byte value 128 and end-of-block 9).  float_png_tables copies the 8 x 257 lengths out.
 *   stream    78 01, the bands, 01 00 00 FF FF, the Adler-32 of the filtered bytes.
 *   h, w      1 ... 16384.  rgb8 has any alignment.
 *   band      1 ... h rows with band (1 + 3 w) <= 65536; 0 = the default max(1, min(8, h, 65536 / (1 + 3 w))).
 *   out       DEVICE, out_cap bytes.  offsets: DEVICE, n_frames + 1 int64, 8-byte aligned; ALWAYS complete and exact, also when
 *             offsets[n_frames] > out_cap: then nothing at or beyond out + out_cap is written (what lies below is valid), and the
 *             caller reads offsets[n_frames] and calls again with room.
 *   crcs      DEVICE, n_frames uint32, or NULL: per frame the CRC-32 of the zlib stream alone (the IDAT chunk's data), from
 *             which a container writer forms the CRC of any chunk that carries the stream (host_models.crc32_combine) without
 *             reading the data again.
 *   work      DEVICE scratch of at least float_png_work_bytes(n_frames, h, w, band) bytes, 16-byte aligned, no zeroing needed.
 *             Frames are coded in groups of 16 that share it in stream order: with g = min(n_frames, 16) frames and b bands per
 *             frame it is g b (24 + slot) + 256 bytes rounded up.  A slot is the provable worst case of a band of n = band (1 + 3 w)
 *             bytes: the 1106-bit block header, 9 bits per byte (the flat table bounds the chosen one), an end-of-block of at
 *             most 15 bits (9 in the flat table), the stored block's 3 bits, up to 7 bits to the byte boundary and 00 00 FF FF -
 *             (1106 + 9 n + 25) / 8 + 4 bytes, rounded up to 16 (14.3 MB for 16 frames of 512 x 512 at the default band).
 * Not built: LZ77 matching, a code fitted to the frame, a stored-block fallback (the flat table bounds a band at 9 / 8 of its
 * size), 16-bit or RGBA frames.
 * The canonical codes and the CRC tables are compile-time constants of the library.  The CRC-32s of the pieces are combined on
 * the device by multiplication with x^(8 n) modulo the CRC polynomial, as crc32_combine does.  Enqueues three kernels per group on
 * `stream`; allocates nothing, synchronises nothing, kernel launches only; the only atomics are integer adds, ORs and XORs in LDS,
 * so two calls give equal bytes.  An argument outside these rules (a null pointer, a side outside 1 ... 16384, a band above h or
 * of more than 65536 bytes, a short or misaligned work) returns FLOAT_E_INVALID, with a message naming the function and the
 * argument, before any HIP call; float_png_work_bytes returns 0 for such sizes. */
size_t float_png_work_bytes(int32_t n_frames, int32_t h, int32_t w, int32_t band);
int float_png_encode(const uint8_t* rgb8, int32_t n_frames, int32_t h, int32_t w, int32_t band, uint8_t* out, size_t out_cap, int64_t* offsets,
                     uint32_t* crcs, void* work, size_t work_bytes, void* stream);
int float_png_tables(int32_t lengths[8 * 257]);

/* ---------------------------------------------------------------- face detector --- */
/* S3FD (VGG-16 trunk, six detection heads) on the detector's view of the portrait, once per clip: what the reference's
 * process_img (utils/image.py:135-180) asks the `face_alignment` package for.  The definition is host_models.sfd_forward /
 * sfd_decode_dense / sfd_nms / sfd_detect, written from the published network with the package's state-dict keys
 * (`conv1_1.weight` ... `conv7_2_mbox_loc.bias`); parity with the package itself is not pinned.
 *   conv1_1 is a direct kernel on the uint8 view (BGR flip, mean (104, 117, 123), bias, ReLU); every other conv is an implicit
 *   GEMM on MFMA (operands of `dtype`, fp32 accumulation, NHWC); the two heads of a level run as one conv of 8 or 6 channels,
 *   zero-padded to 16; 2 x 2 max-pool (floor mode) and L2Norm (fp32 sums) are kernels of their own.  16-bit stores are
 *   range-tracked (float_sfd_saturation, see float_fmt_saturation).
 *   Post-processing: every position is decoded into dense rows [x1, y1, x2, y2, score] in position order (level, y, x); ONE
 *   workgroup compacts the rows with score > score_thr in that order (prefix scan, no atomic cursor), ranks them by (score
 *   descending, position ascending) and runs the greedy NMS (`+1` areas; dropped when IoU > iou_thr).
 * Views: (H, W, 3) uint8 RGB on the device, 16 <= H <= max_h, 16 <= W <= max_w, both at most 4096.  The workspace lives in the
 * handle and is sized from max_h x max_w at create time; detect / maps / post allocate nothing, synchronise nothing and only
 * launch kernels on `stream`, and two calls on the same view give equal bytes.  A null handle or pointer, or a size outside
 * these rules, returns FLOAT_E_INVALID before any HIP call. */
typedef struct {
  int32_t dtype;           /* FLOAT_DT_* of activations / conv weights (FLOAT_DT_FP32 = verification mode) */
  int32_t max_h, max_w;    /* largest view, each 16 ... 4096 */
  int32_t max_candidates;  /* capacity of the selection kernel, 1 ... 2048 (a face yields tens of candidates) */
  int32_t max_boxes;       /* rows of `boxes`, 1 ... max_candidates */
} float_sfd_cfg_t;

typedef struct float_sfd float_sfd_t;

int float_sfd_create(const float_sfd_cfg_t* cfg, const float_tensor_t* tensors, int32_t n_tensors, float_sfd_t** out);
void float_sfd_destroy(float_sfd_t* h);
/* boxes: (max_boxes, 5) fp32, rows [x1, y1, x2, y2, score] in keep order; counts: 2 x int32 = {kept, candidates}, both device
 * memory.  Both counts are the true numbers: with kept > max_boxes only the first max_boxes rows are written, and with
 * candidates > max_candidates nothing is selected (kept = 0) - the call still succeeds and the dense rows stay valid, so the
 * caller selects from float_sfd_dense with the definition instead (face.FaceDetectorHIP does).  Nothing is truncated silently. */
int float_sfd_detect(float_sfd_t* h, const void* rgb8, int32_t H, int32_t W, float score_thr, float iou_thr, float* boxes, int32_t* counts,
                     void* stream);
/* The verification hook: the 12 maps as sfd_forward returns them (after level 0's max-out, before the softmax), fp32 NCHW in
 * one buffer of 6 P floats, P = the number of positions: per level conf (2, h, w) then loc (4, h, w), levels in order. */
int float_sfd_maps(float_sfd_t* h, const void* rgb8, int32_t H, int32_t W, float* maps12, void* stream);
/* The post-processing alone, on maps in the layout of float_sfd_maps that the caller supplies for an H x W view. */
int float_sfd_post(float_sfd_t* h, const float* maps12, int32_t H, int32_t W, float score_thr, float iou_thr, float* boxes, int32_t* counts,
                   void* stream);
/* The dense rows (P, 5) of the last detect / post call on the handle, copied on `stream`. */
int float_sfd_dense(float_sfd_t* h, float* scores_boxes, void* stream);
int float_sfd_saturation(float_sfd_t* h, uint64_t* total, int32_t reset, void* stream);

/* n stacked views of ONE size in one pass (a batch of portraits behind face_align): rgb8 (n, H, W, 3), maps12 (n, 6 P),
 * boxes (n, max_boxes, 5), counts (n, 2) = {kept, candidates} per view, dense rows (n, P, 5).  The kernels run over n x pixels
 * (the small maps of conv5_* ... conv7_2, 22 x 40 pixels and less at 360 x 640, of several views share 64-pixel tiles), decode runs one grid row per view
 * and the selection one workgroup per view, all in one launch each.  View i of every call is BIT FOR BIT what the single-view
 * call returns for that view alone, in fp16, bf16 and fp32: an output element's accumulation order (taps, then 32-channel
 * steps) does not depend on its place in a tile or in the stack, and nothing is split over K.  Views are independent: one with
 * candidates > max_candidates reports {0, candidates} and its neighbours are selected normally; one with no candidate reports
 * {0, 0}.  The range counter stays one per handle.
 *   float_sfd_reserve_batch grows the handle's workspace to n views of H x W (1 <= n <= 64, H x W within max_h x max_w) and
 * never shrinks it; the largest n, H and W reserved so far are what the other four calls accept.  Of the
 * five calls it alone allocates, and where it has to grow it synchronises the device (the dense rows of an earlier call are then gone); a reservation that cannot be allocated (FLOAT_E_NOMEM) leaves the handle as it was.
 * Per view the workspace is every term of the single view's: two ping-pong activation buffers of H x W x 64 elements (at
 * 360 x 640 in a 16-bit type 29.5 MB each), the L2Norm map (H/4 x W/4 x 256 elements, 7.4 MB), the head output, maps and dense
 * rows (under 2 MB together): about 68 MB per view, 1.1 GB for sixteen views.
 *   The other four return FLOAT_E_INVALID before any HIP call, with a message naming the function and the argument, when n is
 * outside 1 ... the reserved n, when the view exceeds the reserved size, or for a null pointer.  The single-view calls are
 * unchanged; float_sfd_dense after a batched call returns view 0's rows. */
int float_sfd_reserve_batch(float_sfd_t* h, int32_t n, int32_t H, int32_t W);
int float_sfd_maps_batch(float_sfd_t* h, const void* rgb8, int32_t n, int32_t H, int32_t W, float* maps12, void* stream);
int float_sfd_post_batch(float_sfd_t* h, const float* maps12, int32_t n, int32_t H, int32_t W, float score_thr, float iou_thr, float* boxes,
                         int32_t* counts, void* stream);
int float_sfd_detect_batch(float_sfd_t* h, const void* rgb8, int32_t n, int32_t H, int32_t W, float score_thr, float iou_thr, float* boxes,
                           int32_t* counts, void* stream);
int float_sfd_dense_batch(float_sfd_t* h, float* scores_boxes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* FLOAT_HIP_H */
