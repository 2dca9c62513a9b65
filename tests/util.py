"""Shared test helpers: load the hyphen-named package by path, locate fixtures."""
import functools
import importlib.util
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG_DIR = os.path.join(ROOT, "comfyui-float_optimized_amd")
GOLDEN = os.path.join(ROOT, "tests", "golden")
PKG_NAME = "float_amd"


def load_pkg():
    if PKG_NAME in sys.modules:
        return sys.modules[PKG_NAME]
    spec = importlib.util.spec_from_file_location(
        PKG_NAME, os.path.join(PKG_DIR, "__init__.py"), submodule_search_locations=[PKG_DIR])
    mod = importlib.util.module_from_spec(spec)
    sys.modules[PKG_NAME] = mod
    spec.loader.exec_module(mod)
    return mod


def golden(name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    return {k: (torch.from_numpy(z[k]) if z[k].ndim else z[k].item()) for k in z.files}


def golden_parts(name):
    """A fixture that tools/make_goldens.py::save_parts wrote as name_0.npz, name_1.npz, ...: one dict of tensors, the pieces
    `key@i` of a split array concatenated again along its second axis."""
    out, pieces, i = {}, {}, 0
    while os.path.exists(os.path.join(GOLDEN, "%s_%d.npz" % (name, i))):
        for k, v in golden("%s_%d" % (name, i)).items():
            if "@" in k:
                key, j = k.split("@")
                pieces.setdefault(key, {})[int(j)] = v
            else:
                out[k] = v
        i += 1
    assert i > 0, "no fixture %s_0.npz in %s" % (name, GOLDEN)
    for key, p in pieces.items():
        out[key] = torch.cat([p[j] for j in range(len(p))], dim=1)
    return out


def rel_l2(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm() / (b.norm() + 1e-30))


def max_abs(a, b):
    return float((a.double() - b.double()).abs().max())


def seeded_normal(seed, *shape, std=1.0):
    """RandomState(seed).standard_normal(shape) * std as fp32: the input generator of tools/make_goldens.py (`rnd`)."""
    return torch.from_numpy(np.random.RandomState(seed).standard_normal(shape).astype(np.float32) * std)


def sample_inputs(cfg, seed, T, dynamic, noise_seed=15):
    """Inputs of tools/make_goldens.py::gen_fmt_sample regenerated from the seed (the full-length fixtures
    fmt_sample_config2 / config5 hold the reference's r_d only): wa, r_s, we (static softmax vector, or per-window
    vectors nearest-upsampled to T like nodes_vadv.py:829-840), and the reference's sequential noise draws."""
    import math
    L = cfg.num_frames_for_clip
    wa = seeded_normal(seed + 11, 1, T, cfg.dim_a)
    r_s = seeded_normal(seed + 12, 1, cfg.dim_w)
    n_chunks = int(math.ceil(T / L))
    if dynamic:
        we_w = torch.softmax(seeded_normal(seed + 13, 1, n_chunks, cfg.dim_e), -1)
        idx = torch.clamp((torch.arange(T).float() * n_chunks / T).long(), max=n_chunks - 1)
        we = we_w[:, idx]
    else:
        we = torch.softmax(seeded_normal(seed + 13, 1, 1, cfg.dim_e), -1)
    g = torch.Generator("cpu")
    g.manual_seed(int(noise_seed))
    noise = torch.stack([torch.randn(1, L, cfg.dim_w, generator=g) for _ in range(n_chunks)])
    return dict(wa=wa, r_s=r_s, we=we, noise=noise)


# ---- attention unit tests (tests/test_aud_attn.py, tests/test_aud_attn_gpu.py, tests/test_fmt_tables.py) ----
TORCH_DTYPE = {"fp16": torch.float16, "bf16": torch.bfloat16, "fp32": torch.float32}
# (Tn, heads) of the audio attention cases: a single frame; a partial 16-key sub-tile and the clamped loads; a one-key second
# 64-key tile; the production pack stride D / 32 = 24 (hidden 768); several tiles; the second 2048-key tile of the one-wave
# kernel = the 33rd and 34th tile of the matrix-pipe kernel
AUD_ATTN_CASES = [(1, 4), (17, 4), (65, 4), (130, 12), (300, 4), (2049, 4), (2120, 4)]
# 16-bit limits against attention_fp64 of the rounded inputs: at most two roundings of half-ulp size (P where the matrix pipe
# takes it, and the output).  max|d| <= 2 * (ulp / 2) * max|v|: 2^-10 (fp16), 2^-7 (bf16) times max|v|.  Each rounding has an
# rms of 2^-11 / sqrt(3) (2^-8 / sqrt(3)) relative, and two add in quadrature: rel-L2 <= 2^-11 (2^-8).
ATTN_LIMITS = {"fp16": (2.0 ** -10, 2.0 ** -11), "bf16": (2.0 ** -7, 2.0 ** -8)}  # (max|d| / max|v|, rel-L2)


def attn_structural_keys(Tn):
    s = {0, 15, 16, 31, 32, 47, 48, 63, 64, 2047, 2048, 64 * ((Tn - 1) // 64), Tn - 2, Tn - 1}
    return sorted(j for j in s if 0 <= j < Tn)


def peaked_qkv(Tn, heads, head_dim, seed, dtype, pairs=None):
    """Peaked attention inputs: q, k = 2 * N(0,1), v = N(0,1), each (Tn, heads, head_dim) fp32 (logits are N(0, 16)); then key j of
    every pair (i, j[, logit = 24]) is planted on query i in every head: k[j] = q[i] * logit * sqrt(head_dim) / |q[i]|^2, which
    makes logit(i, j) = `logit`.  pairs = None: the n-th structural key (tile and sub-tile edges, attn_structural_keys) goes to
    query (37 n + 5) % Tn.  All three tensors are then rounded to the operand type `dtype` ("fp16" | "bf16" | "fp32"), so input
    rounding is part of no error.  Returns (q, k, v, [(i, j), ...])."""
    shape = (Tn, heads, head_dim)
    q, k, v = 2 * seeded_normal(seed, *shape), 2 * seeded_normal(seed + 1, *shape), seeded_normal(seed + 2, *shape)
    if pairs is None:
        pairs = [((37 * n + 5) % Tn, j) for n, j in enumerate(attn_structural_keys(Tn))]
    assert len({p[1] for p in pairs}) == len(pairs), "a key can be planted on one query only"
    for p in pairs:
        i, j, logit = p[0], p[1], (p[2] if len(p) > 2 else 24.0)
        k[j] = q[i] * (logit * head_dim ** 0.5 / (q[i] * q[i]).sum(-1, keepdim=True))
    td = TORCH_DTYPE[dtype]
    q, k, v = (t.to(td).float() for t in (q, k, v))
    return q, k, v, [(p[0], p[1]) for p in pairs]


def qkv_rows(q, k, v):
    """(Tn, heads, head_dim) x 3 -> the (Tn, 3 * hidden) = [q | k | v] rows the attention hooks take."""
    return torch.cat([t.reshape(t.shape[0], -1) for t in (q, k, v)], dim=1).contiguous()


def attention_probs(q, k, mask=None, dtype=torch.float64):
    """softmax(q k^T / sqrt(head_dim)) per head, (heads, Tn, Tn), in `dtype`; mask (Tn, Tn) bool, True = blocked."""
    q, k = q.to(dtype).transpose(0, 1), k.to(dtype).transpose(0, 1)
    s = q @ k.transpose(1, 2) * (q.shape[-1] ** -0.5)
    if mask is not None:
        s = s.masked_fill(mask[None], float("-inf"))
    return torch.softmax(s, dim=-1)


def attention_fp64(q, k, v, mask=None, dtype=torch.float64):
    """The plain softmax attention in float64 (`dtype` = torch.float32: the same formula in fp32, for the fp32 limit):
    (Tn, heads, head_dim) inputs -> (Tn, heads * head_dim)."""
    o = attention_probs(q, k, mask, dtype) @ v.to(dtype).transpose(0, 1)
    return o.transpose(0, 1).reshape(q.shape[0], -1)


@functools.lru_cache(maxsize=None)
def aud_attn_case(Tn, heads, dtype):
    """One audio attention case, made once per process and shared (read-only) by the CPU and the GPU tests: inputs of
    peaked_qkv (head_dim 64, seed 7000 + Tn), their fp64 reference, the smallest fp64 weight of a planted pair over all heads
    and e32 = max|d| of the same formula evaluated by torch in fp32 (what the fp32 limit is made from)."""
    q, k, v, pairs = peaked_qkv(Tn, heads, 64, 7000 + Tn, dtype)
    p = attention_probs(q, k)
    ref = (p @ v.double().transpose(0, 1)).transpose(0, 1).reshape(Tn, -1)
    wmin = min(float(p[:, i, j].min()) for i, j in pairs)
    return {"q": q, "k": k, "v": v, "pairs": pairs, "ref": ref, "vmax": float(v.abs().max()), "pair_weight": wmin,
            "e32": max_abs(attention_fp64(q, k, v, dtype=torch.float32), ref)}


def attention_16bit_model(q, k, v, dtype, tile=64, drop=(), rescale=True):
    """The matrix-pipe kernel's rounding, modelled in torch - NOT the code under test; it shows that ATTN_LIMITS belong to the
    arithmetic.  fp32 logits; running max and sum over `tile`-key tiles; P rounded to `dtype` before the PV product (its fp32
    values go into the sum); fp32 sums; the result rounded to `dtype`.  Defects for the tests of the limits themselves: keys in
    `drop` are never seen; rescale = False leaves accumulator and sum alone when a tile raises the max."""
    td = TORCH_DTYPE[dtype]
    Tn, hd = q.shape[0], q.shape[-1]
    qh, kh, vh = (t.float().transpose(0, 1) for t in (q, k, v))
    s = qh @ kh.transpose(1, 2) * (hd ** -0.5)
    for j in drop:
        s[:, :, j] = float("-inf")
    m = torch.full(s.shape[:2] + (1,), float("-inf"))
    l, acc = torch.zeros_like(m), torch.zeros_like(qh)
    for j0 in range(0, Tn, tile):
        st = s[:, :, j0:j0 + tile]
        mn = torch.maximum(m, st.max(dim=-1, keepdim=True).values)
        live = torch.isfinite(mn)  # a tile whose every key was dropped, in front of any other
        p = torch.where(live, torch.exp(st - torch.where(live, mn, torch.zeros_like(mn))), torch.zeros_like(st))
        alpha = torch.where(live & torch.isfinite(m), torch.exp(m - mn), torch.zeros_like(m)) if rescale else torch.ones_like(m)
        l = l * alpha + p.sum(dim=-1, keepdim=True)
        acc = acc * alpha + p.to(td).float() @ vh[:, j0:j0 + tile]
        m = mn
    return (acc / l).to(td).float().transpose(0, 1).reshape(Tn, -1)


# ---- decoder geometry cases (tests/test_dec_geometry_gpu.py; their conditioning is pinned by tests/test_oracle_golden.py) ----
DEC_SIZE_FRAMES = 7
# (cin, cout, R_in, upsample): conv16 NT = 2; two 64-channel blocks; zblur to 128 px (4 blocks, partial tile of 16); zblur to
# 256 px (partial tile of 4); dec_zconv4_kernel at full channel count
UNIT_CONV_CASES = [(32, 32, 64, 0), (128, 128, 32, 0), (256, 128, 64, 1), (128, 64, 128, 1), (512, 512, 8, 1)]
# (C, R, prev): PIX = 4 with 8 lanes per pixel and several bands; 256 and 512 channels; a level without a pyramid below it
UNIT_FLOW_CASES = [(64, 64, 1), (256, 64, 1), (512, 8, 1), (64, 128, 0)]
UNIT_SEED = 4100


def dec_size_inputs(size):
    """The inputs of tests/test_dec_sizes_gpu.py: (state dict, feats, s_r (1,512), r_d (1,7,512))."""
    W = load_pkg().weights
    g = torch.Generator().manual_seed(1)
    s_r, r_d = torch.randn(1, 512, generator=g), torch.randn(1, DEC_SIZE_FRAMES, 512, generator=g) * 0.5
    return W.synth_decoder_state(size, seed=3), W.synth_feats(size, seed=3), s_r, r_d


def unit_style():
    return seeded_normal(UNIT_SEED + 1, 2, 512)


def unit_conv_case(i):
    """(state with the StyledConv module's key names, x (2,cin,R,R)) of UNIT_CONV_CASES[i]: the recipe of
    tests/test_dec_units_gpu.py::test_styled_conv_routes.  The up-sampling cases take a low-pass x (noise of R/4, enlarged): the
    blur of a transposed conv of WHITE noise is a sum that cancels, while the rounding of the K = cin sums before it does not -
    the fp32 oracle itself then sits at rel-L2 6.5e-7 of the fp64 one at 512 channels, a third of the fp32 limit."""
    cin, cout, R, up = UNIT_CONV_CASES[i]
    k = UNIT_SEED + 100 * (i + 1)
    rnd = seeded_normal
    sd = {"conv.weight": rnd(k + 2, 1, cout, cin, 3, 3), "conv.modulation.weight": rnd(k + 3, cin, 512),
          "conv.modulation.bias": 1 + rnd(k + 4, cin, std=0.1), "activate.bias": rnd(k + 5, 1, cout, 1, 1, std=0.1)}
    return sd, (smooth_field(k + 6, 2, cin, R, R // 4) if up else rnd(k + 6, 2, cin, R, R))


def smooth_field(seed, n, c, r, lo, hi=0.02):
    """Low-pass random field like weights.synth_feats: (n,c,lo,lo) noise enlarged bilinearly to r x r plus `hi` of white noise."""
    f = torch.nn.functional.interpolate(seeded_normal(seed, n, c, lo, lo), size=(r, r), mode="bilinear", align_corners=False)
    return (f + seeded_normal(seed + 50, n, c, r, r, std=hi)).contiguous()


def unit_flow_case(j):
    """(state with `to_flow.*` / `to_rgb.*` keys, x (2,C,R,R), feat (1,C,R,R), prev_flow, prev_rgb) of UNIT_FLOW_CASES[j]: the
    recipe of tests/test_dec_units_gpu.py::test_flow_level with a low-pass feature map like weights.synth_feats instead of white
    noise, so that the fp32 rounding of a sampling position is not what a limit measures.  ToFlow weight gain 0.3 as there; 0.1
    (the flow_gain of weights.synth_decoder_state) above 64 px, where a rounding of the flow is R / 2 times that in pixels."""
    C, R, prev = UNIT_FLOW_CASES[j]
    k = UNIT_SEED + 1000 * (j + 1)
    rnd = seeded_normal
    sd = {"to_flow.bias": rnd(k + 6, 1, 3, 1, 1, std=0.1),
          "to_flow.conv.weight": rnd(k + 7, 1, 3, C, 1, 1, std=0.3 if R <= 64 else 0.1),
          "to_flow.conv.modulation.weight": rnd(k + 8, C, 512), "to_flow.conv.modulation.bias": 1 + rnd(k + 9, C, std=0.1),
          "to_rgb.bias": rnd(k + 13, 1, 3, 1, 1, std=0.1), "to_rgb.conv.0.weight": rnd(k + 14, 3, C, 1, 1),
          "to_rgb.conv.1.bias": rnd(k + 15, 1, 3, 1, 1, std=0.1)}
    x, feat = rnd(k + 10, 2, C, R, R), smooth_field(k + 11, 1, C, R, max(2, R // 8))
    pflow = rnd(k + 12, 2, 3, R // 2, R // 2, std=0.5) if prev else None
    prgb = rnd(k + 16, 2, 3, R // 2, R // 2) if prev else None
    return sd, x, feat, pflow, prgb


def unit_conv_oracle(i, dtype=torch.float64):
    from oracle import float_oracle as O
    sd, x = unit_conv_case(i)
    return O.styled_conv(x.to(dtype), unit_style().to(dtype), {"c." + k: v for k, v in sd.items()}, "c",
                         bool(UNIT_CONV_CASES[i][3]))


def unit_flow_oracle(j, dtype=torch.float64):
    """{"out": flow (2,3,R,R), "blend": (2,C,R,R), "rgb": (2,3,R,R)} of ToFlow + ToRGB in `dtype`."""
    from oracle import float_oracle as O
    sd, x, feat, pflow, prgb = unit_flow_case(j)
    cast = lambda t: None if t is None else t.to(dtype)  # noqa: E731
    fw, bl, o3, _ = O.to_flow(cast(x), unit_style().to(dtype), feat.repeat(2, 1, 1, 1), sd, "to_flow", cast(pflow))
    return {"out": o3, "blend": bl, "rgb": O.to_rgb(fw, sd, "to_rgb", cast(prgb))}
