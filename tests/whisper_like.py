"""Inputs with the statistics of a pretrained Whisper encoder, and the yardsticks the kernels are held to on them.

Numpy only, no test functions.  ``synth.encoder_state_dict`` and the per-kernel tests draw everything Gaussian and
well-conditioned; a pretrained encoder has a few residual-stream channels in the hundreds, LayerNorm gains over two orders
of magnitude (near zero on those channels), fc1 pre-activations in the tens and attention sinks.  The generators here
produce that, deterministically; ``ideal_bf16_error`` / ``noise_bound`` state what a LayerNorm-folded bf16 projection may
cost on such rows from the inputs alone, and ``emulate_prefix_shift`` restates the algebra gemm_astat.hip and mlp_fused.hip
document (so the bounds can be checked against the design without a GPU).
"""

from __future__ import annotations

import numpy as np

from gw_whisper_amd import synth
from oracle import encoder as oenc

LN_EPS = 1e-5
PREFIX = 32                      # columns the kernels take their shift from
LOG2E = 1.4426950408889634

FAMILIES = ("gauss", "out_in32", "out_late", "slope", "block32", "gains", "whisperlike", "nearconst", "degenerate", "out_col0")
FC1_BIAS_HEAD = (12.0, -12.0, 20.0, -20.0, 9.0, -9.0, 30.0, -30.0)
# pre-activations of the GELU sweeps: both sides of the |z| = 8 clamp of the sigmoid forms, the saturated tails, and the bulk
GELU_Z_FIXED = (-40.0, -30.0, -12.5, -9.0, -8.01, -7.99, -6.0, 6.0, 7.99, 8.01, 9.0, 12.5, 30.0, 40.0, 100.0)


def bf(x):
    """fp32 values rounded to bf16 (returned as fp32)."""
    return oenc.bf16_round(np.asarray(x, np.float32))


def outlier_channels(d: int):
    """One outlier channel inside the 32-column prefix, one outside."""
    return [5, d // 2 + 8]


def _log_uniform(rng, lo, hi, n):
    return np.exp(rng.uniform(np.log(lo), np.log(hi), n))


def whisper_like_state_dict(d: int, L: int, H: int, F: int, seed: int, n_mels: int = 80) -> dict:
    """``synth.encoder_state_dict`` reshaped towards a pretrained encoder: two outlier channels that fc2 drives harder
    layer by layer, LayerNorm gains log-uniform over [0.05, 4] and 0.02 on the outlier channels, sharper attention (q and k
    doubled), fc1 biases that put pre-activations at +-9 .. +-30.  float32, deterministic from ``seed``."""
    sd = {k: v.copy() for k, v in synth.encoder_state_dict(d, L, H, F, seed=seed, n_mels=n_mels).items()}
    rng = np.random.default_rng(seed + 90001)
    oc = outlier_channels(d)

    def gain():
        g = _log_uniform(rng, 0.05, 4.0, d)
        g[oc] = 0.02
        return g.astype(np.float32)

    for i in range(L):
        p = f"layers.{i}."
        sd[p + "fc2.bias"][oc[0]] += 40.0 * (i + 1)
        sd[p + "fc2.bias"][oc[1]] -= 25.0 * (i + 1)
        sd[p + "fc2.weight"][oc, :] *= 6.0
        for ln in ("self_attn_layer_norm", "final_layer_norm"):
            sd[p + ln + ".weight"] = gain()
            sd[p + ln + ".bias"] = (0.5 * rng.standard_normal(d)).astype(np.float32)
        sd[p + "self_attn.q_proj.weight"] *= 2.0
        sd[p + "self_attn.k_proj.weight"] *= 2.0
        sd[p + "fc1.bias"] += rng.standard_normal(F).astype(np.float32)
        sd[p + "fc1.bias"][:8] = FC1_BIAS_HEAD
    sd["embed_positions.weight"][:, oc[0]] += 30.0
    sd["layer_norm.weight"] = gain()
    assert all(v.dtype == np.float32 for v in sd.values())
    return sd


def activation_families(rng, M: int, K: int) -> dict:
    """name -> (x [M, K], ln_w [K], ln_b [K]), float32: residual-stream rows a 32-column prefix does not represent, gains
    far from one, and rows without a spread."""
    def base():
        return (rng.standard_normal((M, K)) * 2 + 0.3, 1 + 0.1 * rng.standard_normal(K), 0.1 * rng.standard_normal(K))

    out = {}
    out["gauss"] = base()
    x, g, b = base()
    x[:, 5], x[:, 200] = 150.0, -90.0
    out["out_in32"] = (x, g, b)
    x, g, b = base()
    x[:, 100], x[:, 200] = 150.0, -90.0
    out["out_late"] = (x, g, b)
    x, g, b = base()
    out["slope"] = (x + np.linspace(-20.0, 20.0, K), g, b)
    x, g, b = base()
    x[:, :PREFIX] += 40.0
    out["block32"] = (x, g, b)
    x, g, b = base()
    g = _log_uniform(rng, 0.01, 10.0, K)
    g[rng.permutation(K)[:K // 4]] *= -1.0
    out["gains"] = (x, g, b)
    x, g, b = base()
    x[:, 5], x[:, 200] = 150.0, -90.0
    x += np.linspace(-5.0, 5.0, K)
    g = _log_uniform(rng, 0.05, 5.0, K)
    g[5], g[200] = 0.02, 0.03
    out["whisperlike"] = (x, g, b)
    x, g, b = base()
    out["nearconst"] = (7.0 + 1e-3 * rng.standard_normal((M, K)), g, b)
    x, g, b = base()
    x[:] = 0.0
    x[0::3] = 3.25                         # exactly constant rows
    x[2::3, 0] = 100.0                     # a single nonzero element (rows 1, 4, ... stay all zero)
    out["degenerate"] = (x, g, b)
    # beyond the issue's list: the outlier in column 0 itself -- harmless under the prefix-mean shift (amp 1.06), but a
    # shift by the row's first element would leave every other column at -150 (emulated: 7 x the rms limit)
    x, g, b = base()
    x[:, 0] = 150.0
    out["out_col0"] = (x, g, b)
    assert tuple(out) == FAMILIES
    return {k: tuple(np.ascontiguousarray(a, dtype=np.float32) for a in v) for k, v in out.items()}


def constant_rows(x) -> np.ndarray:
    """Mask of the rows whose elements are all equal (LayerNorm maps them to its bias: the projection is ``cb``)."""
    x = np.asarray(x)
    return (x == x[:, :1]).all(axis=1)


def _xhat(x):
    x = np.asarray(x, np.float64)
    mu = x.mean(axis=1, keepdims=True)
    var = ((x - mu) ** 2).mean(axis=1, keepdims=True)
    return (x - mu) / np.sqrt(var + LN_EPS), mu[:, 0], var[:, 0]


def folded(ln_w, ln_b, W, bias):
    """(W' = bf16(g W) as fp64, u = sum_k W', cb = bias + W b_ln) -- what ``ops.ln_fold_weights`` builds."""
    W = np.asarray(W, np.float32)
    Wf = bf(W * np.asarray(ln_w, np.float32)[None, :]).astype(np.float64)
    cb = np.asarray(bias, np.float64) + W.astype(np.float64) @ np.asarray(ln_b, np.float64)
    return Wf, Wf.sum(axis=1), cb


def ideal_bf16_error(x, ln_w, ln_b, W, bias, gelu: bool = False):
    """(ref, err): the fp64 reference ``LayerNorm(x) W^T + bias`` and the error of the ideal bf16 pipeline
    ``bf16(xhat) bf16(g W)^T + cb`` (evaluated in fp64) against it; ``gelu`` applies the exact GELU to both."""
    xh, _, _ = _xhat(x)
    W64 = np.asarray(W, np.float64)
    ref = (xh * np.asarray(ln_w, np.float64) + np.asarray(ln_b, np.float64)) @ W64.T + np.asarray(bias, np.float64)
    Wf, _, cb = folded(ln_w, ln_b, W, bias)
    ideal = bf(xh).astype(np.float64) @ Wf.T + cb
    if gelu:
        ref, ideal = oenc.gelu(ref), oenc.gelu(ideal)
    return ref, ideal - ref


def noise_bound(x, ln_w, ln_b, W, bias):
    """(amp [M], b [M, N]).  ``b_mn = 2^-9 sqrt(sum_k xhat_mk^2 W'_nk^2)`` is the scale of one bf16 operand rounding in
    output element (m, n); ``amp_m = sqrt(1 + D_m^2 / (2 s_m^2))`` is what a shift by the mean of the row's first 32 columns
    (instead of the row mean) may add to it: D_m = prefix mean - row mean, s_m^2 = row variance + eps.  Both come from
    the inputs alone: amp is the contract the kernel headers document, not a measurement of a kernel."""
    del bias
    xh, mu, var = _xhat(x)
    Wf = bf(np.asarray(W, np.float32) * np.asarray(ln_w, np.float32)[None, :]).astype(np.float64)
    b = 2.0 ** -9 * np.sqrt((xh * xh) @ (Wf * Wf).T)
    D = np.asarray(x, np.float64)[:, :PREFIX].mean(axis=1) - mu
    return np.sqrt(1.0 + D * D / (2.0 * (var + LN_EPS))), b


def emulate_prefix_shift(x, ln_w, ln_b, W, bias, shift: str = "prefix", gelu: bool = False, normalise: bool = False,
                         round_out: bool = False):
    """The algebra gemm_astat.hip (AMODE_LN) documents, in fp64 except where the kernel rounds: c = fp32 shift,
    v = fp32(x - c), one-pass fp32 statistics mean' = sum v / K, var = max(sum v^2 / K - mean'^2, 0), operand bf16(v),
    out = rstd (a W'^T - mean' u) + cb.  ``shift``: "prefix" (the kernels), "first" (the row's first element) or "none" --
    the regressions the bounds must catch.  ``normalise``: mlp_fused.hip's panel form (GWW_MF_NORM), the operand rounded a
    second time, a^ = bf16(fp32(a rstd - mean' rstd)), out = a^ W'^T + cb.  ``round_out``: the bf16 store of the result."""
    x = np.asarray(x, np.float32)
    K = x.shape[1]
    if shift == "prefix":
        c = x[:, :PREFIX].astype(np.float64).mean(axis=1).astype(np.float32)
    elif shift == "first":
        c = x[:, 0].copy()
    else:
        c = np.zeros(x.shape[0], np.float32)
    v = (x - c[:, None]).astype(np.float32)
    v64 = v.astype(np.float64)
    mean = (v64.sum(axis=1) / K).astype(np.float32).astype(np.float64)
    s2 = ((v64 * v64).sum(axis=1) / K).astype(np.float32).astype(np.float64)
    var = np.maximum((s2 - mean * mean).astype(np.float32).astype(np.float64), 0.0)
    rstd = (1.0 / np.sqrt(var + LN_EPS)).astype(np.float32).astype(np.float64)
    Wf, u, cb = folded(ln_w, ln_b, W, bias)
    if normalise:
        r32, nm32 = rstd.astype(np.float32)[:, None], (-mean * rstd).astype(np.float32)[:, None]
        out = bf((bf(v).astype(np.float64) * r32 + nm32).astype(np.float32)).astype(np.float64) @ Wf.T + cb
    else:
        out = rstd[:, None] * (bf(v).astype(np.float64) @ Wf.T - mean[:, None] * u[None, :]) + cb
    out = oenc.gelu(out) if gelu else out
    return bf(out).astype(np.float64) if round_out else out


def mlp_fp64(xn, ln_w, ln_b, W1, b1, W2, b2):
    """fc2(gelu(fc1(LayerNorm(xn)))) in fp64 (HF:modeling_whisper.py:401-405 without the residual add)."""
    xh, _, _ = _xhat(xn)
    h = oenc.gelu((xh * np.asarray(ln_w, np.float64) + np.asarray(ln_b, np.float64)) @ np.asarray(W1, np.float64).T
                  + np.asarray(b1, np.float64))
    return h @ np.asarray(W2, np.float64).T + np.asarray(b2, np.float64)


def mlp_bf16_operands(xn, ln_w, ln_b, W1, b1, W2, b2, kernel_like: bool = False):
    """The same in fp64 with bf16-rounded operands at the two GEMM inputs: bf16(xhat), bf16(g W1); bf16(gelu), bf16(W2) --
    the yardstick of the MLP delta's rms error.  ``kernel_like``: the first GEMM as mlp_fused.hip forms it instead
    (prefix shift, second operand rounding), to tell on the CPU whether the design itself meets a bound."""
    if kernel_like:
        h = emulate_prefix_shift(xn, ln_w, ln_b, W1, b1, gelu=True, normalise=True)
    else:
        xh, _, _ = _xhat(xn)
        Wf, _, cb = folded(ln_w, ln_b, W1, b1)
        h = oenc.gelu(bf(xh).astype(np.float64) @ Wf.T + cb)
    return bf(h).astype(np.float64) @ bf(W2).astype(np.float64).T + np.asarray(b2, np.float64)


def check_folded_projection(got, x, ln_w, ln_b, W, bias, gelu: bool = False):
    """The two bounds a LayerNorm-folded projection is held to on any input: returns (rms ratio, worst per-element ratio,
    ok_rms, ok_elem).  rms error <= 1.5 rms_m(amp_m) x the ideal pipeline's rms error (1.5: a second operand rounding,
    sqrt(3/2), and the bf16 output rounding); |err_mn| <= 10 amp_m b_mn + 2^-8 |ref_mn| + 1e-3."""
    ref, ierr = ideal_bf16_error(x, ln_w, ln_b, W, bias, gelu=gelu)
    amp, b = noise_bound(x, ln_w, ln_b, W, bias)
    err = np.asarray(got, np.float64) - ref
    rms = lambda a: float(np.sqrt((a * a).mean()))
    lim_rms = 1.5 * rms(amp) * rms(ierr)
    lim = 10.0 * amp[:, None] * b + 2.0 ** -8 * np.abs(ref) + 1e-3
    # (a family whose ideal error is exactly zero -- constant rows only -- has nothing to be relative to)
    r_rms = rms(err) / lim_rms if lim_rms > 0 else (0.0 if rms(err) == 0 else np.inf)
    excess = (np.abs(err) - 2.0 ** -8 * np.abs(ref) - 1e-3) / np.maximum(amp[:, None] * b, 1e-30)
    return r_rms, float(excess.max()), rms(err) <= lim_rms, bool((np.abs(err) <= lim).all())


def gelu_sweep_z(rng, n: int) -> np.ndarray:
    """n pre-activations (n >= 79): the fixed values around and beyond the |z| = 8 clamp, 64 random values in [-10, 10],
    the rest a cyclic repeat -- float32."""
    z = np.concatenate([np.asarray(GELU_Z_FIXED), rng.uniform(-10.0, 10.0, 64)])
    assert n >= z.size
    return np.resize(z, n).astype(np.float32)


def to_log2q(qkv):
    """q section scaled by log2(e) and rounded to bf16 once: what the LN-folded q panel of the fast path produces."""
    d = qkv.shape[-1] // 3
    out = qkv.copy()
    out[..., :d] = bf(qkv[..., :d].astype(np.float64) * LOG2E)
    return out


def attn_ref_log2q(qkv_l2, H):
    """oracle/encoder.py::attention (bf16 emulation: un-normalised bf16 P, fp32 row sum) on q / log2(e) -- restated here
    because the oracle would round that quotient to bf16 again."""
    B, Tn, d3 = qkv_l2.shape
    d = d3 // 3
    x = qkv_l2.astype(np.float64)
    heads = lambda a: a.reshape(B, Tn, H, 64).transpose(0, 2, 1, 3)
    q, k, v = heads(x[..., :d] / LOG2E), heads(x[..., d:2 * d]), heads(x[..., 2 * d:])
    s = np.matmul(q, k.transpose(0, 1, 3, 2))
    p = np.exp(s - s.max(axis=-1, keepdims=True))
    o = np.matmul(bf(p.astype(np.float32)).astype(np.float64), v) / p.sum(axis=-1, keepdims=True)
    return o.transpose(0, 2, 1, 3).reshape(B, Tn, d)


def lse_ref_log2q(qkv_l2, H):
    """Natural-log row log-sum-exp [B, H, T] of the same scores, fp64."""
    B, Tn, d3 = qkv_l2.shape
    d = d3 // 3
    x = qkv_l2.astype(np.float64)
    heads = lambda a: a.reshape(B, Tn, H, 64).transpose(0, 2, 1, 3)
    s = np.matmul(heads(x[..., :d] / LOG2E), heads(x[..., d:2 * d]).transpose(0, 1, 3, 2))
    m = s.max(axis=-1, keepdims=True)
    return (m + np.log(np.exp(s - m).sum(axis=-1, keepdims=True)))[..., 0]


def sink_qkv(rng, B: int, Tn: int, H: int, s: float, bland: int):
    """(qkv fp32 [B, Tn, 3 H 64], peaked): ``randn * 0.4``; in every head but ``bland`` channel 0 of q is 1 and channel 0 of
    k is ``s`` on the sink keys {0, Tn - 1} (0 elsewhere), so every query scores them ``s`` above the rest; two rows per head
    attend one mid-sequence key with score 60 (beyond the sinks).  ``peaked`` lists (head, query row, key row)."""
    d = H * 64
    qkv = (rng.standard_normal((B, Tn, 3 * d)) * 0.4).astype(np.float32)
    peaked = []
    for h in range(H):
        if h == bland:
            continue
        qc, kc = h * 64, d + h * 64
        qkv[:, :, qc] = 1.0
        qkv[:, :, kc] = 0.0
        qkv[:, [0, Tn - 1], kc] = s
        rows = ((18 + 3 * h, Tn // 2 + h), (Tn - 40 - 2 * h, Tn // 3 + 2 * h + 1))
        for qr, kr in rows:
            # q row and k row share a +-sqrt(60 / 63) pattern on channels 1 .. 63 (channel 0 stays the sink channel):
            # score 60 with the chosen key, O(1) with every other
            pat = np.where(rng.random(63) < 0.5, -1.0, 1.0) * np.sqrt(60.0 / 63.0)
            qkv[:, qr, qc + 1:qc + 64] = pat
            qkv[:, kr, kc + 1:kc + 64] = pat
            peaked.append((h, qr, kr))
    return qkv, peaked
