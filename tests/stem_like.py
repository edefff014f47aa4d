"""The conv-stem backward on impulse gradients: the case table, the fp64 reference and its
per-element scale, a host emulation of the bf16 / fp32 chains that rounds where the kernels store, the modelled defects,
and the ctypes call of the C entries.  Shared by tests/test_stem_like_host.py (CPU) and tests/test_gpu_stem_like.py.

Layout the kernels work on (gw_whisper_amd/csrc/train_ops.hip, gw_whisper_amd/csrc/encoder_train.hip), restated here for the emulation:
  melT  [B (Tin + 2), C]   token-major, per segment: a zero row, the Tin frames, a zero row
  c1    [B (Tin + 2), d]   conv1 output frame t1 at padded row t1 + 1, pad rows zero
  conv2 rows b (T + 1) + t read padded c1 rows 2 t .. 2 t + 2; row t = T of every segment is junk and carries dz2 = 0
  col   [B (T + 1), 3, d]  col[b, t][k] = dz2[b, t] W2[:, :, k];   dz1 frame t1 (p = t1 + 1):
        p odd: col[b, (p - 1) / 2][1];   p even: col[b, p / 2][0] (only when p / 2 < T) + col[b, p / 2 - 1][2]
  col1  [B (Tin + 2), 3, C] col1[b, t1][k] = dz1[b, t1] W1[:, :, k];   dmel[b, c, tau] = sum_k col1[b, tau + 1 - k][k][c]
"""

import functools
import math

import numpy as np

from gw_whisper_amd import synth

# case -> (d, mels, T, B); every encoder has one layer (heads and ffn of the width below)
CASES = {1: (128, 80, 16, 1), 2: (128, 80, 33, 2), 3: (128, 80, 100, 3), 4: (384, 80, 33, 2), 5: (512, 80, 33, 2),
         6: (1280, 128, 16, 2), 7: (128, 80, 1500, 2)}
WIDTHS = {128: (2, 512), 384: (6, 1536), 512: (8, 2048), 1280: (20, 5120)}
REGIMES = ("synth", "sat")        # synth-scaled stem weights | conv biases of +-6 (gelu' is 1 or 0 on most channels)
PATTERNS = ("first", "last", "seam", "seg1", "dense")
POOLED_CASE = 2                   # the pooled entry (d_hidden [B, d], live at token T - 1 of every segment) runs here

# Absolute accuracy of the device's gelu' near zero slope, as a floor under |gelu'| in the additive term E of the conv
# gradients' bound:
# Abramowitz-Stegun 7.1.26 bounds erf to 1.5e-7, so Phi to 0.75e-7; the fp32 roundings of erf_abs (near 1), of
# 0.5 + z phi(z) and of the final sum add three half-ulps of numbers <= 1 (0.9e-7); v_exp_f32 / v_rcp_f32 are 1 ulp.
# Twice that sum:
GELU_ABS = 2.0 ** -21


def patterns_of(case):
    d, C, Tn, B = CASES[case]
    if case == 7:
        return ("dense", "first", "last")
    return tuple(p for p in PATTERNS if (p != "seam" or Tn >= 33) and (p != "seg1" or B >= 2))


def table():
    """Every (case, pattern) of CASES and patterns_of."""
    return [(c, p) for c in CASES for p in patterns_of(c)]


def live_tokens(case, pattern):
    """[(segment, token)] that carry a gradient; None for the dense pattern."""
    d, C, Tn, B = CASES[case]
    return {"first": [(0, 0)], "last": [(B - 1, Tn - 1)], "seam": [(0, 31), (0, 32)], "seg1": [(1, 0)],
            "pooled": [(b, Tn - 1) for b in range(B)], "dense": None}[pattern]


def bf16_round(x):
    """float array -> the nearest bf16 values (ties to even), as float32."""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    u = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16
    return u.astype(np.uint32).view(np.float32)


@functools.lru_cache(maxsize=None)
def weights(case, regime):
    """Seeded one-layer encoder that is the identity above the stem (out_proj and fc2 zero), conv weights already
    bf16 values, position table cut to T.  Read-only."""
    d, C, Tn, B = CASES[case]
    H, F = WIDTHS[d]
    sd = synth.encoder_state_dict(d, 1, H, F, seed=340 + case, n_mels=C)
    sd["embed_positions.weight"] = sd["embed_positions.weight"][:Tn].copy()
    for k in ("conv1.weight", "conv2.weight"):
        sd[k] = bf16_round(sd[k])
    if regime == "sat":
        rng = np.random.default_rng(3400 + case)
        for k in ("conv1.bias", "conv2.bias"):
            sd[k] = np.where(rng.random(d) < 0.5, -6.0, 6.0).astype(np.float32)
    for k in ("out_proj.weight", "out_proj.bias"):
        sd["layers.0.self_attn." + k][...] = 0
    for k in ("fc2.weight", "fc2.bias"):
        sd["layers.0." + k][...] = 0
    for v in sd.values():
        v.setflags(write=False)
    return sd


@functools.lru_cache(maxsize=None)
def features(case):
    """Log-mel stand-in [B, C, 2 T] in Whisper's normalised range, drawn already rounded to bf16."""
    d, C, Tn, B = CASES[case]
    m = np.clip(np.random.default_rng(34 + case).standard_normal((B, C, 2 * Tn)) * 0.5, -1.5, 1.5)
    m = bf16_round(m)
    m.setflags(write=False)
    return m


def impulse(case, pattern, seed=0):
    """fp32 [B, T, d] (pooled: [B, d]): Gaussian rows at the pattern's live tokens, exact zeros elsewhere.  The GPU tests
    feed it as d_hidden; the host tests use it as the d_x0 that enters the stem."""
    d, C, Tn, B = CASES[case]
    rng = np.random.default_rng(1000 * case + 7 * seed + len(pattern))
    if pattern == "pooled":
        return rng.standard_normal((B, d)).astype(np.float32)
    g = rng.standard_normal((B, Tn, d)).astype(np.float32)
    live = live_tokens(case, pattern)
    if live is None:
        return g
    out = np.zeros_like(g)
    for b, t in live:
        out[b, t] = g[b, t]
    return out


def live_mask(case, pattern):
    """bool [B, T]: the tokens that may carry a gradient."""
    d, C, Tn, B = CASES[case]
    live = live_tokens(case, pattern)
    m = np.zeros((B, Tn), bool)
    if live is None:
        m[...] = True
    else:
        for b, t in live:
            m[b, t] = True
    return m


# ---------------------------------------------------------------- fp64 reference and scale (plain conv1d autograd)
def _gelu(T, z):
    """The exact erf GELU as z Phi(z) with Phi = erfc(-z / sqrt 2) / 2: 1 + erf cancels in the lower tail, where fp64
    autograd of nn.functional.gelu is then good to 1e-16 absolutely but not relatively."""
    return 0.5 * z * T.erfc(-z / math.sqrt(2.0))


def _gelu_grad(T, z):
    return 0.5 * T.erfc(-z / math.sqrt(2.0)) + z * T.exp(-0.5 * z * z) / math.sqrt(2.0 * math.pi)


def _stem64(T, sd, mel):
    f = T.nn.functional
    p = {k: T.from_numpy(np.array(sd[k])).double().requires_grad_(True)
         for k in ("conv1.weight", "conv1.bias", "conv2.weight", "conv2.bias")}
    m = T.from_numpy(np.array(mel)).double().requires_grad_(True)
    z1 = f.conv1d(m, p["conv1.weight"], p["conv1.bias"], padding=1)
    c1 = _gelu(T, z1)
    z2 = f.conv1d(c1, p["conv2.weight"], p["conv2.bias"], stride=2, padding=1)
    return p, m, z1, c1, z2, _gelu(T, z2).transpose(1, 2)


NAMES = ("d_mel", "conv1.weight", "conv1.bias", "conv2.weight", "conv2.bias", "embed_positions.weight")


def reference(T, sd, mel, d_x0):
    """{name: fp64 numpy} of NAMES: the derivative of sum(gelu(conv2(gelu(conv1(mel)))) * d_x0), exact erf GELU."""
    p, m, z1, c1, z2, x0 = _stem64(T, sd, mel)
    g = T.from_numpy(np.asarray(d_x0)).double()
    (x0 * g).sum().backward()
    out = {k: v.grad.numpy() for k, v in p.items()}
    out["d_mel"] = m.grad.numpy()
    out["embed_positions.weight"] = g.sum(0).numpy()
    return out


def scale(T, sd, mel, d_x0, floor=0.0, zround=0.0, z2_too=True):
    """{name: fp64 numpy}: the absolute-value sum of every term of each element -- the same chain with |d_x0|, |gelu'|
    and |W| through the two transposed convolutions; for a weight gradient the sum over rows of |dz| |input|, |dz| from
    that chain.  ``floor`` and ``zround`` widen the two activation factors for the additive term E of the bound:
    |gelu'(z)| + floor + dz |gelu''(z)| and |c1| + e1, where e1 = floor |z1| + zround (|c1| + |z1| |gelu'(z1)|) is c1's
    own error (stored to a relative ``zround`` from a z1 stored likewise), dz1 = zround |z1|, and
    dz2 = zround |z2| + 4 sqrt(sum W2^2 e1^2): the storage of z2 plus what the independent errors of the 3 d entries of
    c1 under it add up to, as a root-sum-square (4 x the rss of maximal errors is 7 standard deviations of uniform ones;
    their plain sum would be sqrt(3 d) larger than any z2 error that occurs).  ``z2_too`` False leaves z2's uncertainty out."""
    f = T.nn.functional
    with T.no_grad():
        p, m, z1, c1, z2, _ = _stem64(T, sd, mel)
        g = T.from_numpy(np.asarray(d_x0)).double().abs().transpose(1, 2)              # [B, d, T]
        w1, w2 = p["conv1.weight"].abs(), p["conv2.weight"].abs()
        phi = lambda z: T.exp(-0.5 * z * z) / math.sqrt(2.0 * math.pi)
        slope = lambda z, dz: _gelu_grad(T, z).abs() + floor + dz * (phi(z) * (2.0 - z * z)).abs()
        e1 = floor * z1.abs() + zround * (c1.abs() + z1.abs() * _gelu_grad(T, z1).abs())
        dz2 = g * slope(z2, (zround * z2.abs() + 4.0 * f.conv1d(e1 * e1, w2 * w2, stride=2, padding=1).sqrt()) * bool(z2_too))
        dc1 = f.conv_transpose1d(dz2, w2, stride=2, padding=1, output_padding=1)
        dz1 = dc1 * slope(z1, zround * z1.abs())
        s_mel = f.conv_transpose1d(dz1, w1, padding=1)
        Tin, Tn = m.shape[2], z2.shape[2]
        melp = f.pad(m.abs(), (1, 1))
        c1p = f.pad(c1.abs() + e1, (1, 1))
        s_w1 = T.stack([T.einsum("bot,bct->oc", dz1, melp[:, :, k:k + Tin]) for k in range(3)], 2)
        s_w2 = T.stack([T.einsum("bot,bct->oc", dz2, c1p[:, :, k:k + 2 * Tn:2]) for k in range(3)], 2)
        return {"d_mel": s_mel.numpy(), "conv1.weight": s_w1.numpy(), "conv1.bias": dz1.sum((0, 2)).numpy(),
                "conv2.weight": s_w2.numpy(), "conv2.bias": dz2.sum((0, 2)).numpy(),
                "embed_positions.weight": g.transpose(1, 2).sum(0).numpy()}


def scales(T, sd, mel, d_x0, precision, weight_grads=True):
    """(S, S + E) of the bound |got - ref| <= c S + E.  E is zero for d_mel and embed_positions (RAW_RATIO): their
    elements sum over all channels and c S alone holds.  For the conv gradients E is S's growth under the activation errors
    no c can carry, because under an impulse an element of a weight gradient is ONE product whose gelu' may sit at its
    zero (z = -0.75) or in its lower tail: GELU_ABS, and the bf16 storage (relative 2^-9) of the pre-activation of the
    row's own channel -- z1 for conv1's, z1 and z2 for conv2's (conv1's gradients sum over all channels of z2 above z1)."""
    S = scale(T, sd, mel, d_x0)
    Sf = dict(S)
    if precision == "bf16" and weight_grads:
        S1 = scale(T, sd, mel, d_x0, floor=GELU_ABS, zround=2.0 ** -9, z2_too=False)
        S2 = scale(T, sd, mel, d_x0, floor=GELU_ABS, zround=2.0 ** -9)
        Sf = {k: (S1[k] if k.startswith("conv1") else S2[k] if k.startswith("conv2") else S[k]) for k in S}
    return S, Sf


# ---------------------------------------------------------------- the chain as the kernels run it
DEFECTS = ("tap1_token0", "tap2_last_token", "halo_frame64", "neighbour_segment", "junk_row", "guard_dropped",
           "kc1_padding", "pos_one_segment_short")


def chain(T, sd, mel, d_x0, mode="fp64", defect=None):
    """The stem backward tap by tap on the padded token-major buffers, written from the comments of
    gw_whisper_amd/csrc/train_ops.hip.
    mode "fp64": no rounding (must equal ``reference``); "bf16": rounds where the bf16 kernels store -- bf16(d_x0), z1,
    c1, z2, dz2, each tap of col, dz1, each tap of col1, the fp32 three-tap sum, fp32 weight gradients; "fp32": a float32
    evaluation.  ``defect``: one of DEFECTS, an indexing error modelled on this layout.  Returns {name: numpy} of NAMES."""
    dt = T.float32 if mode == "fp32" else T.float64
    if mode == "bf16":
        rnd = lambda x: x.float().bfloat16().to(dt)
        f32 = lambda x: x.float().to(dt)
    else:
        rnd = f32 = lambda x: x
    tt = lambda a: T.from_numpy(np.array(a)).to(dt)
    w1, b1, w2, b2 = (tt(sd[k]) for k in ("conv1.weight", "conv1.bias", "conv2.weight", "conv2.bias"))
    m = tt(mel)
    g = tt(d_x0)
    B, C, Tin = m.shape
    Tn, d = Tin // 2, w1.shape[0]
    Kc1 = (3 * C + 63) // 64 * 64
    if mode == "fp32":   # gelu_erf (csrc/common.h) and gelu_grad_exact (csrc/train_f32.hip) of gw_whisper_amd, in float32
        gelu = lambda z: 0.5 * z * (1.0 + T.erf(z * (1.0 / math.sqrt(2.0))))
        dgelu = lambda z: 0.5 * (1.0 + T.erf(z * (1.0 / math.sqrt(2.0)))) + z * (1.0 / math.sqrt(2.0 * math.pi)) * T.exp(-0.5 * z * z)
    else:
        gelu, dgelu = (lambda z: _gelu(T, z)), (lambda z: _gelu_grad(T, z))
    with T.no_grad():
        # forward buffers: flat, as the device holds them (a row index past a segment lands in the next one)
        melT = T.zeros((B * (Tin + 2) + 4, C), dtype=dt)
        melT[:B * (Tin + 2)].view(B, Tin + 2, C)[:, 1:Tin + 1] = m.transpose(1, 2)
        M1, M2 = B * (Tin + 2), B * (Tn + 1)
        z1 = b1 + sum(melT[k:k + M1] @ w1[:, :, k].T for k in range(3))                  # row b (Tin + 2) + t1
        z1 = rnd(z1)
        real1 = (T.arange(M1) % (Tin + 2)) < Tin
        c1 = T.zeros((M1 + 4, d), dtype=dt)
        c1[1:M1 + 1] = rnd(gelu(z1)) * real1[:, None]                                  # frame t1 at padded row t1 + 1
        rows2 = 2 * T.arange(M2)                                                       # row b (T+1) + t reads rows 2 m ..
        z2 = rnd(b2 + sum(c1[rows2 + k] @ w2[:, :, k].T for k in range(3)))
        real2 = (T.arange(M2) % (Tn + 1)) < Tn
        gp = T.zeros((M2, d), dtype=dt)
        gp.view(B, Tn + 1, d)[:, :Tn] = rnd(g)
        if defect in ("junk_row", "guard_dropped"):     # the t < T test of k_stem_dz2 lost: the junk row takes the next
            flat = T.cat([rnd(g).reshape(B * Tn, d), T.zeros((1, d), dtype=dt)])       # segment's token 0
            for b in range(B):
                gp[b * (Tn + 1) + Tn] = flat[(b + 1) * Tn]
            real2 = T.ones(M2, dtype=T.bool)
        dz2 = rnd(gp * dgelu(z2)) * real2[:, None]
        # conv2 gradients on the forward's im2col view
        dw2 = T.stack([dz2.T @ c1[rows2 + k] for k in range(3)], 2)                     # [co, ci, k]
        db2 = dz2.sum(0)
        col = T.stack([rnd(dz2 @ w2[:, :, k]) for k in range(3)], 1)                    # [M2, 3, d]
        # gather into the conv1 output frames
        gsum = T.zeros((M1, d), dtype=dt)
        for b in range(B):
            cb = col[b * (Tn + 1):(b + 1) * (Tn + 1)]
            gs = gsum[b * (Tin + 2):b * (Tin + 2) + Tin]
            gs[0::2] += cb[:Tn, 1]                                                     # p = t1 + 1 odd
            gs[1::2] += cb[:Tn, 2]                                                     # p even: tap 2 of token p / 2 - 1
            gs[1:Tin - 1:2] += cb[1:Tn, 0]                                             # ... and tap 0 of p / 2 < T
            if defect == "tap1_token0":
                gs[0] -= cb[0, 1]
            if defect == "tap2_last_token":
                gs[Tin - 1] -= cb[Tn - 1, 2]
            if defect == "guard_dropped":              # p / 2 = T read all the same: the junk row, live under this defect
                gs[Tin - 1] += cb[Tn, 0]
        dz1 = rnd(f32(gsum) * dgelu(z1)) * real1[:, None]
        # conv1 gradients on the im2col view of melT, K = Kc1 (taps 0..2 of C channels, then padding that is dropped)
        view = T.cat([melT[k:k + M1] for k in range(4)], 1)[:, :Kc1]                    # [M1, Kc1]
        dwk = dz1.T @ view                                                             # [d, Kc1]
        if defect == "kc1_padding":                    # the padded rows taken as if they were 3 C long
            dwk = dwk.reshape(-1)[:d * 3 * C].reshape(d, 3 * C)
        dw1 = dwk[:, :3 * C].reshape(d, 3, C).transpose(1, 2)
        db1 = dz1.sum(0)
        col1 = T.stack([rnd(dz1 @ w1[:, :, k]) for k in range(3)], 1)                   # [M1, 3, C]
        dmel = T.zeros((B, C, Tin), dtype=dt)
        for b in range(B):
            cb = col1[b * (Tin + 2):b * (Tin + 2) + Tin]
            acc = T.zeros((Tin, C), dtype=dt)
            acc[:] += cb[:, 1]                                                         # k = 1: row tau
            acc[:Tin - 1] += cb[1:, 0]                                                 # k = 0: row tau + 1 < Tin
            acc[1:] += cb[:Tin - 1, 2]                                                 # k = 2: row tau - 1 >= 0
            if defect == "halo_frame64" and Tin > 64:
                acc[63] -= cb[64, 0]                                                   # the tile's upper halo row lost
            if defect == "neighbour_segment" and b + 1 < B:
                acc[Tin - 1] += col1[(b + 1) * (Tin + 2), 0]                           # frame Tin of b taken from b + 1
            dmel[b] = f32(acc).T
        nb = B - 1 if defect == "pos_one_segment_short" else B
        dpos = T.zeros((Tn, d), dtype=dt)
        for b in range(nb):                                                            # batch order fixed
            dpos = f32(dpos + g[b])
    out = {"d_mel": dmel, "conv1.weight": f32(dw1), "conv1.bias": f32(db1), "conv2.weight": f32(dw2),
           "conv2.bias": f32(db2), "embed_positions.weight": dpos}
    return {k: v.double().numpy() for k, v in out.items()}


# ---------------------------------------------------------------- the bound
# c = 4 x the emulation's worst ratio (profiles/stem_backward.md; printed by
# tests/test_stem_like_host.py::test_emulation_stays_within_the_bound), per tensor, per precision and per encoder width:
# over all cases, patterns and both regimes of that width.  (The ratio of d_mel and of conv1's gradients falls with d, as
# sums of d terms do against their absolute-value sum; one c for the whole table would be the d = 128 figure and at
# d = 1280 would flag a lost tap by a factor 1.5 only.  conv2's gradients and embed_positions do not depend on d: the
# table's worst.)  The ratio is |emulation - reference| / S for d_mel and embed_positions, whose elements sum over all
# channels, and (|emulation - reference| - E) / S for the conv gradients.  The factor 4 covers the device's GELU / GELU'
# approximations, its fp32 accumulation order and c1 coming from the forward kernels.  Never set from what the kernels give.
RAW_RATIO = ("d_mel", "embed_positions.weight")
_ALL_D = lambda v: {d: v for d in WIDTHS}
WORST = {
    "bf16": {"d_mel": {128: 4.15e-4, 384: 1.35e-4, 512: 7.52e-5, 1280: 3.31e-5},
             "conv1.weight": {128: 1.88e-3, 384: 1.09e-3, 512: 1.04e-3, 1280: 8.54e-4},
             "conv1.bias": {128: 1.33e-3, 384: 6.47e-4, 512: 5.45e-4, 1280: 4.42e-4},
             "conv2.weight": _ALL_D(5.74e-3), "conv2.bias": _ALL_D(5.76e-3), "embed_positions.weight": _ALL_D(1.07e-7)},
    "fp32": {"d_mel": {128: 4.32e-8, 384: 1.07e-8, 512: 1.07e-8, 1280: 4.2e-9}},
}


def worst(precision, name, case):
    return WORST[precision][name][CASES[case][0]]


def c_bound(precision, name, case):
    return 4.0 * worst(precision, name, case)


def _where(name, idx):
    """Names the element: segment / frame or token / channel / tap."""
    if name == "d_mel":
        return f"segment {idx[0]} mel channel {idx[1]} frame {idx[2]} (token {idx[2] // 2}, k_stem_dmel tile {idx[2] // 64})"
    if name.endswith("weight") and name.startswith("conv"):
        return f"out channel {idx[0]} in channel {idx[1]} tap {idx[2]}"
    if name.startswith("embed"):
        return f"token {idx[0]} channel {idx[1]}"
    return f"channel {idx[0]}"


def ratios(name, got, ref, S, S_floor):
    """The ratio c is set from: |got - ref| / S (RAW_RATIO) or (|got - ref| - E) / S clipped at zero, E = S_floor - S;
    0 where S = 0."""
    err = np.abs(np.asarray(got, np.float64) - ref)
    E = 0.0 if name in RAW_RATIO else S_floor - S
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(S > 0, np.maximum(err - E, 0.0) / S, 0.0)
    return r


def compare(name, got, ref, S, S_floor, c):
    """The check of one tensor: |got - ref| <= c S + E with E = S_floor - S (``scales``; 0 for RAW_RATIO), and got
    exactly zero where S = 0.  Returns None when it holds, else the message naming the worst element."""
    got = np.asarray(got, np.float64)
    if not np.isfinite(got).all():
        return f"{name}: not finite at {tuple(int(i) for i in np.argwhere(~np.isfinite(got))[0])}"
    E = 0.0 if name in RAW_RATIO else S_floor - S
    dead = S == 0
    if (got[dead] != 0).any():
        idx = tuple(int(i) for i in np.argwhere(dead & (got != 0))[0])
        return (f"{name}: {got[idx]:.3e} where no term reaches ({_where(name, idx)}); "
                f"{int((got[dead] != 0).sum())} such elements")
    bound = c * S + E
    err = np.abs(got - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(dead, 0.0, err / bound)
    idx = tuple(int(i) for i in np.unravel_index(int(np.argmax(r)), r.shape))
    if r[idx] > 1.0:
        return (f"{name}: |got - ref| = {err[idx]:.3e} is {r[idx]:.2f} x the bound {bound[idx]:.3e} (c = {c:.2e}, "
                f"S = {S[idx]:.3e}) at {_where(name, idx)}: got {got[idx]:.6e}, reference {ref[idx]:.6e}")
    return None


# ---------------------------------------------------------------- the C entries through ctypes
def c_step(T, enc, mel, pooled, d_hidden, want_x0, want_mel, grads=None):
    """gww_encoder_train_forward + _backward (their _f32 twins for an fp32 encoder) straight through ctypes, no targets:
    (d_x0 | None, d_mel | None).  The outputs start as NaN, so an element the backward leaves unwritten shows.  With
    ``grads`` ({field of gww_enc_grads: fp32 tensor}, bf16 only) the backward is gww_encoder_train_backward_full, which
    accumulates into those tensors."""
    import ctypes as C

    from gw_whisper_amd import _lib
    lib = _lib.lib()
    sfx = "_f32" if enc.precision == "fp32" else ""
    B, d, Tn = mel.shape[0], enc.config.d_model, enc.config.max_source_positions
    with T.cuda.device(mel.device):
        enc._sync_weights()
        h = enc._ensure_handle()
        ws_query = "gww_train_workspace_bytes" + ("_full" if grads else sfx)
        ws = T.empty((getattr(lib, ws_query)(h, B),), dtype=T.uint8, device=mel.device)
        saved = T.empty((getattr(lib, "gww_train_saved_bytes" + sfx)(h, B),), dtype=T.uint8, device=mel.device)
        hidden = T.empty((B, d) if pooled else (B, Tn, d), dtype=T.float32, device=mel.device)
        stream = T.cuda.current_stream().cuda_stream
        _lib.check(getattr(lib, "gww_encoder_train_forward" + sfx)(
            h, mel.data_ptr(), B, ws.data_ptr(), ws.numel(), saved.data_ptr(), saved.numel(), hidden.data_ptr(), int(pooled),
            stream), "train_forward" + sfx)
        d_x0 = T.full((B, Tn, d), float("nan"), dtype=T.float32, device=mel.device) if want_x0 else None
        d_mel = T.full(mel.shape, float("nan"), dtype=T.float32, device=mel.device) if want_mel else None
        args = (h, B, ws.data_ptr(), ws.numel(), saved.data_ptr(), saved.numel(), d_hidden.data_ptr(), None, 0,
                d_x0.data_ptr() if want_x0 else None, d_mel.data_ptr() if want_mel else None, int(pooled))
        if grads:
            gl = _lib.EncGrads()
            for field, buf in grads.items():
                assert buf.dtype == T.float32 and buf.is_contiguous() and buf.is_cuda
                setattr(gl, field, buf.data_ptr())
            _lib.check(lib.gww_encoder_train_backward_full(*args, C.byref(gl), stream), "train_backward_full")
        else:
            _lib.check(getattr(lib, "gww_encoder_train_backward" + sfx)(*args, stream), "train_backward" + sfx)
        T.cuda.synchronize()
    return d_x0, d_mel
