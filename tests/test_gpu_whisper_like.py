"""The forward kernels on inputs with a pretrained Whisper encoder's statistics (tests/whisper_like.py): outlier channels,
LayerNorm gains over two orders of magnitude, pre-activations in the tens, attention sinks.  Needs an MI355X (-m gpu).

Every reference is fp64.  The LayerNorm-folded projections are held to two bounds that come from the inputs alone
(``whisper_like.check_folded_projection``; tests/test_whisper_like_host.py checks on the CPU that the algebra the kernels
document stays inside them), the fused GELUs to their documented error on both sides of the |z| = 8 clamp, the attention
forward to the existing tolerances at every head count with sink keys, the encoder to the oracle's own bf16 emulation error.

Weights and biases of the projections follow ``synth.encoder_state_dict`` (N(0, 1 / fan_in), 0.02 N): the rms bound has no
term for the bf16 rounding of the stored result, which its factor 1.5 budgets at 0.87 of the ideal pipeline's error -- true
while the result's rms is about that of the projection itself.  A bias of order one would make the output rounding alone
(2^-8 / sqrt(3) relative) as large as the ideal operand error.
"""

import functools

import numpy as np
import pytest

from gw_whisper_amd import synth
from oracle import encoder as oenc
from oracle import logmel as olm

from . import whisper_like as wl

pytestmark = pytest.mark.gpu

bf = wl.bf
rms = lambda a: float(np.sqrt((np.asarray(a, np.float64) ** 2).mean()))


@pytest.fixture(scope="module")
def T():
    import torch
    assert torch.cuda.is_available()
    return torch


# ------------------------------------------------------------------ LayerNorm-folded kernels, every family
M_FULL = 300                     # ragged against the 256- and 128-row panels


@functools.lru_cache(maxsize=None)
def _operands(K, N, F=1536):
    """Families and one set of weights per contraction width, shared (read-only) by every test below."""
    rng = np.random.default_rng(1000 + K + N)
    w = lambda n, k: (rng.standard_normal((n, k)) / np.sqrt(k)).astype(np.float32)
    b = lambda n: (0.02 * rng.standard_normal(n)).astype(np.float32)
    o = dict(fam=wl.activation_families(rng, M_FULL, K), wq=w(N, K), bq=b(N), w1=w(F, K), b1=b(F), w2=bf(w(K, F)), b2=b(K),
             wo=bf(w(K, K)), bo=b(K), ctx=bf(rng.standard_normal((M_FULL, K))),
             # a pending delta that is exact in bf16 and adds exactly: multiples of 1/8 in [0, 2]
             dl=(rng.integers(0, 17, (M_FULL, K)) / 8.0).astype(np.float32))
    for v in o.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return o


def _launch(T, M, fn, *rows):
    """``fn(*device operands of some rows)`` -> tuple of device tensors, one row per input row.  M = 300: one launch.
    M = 1: the single-row shape, launched on every row of the family in turn and put together again -- the rms bound is a
    statistic of the family; one row's error is a single draw of its roundings (that of its outlier element alone moves a
    row's rms error by half)."""
    dev = [T.from_numpy(np.ascontiguousarray(a)).cuda() for a in rows]
    if M == M_FULL:
        return tuple(t.float().cpu().numpy() for t in fn(*dev))
    outs = [fn(*(a[r:r + 1].contiguous() for a in dev)) for r in range(M_FULL)]
    assert all(t.shape[0] == 1 for t in outs[0])
    return tuple(T.cat(part).float().cpu().numpy() for part in zip(*outs))


def _check_projection(tag, got, x, g, b, W, bias, gelu=False):
    """Both bounds, finiteness, and exactly constant rows -> cb to within the bf16 rounding of the result."""
    got = np.asarray(got, np.float64)
    assert np.isfinite(got).all(), tag
    r_rms, r_el, ok_rms, ok_el = wl.check_folded_projection(got, x, g, b, W, bias, gelu=gelu)
    print(f"{tag}: rms error / limit {r_rms:.3f}, worst element excess / (amp b) {r_el:.2f} (limit 10)")
    cr = wl.constant_rows(x)
    if cr.any():
        _, _, cb = wl.folded(g, b, W, bias)
        want = np.broadcast_to(oenc.gelu(cb) if gelu else cb, got.shape)[cr]
        # half a bf16 ulp of the result (8 significant bits: 2^-8 relative at most), and the fp32 summation of cb (K terms:
        # the existing fold test's 1e-5)
        assert (np.abs(got[cr] - want) <= 2.0 ** -8 * np.abs(want) + 1e-5).all(), tag
    assert ok_rms, f"{tag}: rms error {r_rms:.3f} of the limit"
    assert ok_el, f"{tag}: element excess {r_el:.2f} amp b"


def _family_x(o, family, with_delta):
    """(x handed to the kernel, delta or None, x_new = fp32(x + delta) as numpy computes it, gain, bias).  x is the family's
    row minus the delta, so that x_new IS the family's row (exactly so for `nearconst` and `degenerate`)."""
    x, g, b = o["fam"][family]
    if not with_delta:
        return x, None, x, g, b
    dl = o["dl"]
    x_in = (x - dl).astype(np.float32)
    x_new = (x_in + dl).astype(np.float32)
    if family in ("nearconst", "degenerate"):
        assert np.array_equal(x_new, x)
    return x_in, dl, x_new, g, b


@pytest.mark.parametrize("M", [300, 1])
@pytest.mark.parametrize("with_delta", [False, True], ids=["x", "x+delta"])
@pytest.mark.parametrize("K,N,epi", [(384, 1152, 0), (512, 2048, 1)], ids=["k384", "k512_gelu"])
@pytest.mark.parametrize("family", wl.FAMILIES)
def test_gemm_astat_layernorm_fold(T, gww, family, K, N, epi, with_delta, M):
    """gemm_astat.hip, AMODE_LN: Linear(LayerNorm(x + delta)) with the operand bf16(x_new - prefix mean)."""
    from gw_whisper_amd import ops
    o = _operands(K, N)
    x_in, dl, x_new, g, b = _family_x(o, family, with_delta)
    c = lambda a: T.from_numpy(np.ascontiguousarray(a)).cuda()
    wf, u, cb = ops.ln_fold_weights(c(o["wq"]), c(g), c(b), c(o["bq"]))
    if with_delta:
        got, got_x = _launch(T, M, lambda x, d: ops.gemm_astat(x, wf, None, epilogue=epi, ln=(u, cb), delta=d.bfloat16(),
                                                               return_x=True), x_in, dl)
    else:
        got, got_x = _launch(T, M, lambda x: ops.gemm_astat(x, wf, None, epilogue=epi, ln=(u, cb), return_x=True), x_in)
    np.testing.assert_array_equal(got_x, x_new)
    _check_projection(f"gemm_astat[{family} K={K} epi={epi} delta={with_delta} M={M}]", got, x_new, g, b, o["wq"], o["bq"],
                      gelu=bool(epi))


@pytest.mark.parametrize("M", [300, 1])
@pytest.mark.parametrize("family", wl.FAMILIES)
def test_lnqkv_fused(T, gww, family, M):
    """k_mlp_fused, MODE 2: the panel prologue (prefix shift, then the operand normalised and rounded a second time)."""
    from gw_whisper_amd import ops
    o = _operands(384, 1152)
    x, _, _, g, b = _family_x(o, family, False)
    c = lambda a: T.from_numpy(np.ascontiguousarray(a)).cuda()
    wqf, uq, cq = ops.ln_fold_weights(c(o["wq"]), c(g), c(b), c(o["bq"]))
    wt = ops.mlp_pack(None, None, wqf)
    got, x_after = _launch(T, M, lambda xd: (ops.lnqkv_fused(xd, wt, uq, cq), xd), x)
    assert np.array_equal(x_after, x)                                     # x is only read
    _check_projection(f"lnqkv_fused[{family} M={M}]", got, x, g, b, o["wq"], o["bq"])


def _mlp_delta_errors(got, x_new, g, b, o, w2=None, b2=None):
    """(reference, rms error, rms error / that of the fp64 evaluation with bf16-rounded operands at the same two GEMM inputs)."""
    w2 = o["w2"] if w2 is None else w2
    b2 = o["b2"] if b2 is None else b2
    ref = wl.mlp_fp64(x_new, g, b, o["w1"], o["b1"], w2, b2)
    yard = rms(wl.mlp_bf16_operands(x_new, g, b, o["w1"], o["b1"], w2, b2) - ref)
    return ref, rms(got - ref), rms(got - ref) / yard


def _fc2(o, family):
    """fc2 of the kernels with a q / k / v tail: zero for the families without a spread, so that the rows LayerNorm_1 sees
    at the seam are the family's rows themselves (x_next = x_new exactly)."""
    if family in ("nearconst", "degenerate"):
        return np.zeros_like(o["w2"]), np.zeros_like(o["b2"])
    return o["w2"], o["b2"]


def _attn_out_operands(o, family):
    """(x, ctx, bo, gain, bias): the block kernels form x_mid = x + ctx Wo^T + bo themselves; ctx and bo are zero for the
    families without a spread (x_mid = x exactly)."""
    x, g, b = o["fam"][family]
    if family in ("nearconst", "degenerate"):
        return x, np.zeros_like(o["ctx"]), np.zeros_like(o["bo"]), g, b
    return x, o["ctx"], o["bo"], g, b


def _run_mlp_fused(T, M, o, family, with_qkv, w2=None, b2=None):
    """ops.mlp_fused on the family: (C or qkv, x_new or x_next), and the operands' numpy side."""
    from gw_whisper_amd import ops
    x_in, dl, x_new, g, b = _family_x(o, family, True)
    w2 = o["w2"] if w2 is None else w2
    b2 = o["b2"] if b2 is None else b2
    c = lambda a: T.from_numpy(np.ascontiguousarray(a)).cuda()
    w1f, u, cb = ops.ln_fold_weights(c(o["w1"]), c(g), c(b), c(o["b1"]))
    b2d = c(b2)
    if with_qkv:
        wqf, uq, cq = ops.ln_fold_weights(c(o["wq"]), c(g), c(b), c(o["bq"]))
        wt = ops.mlp_pack(w1f, c(w2).bfloat16(), wqf)
        fn = lambda x, d: ops.mlp_fused(x, d.bfloat16(), wt, u, cb, b2d, qkv=(uq, cq))
    else:
        wt = ops.mlp_pack(w1f, c(w2).bfloat16())
        fn = lambda x, d: ops.mlp_fused(x, d.bfloat16(), wt, u, cb, b2d)
    return _launch(T, M, fn, x_in, dl), (x_new, g, b)


def _run_attn_out(T, M, o, family, w2=None, b2=None):
    """ops.attn_out_mlp_fused with the q / k / v tail on the family: (qkv, x_next), and x_mid in fp64."""
    from gw_whisper_amd import ops
    x, ctx, bo, g, b = _attn_out_operands(o, family)
    w2 = o["w2"] if w2 is None else w2
    b2 = o["b2"] if b2 is None else b2
    c = lambda a: T.from_numpy(np.ascontiguousarray(a)).cuda()
    w1f, u, cb = ops.ln_fold_weights(c(o["w1"]), c(g), c(b), c(o["b1"]))
    wqf, uq, cq = ops.ln_fold_weights(c(o["wq"]), c(g), c(b), c(o["bq"]))
    wo, bod, w2d, b2d = c(o["wo"]).bfloat16(), c(bo), c(w2).bfloat16(), c(b2)
    fn = lambda xd, cd: ops.attn_out_mlp_fused(xd, cd.bfloat16(), wo, bod, w1f, w2d, u, cb, b2d, qkv=(wqf, uq, cq))
    delta1 = ctx.astype(np.float64) @ o["wo"].astype(np.float64).T + bo
    return _launch(T, M, fn, x, ctx), (x, delta1, g, b)


@pytest.mark.parametrize("M", [300, 1])
@pytest.mark.parametrize("family", wl.FAMILIES)
def test_mlp_fused(T, gww, family, M):
    """k_mlp_fused, MODE 0: LayerNorm -> fc1 -> GELU -> fc2 of x + delta, F = 1536: x_new exact, the bf16 MLP delta by the
    existing test's per-element formula (bf16 operands twice, bf16 result)."""
    o = _operands(384, 1152)
    (got, got_x), (x_new, g, b) = _run_mlp_fused(T, M, o, family, False)
    np.testing.assert_array_equal(got_x, x_new)
    got = got.astype(np.float64)
    assert np.isfinite(got).all()
    ref, e, ratio = _mlp_delta_errors(got, x_new, g, b, o)
    print(f"mlp_fused[{family} M={M}]: MLP delta rms error {e:.2e}, max {np.abs(got - ref).max():.2e}")
    np.testing.assert_allclose(got, ref, atol=4e-2, rtol=2 ** -7)


# The MLP delta's rms bound carries no prefix-amplification factor.  The stand-alone block (k_mlp_fused, MODE 0) forms its fc1
# operand as its header documents, bf16(x - prefix mean) normalised and rounded again; where the prefix mean lies 1.5 / 3.3 row
# sigma from the row mean that alone exceeds the bound: measured on MI355X 1.64 x (`slope`) and 2.59 x (`block32`), and the CPU
# emulation of the documented algebra (whisper_like.mlp_bf16_operands(kernel_like=True), rounded to bf16) gives the same 1.64 x
# and 2.59 x.  The other families measure 1.05 .. 1.34 x.  (The block with out_proj in front normalises from the accumulators
# with the exact row mean and one rounding: 1.00 x on every family.)
_MLP_BY_DESIGN = {
    "slope": "documented design: fc1 operand bf16(x - prefix mean), prefix mean 1.5 row sigma off the row mean; measured and "
             "emulated 1.64 x the bf16-operand evaluation's rms error",
    "block32": "documented design: fc1 operand bf16(x - prefix mean), prefix mean 3.3 row sigma off the row mean; measured and "
               "emulated 2.59 x the bf16-operand evaluation's rms error",
}


def _mlp_rms_cases():
    for kernel in ("mlp_fused", "attn_out_mlp_fused"):
        for family in wl.FAMILIES:
            if kernel == "attn_out_mlp_fused" and family in ("nearconst", "degenerate"):
                continue                 # (these run with fc2 = 0 there: no delta)
            for M in (300, 1):
                why = _MLP_BY_DESIGN.get(family) if kernel == "mlp_fused" else None
                yield pytest.param(kernel, family, M, marks=[pytest.mark.xfail(strict=True, reason=why)] if why else [])


@pytest.mark.parametrize("kernel,family,M", list(_mlp_rms_cases()))
def test_mlp_delta_rms(T, gww, kernel, family, M):
    """The MLP delta's rms error within 1.5 x that of the fp64 evaluation with bf16-rounded operands at the same two GEMM
    inputs -- the stand-alone block's bf16 output, and x_next - x_mid of the block with out_proj in front (out_proj adds no
    operand error: ctx and Wo are bf16 already; the fp32 spacing of the stream, 2^-24 x 150, is far below the delta's 1e-3)."""
    o = _operands(384, 1152)
    if kernel == "mlp_fused":
        (got, _), (x_new, g, b) = _run_mlp_fused(T, M, o, family, False)
        got = got.astype(np.float64)
    else:
        (_, x_next), (x, delta1, g, b) = _run_attn_out(T, M, o, family)
        x_new = x.astype(np.float64) + delta1
        got = x_next.astype(np.float64) - x_new
    _, e, ratio = _mlp_delta_errors(got, x_new, g, b, o)
    print(f"MLP delta rms {kernel}[{family} M={M}]: {e:.2e} = {ratio:.2f} x the bf16-operand evaluation's (limit 1.5)")
    assert ratio <= 1.5


@pytest.mark.parametrize("M", [300, 1])
@pytest.mark.parametrize("family", wl.FAMILIES)
def test_mlp_fused_with_qkv(T, gww, family, M):
    """k_mlp_fused, MODE 1: x_next = x_new + bf16(mlp) (the stand-alone kernel's delta, one fp32 add) and the next layer's
    q / k / v = Linear(LayerNorm_1(x_next)) from the seam's prologue."""
    o = _operands(384, 1152)
    w2, b2 = _fc2(o, family)
    (qkv, xn), (x_new, g, b) = _run_mlp_fused(T, M, o, family, True, w2, b2)
    (delta2, got_x), _ = _run_mlp_fused(T, M, o, family, False, w2, b2)
    np.testing.assert_array_equal(got_x, x_new)
    assert np.isfinite(xn).all()
    np.testing.assert_allclose(xn, x_new.astype(np.float64) + delta2.astype(np.float64), atol=2e-5, rtol=1e-6)
    if family in ("nearconst", "degenerate"):
        np.testing.assert_array_equal(xn, x_new)
    _check_projection(f"mlp_fused+qkv[{family} M={M}]", qkv, xn, g, b, o["wq"], o["bq"])


@pytest.mark.parametrize("M", [300, 1])
@pytest.mark.parametrize("family", wl.FAMILIES)
def test_attn_out_mlp_fused_with_qkv(T, gww, family, M):
    """k_mlp_fused<1, true>: out_proj + LN2 + fc1 + GELU + fc2 + the next LN1 + q / k / v; the residual stream stays in the
    accumulators.  x_next by the existing rule (each delta rounded to bf16 at most once, 4e-2 of bf16-operand noise),
    q / k / v by the projection bounds on the kernel's own x_next."""
    o = _operands(384, 1152)
    w2, b2 = _fc2(o, family)
    (qkv, x_next), (x, delta1, g, b) = _run_attn_out(T, M, o, family, w2, b2)
    got_x = x_next.astype(np.float64)
    assert np.isfinite(got_x).all()
    x_mid = x.astype(np.float64) + delta1
    mlp = wl.mlp_fp64(x_mid, g, b, o["w1"], o["b1"], w2, b2)
    tol_x = np.abs(mlp) * 2.0 ** -7 + np.abs(delta1) * 2.0 ** -7 + 4e-2
    assert (np.abs(got_x - (x_mid + mlp)) <= tol_x).all(), np.abs(got_x - (x_mid + mlp)).max()
    if family in ("nearconst", "degenerate"):
        np.testing.assert_array_equal(x_next, x)
    _check_projection(f"attn_out_mlp_fused+qkv[{family} M={M}]", qkv, x_next, g, b, o["wq"], o["bq"])


@pytest.mark.parametrize("M", [300, 1])
@pytest.mark.parametrize("family", wl.FAMILIES)
def test_attn_out_mlp_final(T, gww, family, M):
    """k_mlp_fused<3, true>: the last block with the encoder's final LayerNorm as its epilogue, fp32 out.  y against
    LayerNorm(x_mid + mlp) in fp64 on the kernel's own x_mid: an element of x_next carries the MLP delta's error (the
    existing 4e-2 + 2^-7 |mlp| at the level of the stream), which LayerNorm scales by |gain_k| / s_m; the row's rstd moves
    by the same relative amount, hence the term relative to y - bias."""
    from gw_whisper_amd import ops
    o = _operands(384, 1152)
    x, ctx, bo, g, b = _attn_out_operands(o, family)
    c = lambda a: T.from_numpy(np.ascontiguousarray(a)).cuda()
    w1f, u, cb = ops.ln_fold_weights(c(o["w1"]), c(g), c(b), c(o["b1"]))
    wo, bod, w2d, b2d, gd, bd = c(o["wo"]).bfloat16(), c(bo), c(o["w2"]).bfloat16(), c(o["b2"]), c(g), c(b)
    y, got_mid = _launch(T, M, lambda xd, cd: ops.attn_out_mlp_final(xd, cd.bfloat16(), wo, bod, w1f, w2d, u, cb, b2d, gd, bd),
                         x, ctx)
    delta1 = ctx.astype(np.float64) @ o["wo"].astype(np.float64).T + bo
    x_mid = x.astype(np.float64) + delta1
    got_mid = got_mid.astype(np.float64)
    assert np.abs(got_mid - x_mid).max() <= np.abs(delta1).max() * 2.0 ** -7 + 1e-3
    mlp = wl.mlp_fp64(got_mid, g, b, o["w1"], o["b1"], o["w2"], o["b2"])
    x_next = got_mid + mlp
    ref = oenc.layer_norm(x_next, g.astype(np.float64), b.astype(np.float64))
    s_m = np.sqrt(x_next.var(axis=1, keepdims=True) + wl.LN_EPS)
    got = y.astype(np.float64)
    assert np.isfinite(got).all()
    tol = np.abs(g)[None, :] / s_m * (4e-2 + 2.0 ** -7 * np.abs(mlp)) + 2.0 ** -7 * np.abs(ref - b[None, :]) + 1e-5
    worst = float((np.abs(got - ref) / tol).max())
    print(f"attn_out_mlp_final[{family} M={M}]: rms error {rms(got - ref):.2e}, worst element {worst:.2f} of its tolerance")
    assert worst <= 1.0


# ------------------------------------------------------------------ GELU away from the origin
def _gelu64(z):
    return oenc.gelu(np.asarray(z, np.float64))


def _check_gelu(tag, got, z, atol, rtol=2.0 ** -8, exact=True, out_bf16=True, bulk=True):
    """|got - gelu(z)| <= rtol |gelu(z)| + atol; no NaN / Inf; z >= 9 -> z itself (rounded as the output is); z <= -9 -> 0
    to within atol.  ``z`` is the pre-activation exactly as the kernel forms it (fp32) when ``exact``."""
    got, z = np.asarray(got, np.float64), np.asarray(z, np.float64)
    assert np.isfinite(got).all(), tag
    ref = _gelu64(z)
    err = np.abs(got - ref)
    lim = rtol * np.abs(ref) + atol
    print(f"{tag}: z in [{z.min():.2f}, {z.max():.2f}], worst |err| / limit {float((err / lim).max()):.3f}, "
          f"max |err| at |z| >= 8: {float(err[np.abs(z) >= 8].max(initial=0)):.2e}")
    assert (err <= lim).all(), f"{tag}: z = {z.ravel()[np.argmax(err / lim)]}, got {got.ravel()[np.argmax(err / lim)]}"
    hi, lo = z >= 9, z <= -9
    assert hi.any() and lo.any() and (not bulk or (np.abs(z) < 8).any())
    if exact:
        want = bf(z[hi]) if out_bf16 else z[hi].astype(np.float32)
        np.testing.assert_array_equal(got[hi].astype(np.float32), want, err_msg=tag)
    assert (np.abs(got[lo]) <= np.broadcast_to(atol, got.shape)[lo]).all(), tag


ATOL_SIG = 3e-5       # gelu_sig / gelu_sig4 / the table: documented |err| <= 2.6e-5 on the whole real line


def _atol_fast(z):
    """gelu_fast: 0.5 z (1 + erf) with erf by Abramowitz-Stegun 7.1.26, |err| <= 1.5e-7, one v_rcp_f32 and one v_exp_f32
    (1 ulp = 6e-8 each on factors <= 1): 3e-7 on erf, times |z| / 2."""
    return 0.5 * np.abs(z) * 3e-7 + 1e-7


def _atol_erf(z):
    """gelu_erf: ocml erff (a few ulp of 1: 5e-7) times |z| / 2, the fp32 path's whole error besides the final rounding."""
    return 0.5 * np.abs(z) * 5e-7 + 1e-7


@pytest.mark.parametrize("random_w1", [False, True], ids=["w1=0", "w1_small"])
@pytest.mark.parametrize("kernel", ["mlp_fused", "attn_out_mlp_fused"])
def test_gelu_slice_sweep(T, gww, kernel, random_w1):
    """The hand-scheduled GELU of k_mlp_fused made visible: fc2 is a 0 / 1 selection (column j of the output is
    bf16(gelu(z_j)) once), z is set through fc1's bias -- exactly (W1 = 0: z = cb) or moved by a small random W1."""
    from gw_whisper_amd import ops
    d, F, M = 384, 512, 300
    rng = np.random.default_rng(77)
    o = _operands(384, 1152)
    x, g, b = o["fam"]["gauss"]
    z0 = wl.gelu_sweep_z(rng, F)
    w1 = (0.005 * rng.standard_normal((F, d)) / np.sqrt(d)).astype(np.float32) if random_w1 else np.zeros((F, d), np.float32)
    w2 = np.zeros((d, F), np.float32)
    w2[np.arange(d), np.arange(d)] = 1.0
    lnb = b if random_w1 else np.zeros_like(b)          # (W1 = 0: cb = b1 + W1 b_ln = b1 exactly either way)
    c = lambda a: T.from_numpy(np.ascontiguousarray(a)).cuda()
    w1f, u, cb = ops.ln_fold_weights(c(w1), c(g), c(lnb), c(z0))
    zeros = np.zeros((M, d), np.float32)
    if kernel == "mlp_fused":
        out, _ = ops.mlp_fused(c(x), c(zeros).bfloat16(), ops.mlp_pack(w1f, c(w2).bfloat16()), u, cb, c(np.zeros(d, np.float32)))
        xn = x
    else:
        out, x_mid = ops.attn_out_mlp_fused(c(x), c(o["ctx"]).bfloat16(), c(o["wo"]).bfloat16(), c(o["bo"]), w1f,
                                            c(w2).bfloat16(), u, cb, c(np.zeros(d, np.float32)))
        xn = x_mid.cpu().numpy()
    got = out.float().cpu().numpy()
    tag = f"gelu sweep {kernel}[{'small W1' if random_w1 else 'W1 = 0'}]"
    if not random_w1:
        assert np.array_equal(cb.cpu().numpy(), z0)
        _check_gelu(tag, got, np.broadcast_to(z0[:d], got.shape), ATOL_SIG)
    else:
        z = oenc.layer_norm(xn.astype(np.float64), g, lnb) @ w1.astype(np.float64).T + z0
        # the pre-activation itself carries the projection's operand noise (the per-element bound of the folded projections,
        # 10 amp b), passed on by |gelu'| <= 1.13
        amp, bn = wl.noise_bound(xn, g, lnb, w1, z0)
        dz = 1.13 * 10.0 * amp[:, None] * bn
        assert dz.max() < 3e-4
        _check_gelu(tag, got, z[:, :d], ATOL_SIG + dz[:, :d], exact=False)


def _exact_gemm_operands(rng, M, N, K):
    """A in {-1, 0, 1}, W[n] = 0.25 e_(n mod K): every product and sum is exact in fp32, so the pre-activation the kernel
    forms is fp32(0.25 A[m, n mod K] + bias[n]), one rounding -- known bit for bit."""
    a = rng.integers(-1, 2, (M, K)).astype(np.float32)
    w = np.zeros((N, K), np.float32)
    w[np.arange(N), np.arange(N) % K] = 0.25
    bias = wl.gelu_sweep_z(rng, N)
    z = (0.25 * a[:, np.arange(N) % K]).astype(np.float32) + bias[None, :]
    assert z.dtype == np.float32
    return a, w, bias, z


@pytest.mark.parametrize("kernel,M,N,K", [("gemm_bf16", 300, 384, 384), ("gemm_bf16_v4", 256, 256, 128), ("gemm_f32", 300, 128, 96),
                                          ("gemm_astat", 300, 512, 512), ("gemm_fulln", 300, 384, 1152)])
def test_gemm_gelu_epilogue_sweep(T, gww, kernel, M, N, K):
    """epilogue = 1 of every GEMM with pre-activations swept through the tails (gelu_fast; gelu_erf in fp32)."""
    from gw_whisper_amd import ops
    a, w, bias, z = _exact_gemm_operands(np.random.default_rng(N + K), M, N, K)
    c = lambda t: T.from_numpy(t).cuda()
    if kernel == "gemm_f32":
        got = ops.gemm(c(a), c(w), c(bias), epilogue=1).cpu().numpy()
        _check_gelu(kernel, got, z, _atol_erf(z), rtol=2.0 ** -23, out_bf16=False)
        return
    fn = {"gemm_bf16": ops.gemm, "gemm_bf16_v4": ops.gemm, "gemm_astat": ops.gemm_astat, "gemm_fulln": ops.gemm_fulln}[kernel]
    got = fn(c(a).bfloat16(), c(w).bfloat16(), c(bias), epilogue=1).float().cpu().numpy()
    assert got.shape == (M, N)
    # (k_gemm_bf16_v4 -- M % 256 == 0, N % 256 == 0, K % 128 == 0 -- applies gelu_sig4, the other three gelu_fast)
    _check_gelu(kernel, got, z, ATOL_SIG if kernel == "gemm_bf16_v4" else _atol_fast(z))


def test_gemm_astat_layernorm_gelu_sweep(T, gww):
    """The LayerNorm-folded form with the GELU epilogue (fc1 of the per-op walk): W = 0, so z = cb."""
    from gw_whisper_amd import ops
    K, N = 512, 2048
    rng = np.random.default_rng(5)
    x, g, b = _operands(K, N)["fam"]["whisperlike"]
    z0 = wl.gelu_sweep_z(rng, N)
    c = lambda t: T.from_numpy(np.ascontiguousarray(t)).cuda()
    wf, u, cb = ops.ln_fold_weights(c(np.zeros((N, K), np.float32)), c(g), c(b), c(z0))
    assert np.array_equal(cb.cpu().numpy(), z0)
    got = ops.gemm_astat(c(x), wf, None, epilogue=1, ln=(u, cb)).float().cpu().numpy()
    _check_gelu("gemm_astat LN fold + GELU", got, np.broadcast_to(z0, got.shape), _atol_fast(z0)[None, :])


@pytest.mark.parametrize("d", [384, 512])
def test_conv1_gelu_sweep(T, gww, d):
    """conv1 + GELU of the stem: zero weights (every frame of channel c is gelu(bias_c), swept), then random weights under
    biases of +-15 (every pre-activation in the saturated tails: z itself, or zero)."""
    from gw_whisper_amd import ops
    B, Tn = 2, 257
    rng = np.random.default_rng(d)
    mel = T.from_numpy((rng.standard_normal((B, 80, Tn)) * 0.8).astype(np.float32))
    z0 = wl.gelu_sweep_z(rng, d)
    got = ops.conv1_gelu(mel.cuda(), T.zeros(d, 80, 3).cuda(), T.from_numpy(z0).cuda()).float().cpu().numpy()
    assert not got[:, 0].any() and not got[:, Tn + 1].any()
    _check_gelu(f"conv1_gelu[d={d}, W = 0]", got[:, 1:Tn + 1], np.broadcast_to(z0, (B, Tn, d)), ATOL_SIG)
    w = T.from_numpy((rng.standard_normal((d, 80, 3)) / np.sqrt(240)).astype(np.float32))
    bias = T.from_numpy(np.where(np.arange(d) % 2 == 0, 15.0, -15.0).astype(np.float32))
    got = ops.conv1_gelu(mel.cuda(), w.cuda(), bias.cuda()).float().cpu().numpy()
    r16 = lambda t: t.to(T.bfloat16).to(T.float64)
    z = T.nn.functional.conv1d(r16(mel), r16(w), bias.double(), padding=1).transpose(1, 2).numpy()
    assert np.abs(z).min() > 9
    # fp32 accumulation of 240 bf16 products (the GEMM tests' 1e-5 sqrt(K)) moves z, and |gelu'| <= 1.13
    _check_gelu(f"conv1_gelu[d={d}, bias +-15]", got[:, 1:Tn + 1], z, ATOL_SIG + 1.13e-5 * np.sqrt(240), exact=False,
                bulk=False)


# ------------------------------------------------------------------ forward attention: sink keys at every head count
ATT_CASES = [(2, 332, H, s) for H in (6, 8, 12, 16, 20) for s in (12.0, 40.0)] + [(1, 1500, 20, 40.0)]


def _per_head(fn, qkv, H):
    """An fp64 reference applied head by head (the [B, H, T, T] fp64 scores of 20 heads at T = 1500 are 360 MB apiece)."""
    d = H * 64
    out = []
    for h in range(H):
        sl = [slice(s * d + h * 64, s * d + (h + 1) * 64) for s in range(3)]
        out.append(fn(np.concatenate([qkv[..., s] for s in sl], axis=-1)))
    return out


def _attn_ref(qkv, H, bf16):
    f = lambda one: oenc.attention(*(one[..., 64 * i:64 * (i + 1)].astype(np.float64) for i in range(3)), 1, bf16, np.float64)
    return np.concatenate(_per_head(f, qkv, H), axis=-1)


def _rerandomise_other_heads(rng, qkv, H, keep):
    d = H * 64
    out = qkv.copy()
    for h in range(H):
        if h not in keep:
            for s in range(3):
                out[..., s * d + h * 64:s * d + (h + 1) * 64] = rng.standard_normal(qkv.shape[:2] + (64,)) * 0.4
    return out


def _check_sinks(T, tag, run, qkv, ref, peaked, H, bland, tol, rng, post=lambda a: a):
    """Against the reference; each peaked row equals its key's v; the output of a head does not depend on the other heads."""
    d = H * 64
    got_dev = run(qkv)
    got = got_dev.float().cpu().numpy()
    assert np.isfinite(got).all(), tag
    print(f"{tag}: max |ctx - fp64| {np.abs(got - ref).max():.2e}")
    np.testing.assert_allclose(got, ref, **tol)
    v = post(qkv)[..., 2 * d:]
    for h, qr, kr in peaked:
        np.testing.assert_allclose(got[:, qr, h * 64:(h + 1) * 64], v[:, kr, h * 64:(h + 1) * 64], atol=1e-2, err_msg=tag)
    keep = (bland, (bland + 1) % H)
    other = run(_rerandomise_other_heads(rng, qkv, H, keep))
    assert not T.equal(other, got_dev)
    for h in keep:
        assert T.equal(other[..., h * 64:(h + 1) * 64], got_dev[..., h * 64:(h + 1) * 64]), f"{tag}: head {h} depends on others"


@pytest.mark.parametrize("B,Tn,H,s", ATT_CASES)
def test_attention_sinks_bf16(T, gww, B, Tn, H, s):
    from gw_whisper_amd import ops
    rng = np.random.default_rng(B * 1000 + Tn + H + int(s))
    bland = int(s) % H
    qkv, peaked = wl.sink_qkv(rng, B, Tn, H, s, bland)
    qkv = bf(qkv)
    run = lambda a: ops.attention(T.from_numpy(bf(a)).cuda().bfloat16(), H)
    _check_sinks(T, f"attention bf16[B={B} T={Tn} H={H} s={s}]", run, qkv, _attn_ref(qkv, H, True), peaked, H, bland,
                 dict(atol=6e-3, rtol=2 ** -7), rng)


@pytest.mark.parametrize("B,Tn,H,s", ATT_CASES)
def test_attention_sinks_f32(T, gww, B, Tn, H, s):
    from gw_whisper_amd import ops
    rng = np.random.default_rng(B * 1000 + Tn + H + int(s) + 1)
    bland = int(s) % H
    qkv, peaked = wl.sink_qkv(rng, B, Tn, H, s, bland)
    run = lambda a: ops.attention(T.from_numpy(a.astype(np.float32)).cuda(), H)
    _check_sinks(T, f"attention fp32[B={B} T={Tn} H={H} s={s}]", run, qkv, _attn_ref(qkv, H, False), peaked, H, bland,
                 dict(atol=2e-5, rtol=1e-4), rng)


@pytest.mark.parametrize("B,Tn,H,s", ATT_CASES)
def test_attention_sinks_log2q(T, gww, B, Tn, H, s):
    from gw_whisper_amd import ops
    rng = np.random.default_rng(B * 1000 + Tn + H + int(s) + 2)
    bland = int(s) % H
    qkv, peaked = wl.sink_qkv(rng, B, Tn, H, s, bland)
    prep = lambda a: wl.to_log2q(bf(a))
    q2 = prep(qkv)
    ref = np.concatenate(_per_head(lambda one: wl.attn_ref_log2q(one, 1), q2, H), axis=-1)
    lse_ref = np.concatenate(_per_head(lambda one: wl.lse_ref_log2q(one, 1), q2, H), axis=1)
    lse = {}

    def run(a):
        ctx, lse["last"] = ops.attention_log2q(T.from_numpy(prep(a)).cuda().bfloat16(), H, want_lse=True)
        return ctx
    tag = f"attention log2q[B={B} T={Tn} H={H} s={s}]"
    got_lse = ops.attention_log2q(T.from_numpy(q2).cuda().bfloat16(), H, want_lse=True)[1]
    assert T.isfinite(got_lse).all()
    np.testing.assert_allclose(got_lse.cpu().numpy(), lse_ref, atol=2e-2, rtol=1e-3)
    _check_sinks(T, tag, run, qkv, ref, peaked, H, bland, dict(atol=6e-3, rtol=2 ** -7), rng, post=prep)
    keep = (bland, (bland + 1) % H)
    for h in keep:                                   # (the lse of the last run: the re-randomised operand)
        assert T.equal(lse["last"][:, h], got_lse[:, h]), f"{tag}: lse of head {h} depends on others"


# ------------------------------------------------------------------ encoder forward on Whisper-like weights
ENC_DIMS = {"d384": (384, 2, 6, 1536), "d512": (512, 2, 8, 2048)}


def _mels():
    padded = olm.log_mel(synth.strain_segments(2, seed=21))
    dense = (0.5 * np.random.default_rng(8).standard_normal((2, 80, 3000))).astype(np.float32)
    return {"padded": padded, "dense": dense}


@pytest.fixture(scope="module", params=list(ENC_DIMS))
def enc_case(request):
    """Per width: the weights, both inputs, and the oracle's fp64 run (with stages) and bf16-emulating run of each --
    computed once."""
    dims = ENC_DIMS[request.param]
    sd = wl.whisper_like_state_dict(*dims, seed=7)
    cfg = oenc.EncCfg(*dims)
    runs = {}
    for name, mel in _mels().items():
        ref, stages = oenc.encoder_forward(sd, mel, cfg, dtype=np.float64, return_stages=True)
        emu = oenc.encoder_forward(sd, mel, cfg, dtype=np.float64, emulate_bf16=True)
        L = dims[1]
        runs[name] = dict(mel=mel, ref=ref, emu=emu, hidden=[stages["embed"]] + [stages[f"l{i}.out"] for i in range(L - 1)])
    return request.param, dims, sd, runs


def _encoder(T, dims, sd, precision):
    from gw_whisper_amd.encoder import WhisperConfig, WhisperEncoder
    return WhisperEncoder.from_numpy_state_dict(sd, WhisperConfig(*dims), precision=precision).cuda()


@pytest.mark.parametrize("mel_kind", ["padded", "dense"])
def test_encoder_fp32_on_whisper_like_weights(T, gww, enc_case, mel_kind):
    """fp32 against the fp64 oracle: the final output at the project's tolerance, every per-layer hidden state (they carry
    the outlier channels) to 2e-4 of its row's sigma + 1e-4 relative."""
    name, dims, sd, runs = enc_case
    r = runs[mel_kind]
    enc = _encoder(T, dims, sd, "fp32")
    mel = T.from_numpy(r["mel"]).cuda()
    with T.no_grad():
        out = enc(mel, output_hidden_states=True)
        plain = enc(mel).last_hidden_state
        last = enc.last_token(mel)
    hs = out.hidden_states
    L = dims[1]
    assert len(hs) == L + 1 and T.equal(hs[-1], out.last_hidden_state) and T.equal(plain, out.last_hidden_state)
    got = out.last_hidden_state.cpu().numpy()
    print(f"encoder fp32[{name} {mel_kind}]: max |out - fp64| {np.abs(got - r['ref']).max():.2e}")
    np.testing.assert_allclose(got, r["ref"], atol=2e-4, rtol=1e-4)
    np.testing.assert_allclose(last.cpu().numpy(), got[:, -1], atol=1e-5)
    for i, ref in enumerate(r["hidden"]):
        h = hs[i].cpu().numpy()
        s_row = ref.std(axis=-1, keepdims=True)
        worst = float((np.abs(h - ref) / (2e-4 * s_row + 1e-4 * np.abs(ref))).max())
        print(f"  hidden_states[{i}]: max |x| {np.abs(ref).max():.0f}, worst element {worst:.2f} of its tolerance")
        assert worst <= 1.0, i


@pytest.mark.parametrize("mel_kind", ["padded", "dense"])
def test_encoder_bf16_on_whisper_like_weights(T, gww, enc_case, mel_kind):
    """bf16 against the fp64 oracle, measured by the oracle's own bf16 emulation on the same input: rms error within 2 x,
    max error within 3 x (the Gaussian test holds the kernels to 0.8 of the emulation's error OF the emulation, 1.3 x in
    quadrature; 2 x leaves room for the bf16 storage of q / k / v / ctx, which the oracle does not model).  The pooled
    last token by the existing rule; the stem shortcut on and off bit for bit."""
    name, dims, sd, runs = enc_case
    r = runs[mel_kind]
    enc = _encoder(T, dims, sd, "bf16")
    mel = T.from_numpy(r["mel"]).cuda()
    bits = lambda a: a.contiguous().view(T.int32)
    with T.no_grad():
        out = enc(mel, output_hidden_states=True)
        hidden, last_full = enc.forward_raw(mel, want_hidden=True, want_last=True)
        flags = enc.stem_shortcut_flags(2)
        pooled = enc.last_token(mel)
        enc.set_stem_shortcut(False)
        hidden_off, last_off = enc.forward_raw(mel, want_hidden=True, want_last=True)
        pooled_off = enc.last_token(mel)
        enc.set_stem_shortcut(True)
    assert flags == ((1, -1) if mel_kind == "padded" else (0, -1))
    assert T.equal(bits(hidden), bits(hidden_off)) and T.equal(bits(last_full), bits(last_off))
    assert T.equal(bits(pooled), bits(pooled_off))
    assert T.equal(last_full, hidden[:, -1]) and T.equal(out.last_hidden_state, hidden)
    assert (pooled - last_full).abs().max().item() < 0.06
    got = hidden.cpu().numpy().astype(np.float64)
    assert np.isfinite(got).all()
    e_rms, e_max = rms(r["emu"] - r["ref"]), np.abs(r["emu"] - r["ref"]).max()
    k_rms, k_max = rms(got - r["ref"]), np.abs(got - r["ref"]).max()
    print(f"encoder bf16[{name} {mel_kind}]: rms error {k_rms:.2e} = {k_rms / e_rms:.2f} x the emulation's {e_rms:.2e} (limit 2), "
          f"max error {k_max:.2e} = {k_max / e_max:.2f} x the emulation's {e_max:.2e} (limit 3), "
          f"|pooled - full| {(pooled - last_full).abs().max().item():.2e}")
    L = dims[1]
    for i, ref in enumerate(r["hidden"]):
        h = out.hidden_states[i].cpu().numpy()
        assert np.isfinite(h).all()
        print(f"  hidden_states[{i}]: rms error {rms(h - ref):.2e} on max |x| {np.abs(ref).max():.0f}")
    assert len(out.hidden_states) == L + 1
    assert k_rms <= 2 * e_rms
    assert k_max <= 3 * e_max
