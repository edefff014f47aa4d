"""HIP kernels vs the numpy oracle, through the C ABI.  Needs an MI355X (-m gpu)."""

import numpy as np
import pytest

from gw_whisper_amd import synth
from oracle import dora as odora
from oracle import encoder as oenc
from oracle import logmel as olm

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def T():
    import torch
    assert torch.cuda.is_available()
    return torch


def _bf(x):
    """numpy fp32 -> values rounded to bf16 (as fp32)."""
    return oenc.bf16_round(np.asarray(x, np.float32))


# ------------------------------------------------------------------ log-mel
def test_logmel_matches_oracle_and_hf_golden(T, gww, golden):
    """On WHITE noise: every mel bin lies within two decades of the others, the max - 8 clamp never acts on a live frame and
    no output is the remainder of a cancellation, so 2e-5 holds on every element.  It says nothing about band-limited
    strain, where an fp32 front end (HF's included) is off exact arithmetic by up to 1e-4 in the leakage skirt:
    test_gpu_logmel_like.py holds the kernel per element there."""
    from gw_whisper_amd import ops
    g = golden("logmel.npz")
    seg = synth.strain_segments(4, seed=11)
    out = ops.logmel(T.from_numpy(seg).cuda()).cpu().numpy()
    assert out.shape == (4, 80, 3000)
    ref = olm.log_mel(seg)
    # fp32 DFT by direct summation vs an FFT: tolerance 2e-5 on values in [-0.7, 1.4]
    np.testing.assert_allclose(out, ref, atol=2e-5, rtol=0)
    np.testing.assert_allclose(out[:, :, :112], g["seg16000_frames0_112"], atol=2e-5, rtol=0)
    for i in range(4):
        assert np.all(out[i, :, 102:] == out[i, 0, 2999]), "dead frames must be one constant"
        assert abs(out[i, 0, 2999] - g["seg16000_pad_value"][i]) < 2e-5


@pytest.mark.parametrize("n", [1, 159, 12345, 40000])
def test_logmel_ragged_lengths(T, gww, golden, n):
    from gw_whisper_amd import ops
    g = golden("logmel.npz")
    w = synth.strain_segments(1, seed=100 + n, n_samples=n)
    out = ops.logmel(T.from_numpy(w).cuda()).cpu().numpy()[0]
    ref = g[f"len{n}_frames"]
    np.testing.assert_allclose(out[:, :ref.shape[1]], ref, atol=2e-5, rtol=0)
    assert abs(out[0, 2999] - g[f"len{n}_pad_value"]) < 2e-5


@pytest.mark.parametrize("n", [480000, 480321])
def test_logmel_full_buffer_and_truncation(T, gww, golden, n):
    from gw_whisper_amd import ops
    g = golden("logmel.npz")
    w = synth.strain_segments(1, seed=200 + n, n_samples=n)
    out = ops.logmel(T.from_numpy(w).cuda()).cpu().numpy()[0]
    np.testing.assert_allclose(out[:, g[f"len{n}_cols"]], g[f"len{n}_frames"], atol=2e-5, rtol=0)


def test_logmel_constant_collapse_and_empty(T, gww, golden):
    from gw_whisper_amd import ops
    g = golden("logmel.npz")
    z = ops.logmel(T.zeros(1, 16000).cuda()).cpu().numpy()[0]
    assert z.min() == z.max() == g["zeros_value"][0] == -1.5
    r = ops.logmel(T.from_numpy((synth.strain_segments(1, seed=5) * 1e-21).astype(np.float32)).cuda()).cpu().numpy()[0]
    assert r.min() == g["raw1e21_value"][0] and r.max() == g["raw1e21_value"][1]
    e = ops.logmel(T.zeros(0, 16000).cuda())
    assert tuple(e.shape) == (0, 80, 3000)


def test_logmel_idempotent_batching(T, gww):
    """Size-independent property: a segment's features do not depend on its batch."""
    from gw_whisper_amd import ops
    seg = synth.strain_segments(37, seed=2)
    a = ops.logmel(T.from_numpy(seg).cuda()).cpu().numpy()
    b = ops.logmel(T.from_numpy(seg[5:6]).cuda()).cpu().numpy()
    assert np.array_equal(a[5], b[0])


# ------------------------------------------------------------------ LayerNorm / cast
@pytest.mark.parametrize("d", [128, 384, 512, 768, 1024, 1280])
def test_layernorm(T, gww, d):
    from gw_whisper_amd import ops
    rng = np.random.default_rng(d)
    x = (rng.standard_normal((1003, d)) * 3 + 0.5).astype(np.float32)
    w = (1 + 0.1 * rng.standard_normal(d)).astype(np.float32)
    b = (0.1 * rng.standard_normal(d)).astype(np.float32)
    ref = oenc.layer_norm(x.astype(np.float64), w, b)
    y = ops.layernorm(T.from_numpy(x).cuda(), T.from_numpy(w).cuda(), T.from_numpy(b).cuda()).cpu().numpy()
    np.testing.assert_allclose(y, ref, atol=3e-6, rtol=1e-5)
    yb = ops.layernorm(T.from_numpy(x).cuda(), T.from_numpy(w).cuda(), T.from_numpy(b).cuda(), out_bf16=True)
    # same fp32 value rounded to bf16; the two instantiations may contract the final FMA
    # differently, which flips a rounding tie in a handful of elements
    ybf = yb.float().cpu().numpy()
    np.testing.assert_allclose(ybf, _bf(y), atol=0, rtol=2 ** -7)
    assert (ybf == _bf(y)).mean() > 0.9999


def test_cast_bf16_round_to_nearest_even(T, gww):
    from gw_whisper_amd import ops
    rng = np.random.default_rng(0)
    x = rng.standard_normal(100003).astype(np.float32) * 10
    x[:4] = [1.00390625, 1.005859375, -0.0, 3.0e38]
    y = ops.cast_bf16(T.from_numpy(x).cuda()).float().cpu().numpy()
    np.testing.assert_array_equal(y, _bf(x))


# ------------------------------------------------------------------ GEMM
@pytest.mark.parametrize("M,N,K", [(128, 128, 64), (300, 384, 384), (1501, 1152, 384), (777, 384, 1536), (64, 1536, 384),
                                   # M % 256 == 0 and >= 4096: the persistent row-panel kernel (v2)
                                   (4096, 384, 384), (5120, 1152, 384), (4352, 384, 1536), (4096, 1536, 384), (8192, 128, 128),
                                   # whisper-small widths: N > 1536 runs the same kernel with the columns split over blocks
                                   (4096, 2304, 768), (4352, 3072, 768), (4096, 768, 3072), (4096, 5120, 128),
                                   # k_gemm_bf16_v4 (N % 256 == 0, N <= 3072, K % 128 == 0, M % 256 == 0): the smallest stream (one
                                   # tile of two k-tiles), one item per block, and MORE items than CUs -- a block's k-tile stream then
                                   # runs through several (panel, split) items: 300 / 260 panels x 2 / 1 splits
                                   (256, 256, 128), (512, 512, 256), (76800, 512, 256), (66560, 256, 384), (2560, 3072, 128)])
@pytest.mark.parametrize("epi", [0, 1, 2])
def test_gemm_bf16(T, gww, M, N, K, epi):
    from gw_whisper_amd import ops
    rng = np.random.default_rng(M * 7 + N + K + epi)
    a = _bf(rng.standard_normal((M, K)))
    w = _bf(rng.standard_normal((N, K)) / np.sqrt(K))
    bias = rng.standard_normal(N).astype(np.float32)
    resid = rng.standard_normal((M, N)).astype(np.float32)
    ref = a.astype(np.float64) @ w.astype(np.float64).T + bias
    if epi == 1:
        ref = oenc.gelu(ref)
    if epi == 2:
        ref = ref + resid
    c = ops.gemm(T.from_numpy(a).cuda().bfloat16(), T.from_numpy(w).cuda().bfloat16(), T.from_numpy(bias).cuda(),
                 epilogue=epi, resid=T.from_numpy(resid).cuda() if epi == 2 else None)
    got = c.float().cpu().numpy()
    if epi == 2:
        # fp32 out: only fp32 accumulation-order noise
        np.testing.assert_allclose(got, ref, atol=2e-5 * np.sqrt(K), rtol=1e-5)
    else:
        # bf16 out: one rounding of the exact result
        np.testing.assert_allclose(got, ref, atol=1e-5 * np.sqrt(K), rtol=2 ** -8)


@pytest.mark.parametrize("M,N,K", [(4096, 1536, 384), (66560, 1536, 256), (2560, 3072, 128)])
@pytest.mark.parametrize("epi", [0, 1, 2])
def test_gemm_v4_result_does_not_depend_on_the_column_split(T, gww, M, N, K, epi):
    """k_gemm_bf16_v4: an output element's accumulation order does not depend on how the column tiles are dealt to work
    items, so every column split (gww_gemm_bf16_v4_split: 1 .. N / 256 tiles per item, i.e. one to many tiles per item,
    items per block and residual preloads across tile AND item boundaries) must give bit-identical results -- and the fp64
    product."""
    from gw_whisper_amd import ops
    rng = np.random.default_rng(M + N + K + epi)
    a = T.from_numpy(_bf(rng.standard_normal((M, K)))).cuda().bfloat16()
    w = T.from_numpy(_bf(rng.standard_normal((N, K)) / np.sqrt(K))).cuda().bfloat16()
    bias = T.from_numpy(rng.standard_normal(N).astype(np.float32)).cuda()
    resid = T.from_numpy(rng.standard_normal((M, N)).astype(np.float32)).cuda() if epi == 2 else None
    tn = N // 256
    outs = {}
    for split in [s for s in range(1, tn + 1) if tn % s == 0]:
        outs[split] = ops.gemm_v4_split(a, w, bias, epilogue=epi, resid=resid, n_split=split)
    auto = ops.gemm(a, w, bias, epilogue=epi, resid=resid)
    assert T.equal(auto, ops.gemm_v4_split(a, w, bias, epilogue=epi, resid=resid, n_split=0))   # gww_gemm_bf16 took this kernel
    for split, o in outs.items():
        assert T.equal(o, auto), f"split {split} differs from the automatic split"
    if M <= 4096:
        ref = a.double() @ w.double().T + bias.double()
        if epi == 1:
            ref = T.nn.functional.gelu(ref)
        if epi == 2:
            ref = ref + resid.double()
        tol = dict(atol=2e-5 * np.sqrt(K), rtol=1e-5) if epi == 2 else dict(atol=1e-5 * np.sqrt(K), rtol=2 ** -8)
        np.testing.assert_allclose(auto.double().cpu().numpy(), ref.cpu().numpy(), **tol)


@pytest.mark.parametrize("M,N,K", [(256, 128, 384), (1500, 1152, 384), (3000, 384, 384), (777, 1536, 384),
                                   (512, 256, 256), (300, 512, 512), (5000, 1536, 384), (6000, 1024, 512)])
@pytest.mark.parametrize("epi", [0, 1])
def test_gemm_astat_bf16(T, gww, M, N, K, epi):
    """A panel held in registers, W through the LDS-DMA ring (gemm_astat.hip)."""
    from gw_whisper_amd import ops
    rng = np.random.default_rng(M * 3 + N + K + epi)
    a = _bf(rng.standard_normal((M, K)))
    w = _bf(rng.standard_normal((N, K)) / np.sqrt(K))
    bias = rng.standard_normal(N).astype(np.float32)
    ref = a.astype(np.float64) @ w.astype(np.float64).T + bias
    if epi == 1:
        ref = oenc.gelu(ref)
    c = ops.gemm_astat(T.from_numpy(a).cuda().bfloat16(), T.from_numpy(w).cuda().bfloat16(),
                       T.from_numpy(bias).cuda(), epilogue=epi)
    got = c.float().cpu().numpy()
    assert got.shape == (M, N)
    np.testing.assert_allclose(got, ref, atol=1e-5 * np.sqrt(K), rtol=2 ** -8)


@pytest.mark.parametrize("M,N,K", [(256, 1152, 384), (1500, 1536, 384), (700, 512, 512), (3000, 2048, 512),
                                   (9000, 1536, 512)])
@pytest.mark.parametrize("epi", [0, 1])
@pytest.mark.parametrize("with_delta", [False, True])
def test_gemm_astat_fused_layernorm(T, gww, M, N, K, epi, with_delta):
    """Deferred residual add + LayerNorm applied algebraically inside the GEMM (one pass over x):
    equals Linear(LayerNorm(x + delta)) up to bf16 operand rounding, x_new is written back exactly,
    also for rows with a large common offset (mean >> sigma)."""
    from gw_whisper_amd import ops
    rng = np.random.default_rng(M + N + K + epi)
    x = (rng.standard_normal((M, K)) * 2 + 0.3).astype(np.float32)
    x[::7] += 25.0                                   # rows whose mean dwarfs their spread
    dl = _bf(rng.standard_normal((M, K)) * 0.5) if with_delta else None
    lw = (1 + 0.1 * rng.standard_normal(K)).astype(np.float32)
    lb = (0.1 * rng.standard_normal(K)).astype(np.float32)
    w = (rng.standard_normal((N, K)) / np.sqrt(K)).astype(np.float32)
    bias = rng.standard_normal(N).astype(np.float32)
    xn = x + dl if with_delta else x
    ref = oenc.layer_norm(xn.astype(np.float64), lw, lb) @ w.astype(np.float64).T + bias
    if epi == 1:
        ref = oenc.gelu(ref)
    wf, u, cb = ops.ln_fold_weights(T.from_numpy(w).cuda(), T.from_numpy(lw).cuda(), T.from_numpy(lb).cuda(),
                                    T.from_numpy(bias).cuda())
    # the folding itself
    np.testing.assert_array_equal(wf.float().cpu().numpy(), _bf(w * lw[None, :]))
    np.testing.assert_allclose(u.cpu().numpy(), _bf(w * lw[None, :]).astype(np.float64).sum(1), rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(cb.cpu().numpy(), bias + w.astype(np.float64) @ lb, rtol=1e-5, atol=1e-5)
    c, x_new = ops.gemm_astat(T.from_numpy(x).cuda(), wf, None, epilogue=epi, ln=(u, cb),
                              delta=T.from_numpy(dl).cuda().bfloat16() if with_delta else None, return_x=True)
    np.testing.assert_array_equal(x_new.cpu().numpy(), xn.astype(np.float32))
    got = c.float().cpu().numpy()
    # bf16 rounding of the shifted operand and of the folded weight (2^-9 each, K terms) + bf16 output
    np.testing.assert_allclose(got, ref, atol=3e-2, rtol=2 ** -7)
    assert np.sqrt(((got - ref) ** 2).mean()) < 6e-3


@pytest.mark.parametrize("M,N,K", [(128, 384, 64), (1500, 384, 1536), (777, 384, 1152), (300, 512, 2048), (4000, 384, 128)])
@pytest.mark.parametrize("epi", [0, 1])
def test_gemm_fulln_bf16(T, gww, M, N, K, epi):
    """Complete output rows per workgroup, A streamed once (gemm_fulln.hip)."""
    from gw_whisper_amd import ops
    rng = np.random.default_rng(M * 5 + N + K + epi)
    a = _bf(rng.standard_normal((M, K)))
    w = _bf(rng.standard_normal((N, K)) / np.sqrt(K))
    bias = rng.standard_normal(N).astype(np.float32)
    ref = a.astype(np.float64) @ w.astype(np.float64).T + bias
    if epi == 1:
        ref = oenc.gelu(ref)
    c = ops.gemm_fulln(T.from_numpy(a).cuda().bfloat16(), T.from_numpy(w).cuda().bfloat16(), T.from_numpy(bias).cuda(),
                       epilogue=epi)
    got = c.float().cpu().numpy()
    assert got.shape == (M, N)
    np.testing.assert_allclose(got, ref, atol=1e-5 * np.sqrt(K), rtol=2 ** -8)


@pytest.mark.parametrize("M,N,K", [(64, 64, 32), (300, 384, 384), (1501, 128, 96)])
@pytest.mark.parametrize("epi", [0, 1, 2])
def test_gemm_f32(T, gww, M, N, K, epi):
    from gw_whisper_amd import ops
    rng = np.random.default_rng(M + N + K + epi)
    a = rng.standard_normal((M, K)).astype(np.float32)
    w = (rng.standard_normal((N, K)) / np.sqrt(K)).astype(np.float32)
    bias = rng.standard_normal(N).astype(np.float32)
    resid = rng.standard_normal((M, N)).astype(np.float32)
    ref = a.astype(np.float64) @ w.astype(np.float64).T + bias
    if epi == 1:
        ref = oenc.gelu(ref)
    if epi == 2:
        ref = ref + resid
    c = ops.gemm(T.from_numpy(a).cuda(), T.from_numpy(w).cuda(), T.from_numpy(bias).cuda(), epilogue=epi,
                 resid=T.from_numpy(resid).cuda() if epi == 2 else None)
    np.testing.assert_allclose(c.cpu().numpy(), ref, atol=3e-6 * np.sqrt(K), rtol=1e-5)


def test_gemm_identity_with_asymmetric_operand(T, gww):
    """A = I against an asymmetric W catches a transposed C write (guide section 3)."""
    from gw_whisper_amd import ops
    n = 128
    a = np.eye(n, dtype=np.float32)
    w = _bf(np.arange(n * n, dtype=np.float32).reshape(n, n) % 251 - 100.0)
    c = ops.gemm(T.from_numpy(a).cuda().bfloat16(), T.from_numpy(w).cuda().bfloat16()).float().cpu().numpy()
    np.testing.assert_array_equal(c, w.T)


# ------------------------------------------------------------------ attention
def _attn_ref(qkv, H, bf16):
    B, Tn, d3 = qkv.shape
    d = d3 // 3
    q, k, v = qkv[..., :d], qkv[..., d:2 * d], qkv[..., 2 * d:]
    return oenc.attention(q.astype(np.float64), k.astype(np.float64), v.astype(np.float64), H, bf16, np.float64)


@pytest.mark.parametrize("B,Tn,H", [(1, 64, 1), (2, 200, 2), (1, 1500, 2), (3, 129, 6)])
def test_attention_bf16(T, gww, B, Tn, H):
    from gw_whisper_amd import ops
    rng = np.random.default_rng(B * 1000 + Tn + H)
    qkv = _bf(rng.standard_normal((B, Tn, 3 * H * 64)) * 0.7)
    ref = _attn_ref(qkv, H, True)
    got = ops.attention(T.from_numpy(qkv).cuda().bfloat16(), H).float().cpu().numpy()
    # bf16 P and bf16 output rounding on |ctx| <~ 1
    np.testing.assert_allclose(got, ref, atol=6e-3, rtol=2 ** -7)


# (the log2-unit-q operand and its fp64 reference are shared with test_gpu_whisper_like.py)
from tests.whisper_like import LOG2E as _LOG2E, attn_ref_log2q as _attn_ref_log2q, to_log2q as _to_log2q  # noqa: E402


@pytest.fixture(params=["default"])
def att_variant(request):
    """The log2-unit-q kernel of the product library: k_attention_dma_bf16<3, false, true>.  The kept-off variants
    (k_attention_l2_bf16, k_attention_pp_bf16, the other k_attention_dma_bf16 instantiations and round 4's one-wave-per-SIMD
    k_attention_w64_bf16) are compiled into the laboratory build only (make LAB=1 -> libgww_lab.so, where GWW_ATT_VAR /
    GWW_ATT_W64 select them; tools/run/att_w64_ab.py runs these same cases' shapes on both)."""
    return request.param


@pytest.mark.parametrize("B,Tn,H", [(1, 64, 1), (1, 37, 1), (2, 200, 2), (1, 128, 1), (1, 192, 2), (1, 1500, 2),
                                    (3, 129, 6), (2, 257, 1), (1, 1, 1), (2, 65, 2), (1, 256, 1), (2, 300, 3), (1, 513, 2),
                                    (1, 31, 2), (1, 33, 1), (2, 96, 1), (1, 1472, 1)])
def test_attention_log2q(T, gww, att_variant, B, Tn, H):
    """The log2-unit-q kernel (reference through the matrix pipe, first tile re-based, deferred re-basing later):
    one, two, three ... tiles, ragged and full last tiles, a single key, and the log-sum-exp it hands to
    training-style consumers."""
    from gw_whisper_amd import ops
    rng = np.random.default_rng(B * 1000 + Tn + H)
    qkv = _to_log2q(_bf(rng.standard_normal((B, Tn, 3 * H * 64)) * 0.7))
    ref = _attn_ref_log2q(qkv, H)
    got, lse = ops.attention_log2q(T.from_numpy(qkv).cuda().bfloat16(), H, want_lse=True)
    np.testing.assert_allclose(got.float().cpu().numpy(), ref, atol=6e-3, rtol=2 ** -7)
    d = H * 64
    q = qkv[..., :d].astype(np.float64) / _LOG2E
    k = qkv[..., d:2 * d].astype(np.float64)
    for h in range(H):
        s = np.einsum("bqd,bkd->bqk", q[..., h * 64:(h + 1) * 64], k[..., h * 64:(h + 1) * 64])
        m = s.max(-1, keepdims=True)
        ref_lse = (m + np.log(np.exp(s - m).sum(-1, keepdims=True)))[..., 0]
        np.testing.assert_allclose(lse[:, h].cpu().numpy(), ref_lse, atol=2e-2, rtol=1e-3)


@pytest.mark.parametrize("offset", [-100.0, -12.0, 0.0, 9.0, 100.0])
def test_attention_log2q_uniform_score_offsets(T, gww, att_variant, offset):
    """Rows whose scores are ALL far below or above zero: softmax is shift-invariant, the kernel must be too (the first
    tile is scored against reference 0 and then re-based -- 2^-144 would underflow to l = 0, 2^+144 overflow)."""
    from gw_whisper_amd import ops
    rng = np.random.default_rng(11)
    H, Tn = 2, 300
    qkv = (rng.standard_normal((1, Tn, 3 * H * 64)) * 0.4).astype(np.float32)
    qkv[0, :, 0] = 1.0                       # q[:, 0] = 1 in head 0 ...
    qkv[0, :, 128] = offset                  # ... and k[:, 0] = offset: every score of head 0 moves by `offset`
    qkv = _to_log2q(_bf(qkv))
    ref = _attn_ref_log2q(qkv, H)
    got, lse = ops.attention_log2q(T.from_numpy(qkv).cuda().bfloat16(), H, want_lse=True)
    assert T.isfinite(got).all() and T.isfinite(lse).all()
    np.testing.assert_allclose(got.float().cpu().numpy(), ref, atol=6e-3, rtol=2 ** -7)


def test_attention_log2q_staircase_rebases_at_every_tile(T, gww, att_variant):
    """The best key of every query moves up by ~14 (natural units, above the deferral threshold) from each 64-key tile
    to the next: a re-base in every tile, nine in a row."""
    from gw_whisper_amd import ops
    rng = np.random.default_rng(12)
    H, Tn = 1, 600
    qkv = (rng.standard_normal((1, Tn, 192)) * 0.2).astype(np.float32)
    qkv[0, :, 0] = 1.0
    qkv[0, :, 64] = 14.0 * (np.arange(Tn) // 64)          # k[:, 0]: staircase over the key tiles
    qkv = _to_log2q(_bf(qkv))
    ref = _attn_ref_log2q(qkv, H)
    got = ops.attention_log2q(T.from_numpy(qkv).cuda().bfloat16(), H).float().cpu().numpy()
    assert np.isfinite(got).all()
    np.testing.assert_allclose(got, ref, atol=6e-3, rtol=2 ** -7)


def test_attention_log2q_spike_forces_rebase(T, gww, att_variant):
    """A key far above the running reference late in the sequence (score 256): O, l AND the scores of the tile
    computed against the old reference must move to the new one; then a long tail of small scores."""
    from gw_whisper_amd import ops
    rng = np.random.default_rng(5)
    H, Tn = 1, 600
    qkv = (rng.standard_normal((1, Tn, 192)) * 0.3).astype(np.float32)
    qkv[0, 17, :64] = 2.0
    qkv[0, 450, 64:128] = 2.0
    qkv[0, 300, :64] = -3.0            # a row whose scores are all very negative against key 450
    qkv = _to_log2q(_bf(qkv))
    ref = _attn_ref_log2q(qkv, H)
    got = ops.attention_log2q(T.from_numpy(qkv).cuda().bfloat16(), H).float().cpu().numpy()
    assert np.isfinite(got).all()
    np.testing.assert_allclose(got, ref, atol=6e-3, rtol=2 ** -7)
    np.testing.assert_allclose(got[0, 17], qkv[0, 450, 128:192], atol=1e-2)


def test_attention_bf16_spike_forces_rescale(T, gww):
    """One key dominates one query late in the sequence: the running max jumps at a
    chosen tile and every earlier partial sum must be rescaled (guide rule 26)."""
    from gw_whisper_amd import ops
    rng = np.random.default_rng(5)
    H, Tn = 1, 600
    qkv = (rng.standard_normal((1, Tn, 192)) * 0.3).astype(np.float32)
    qkv[0, 17, :64] = 2.0             # q row 17
    qkv[0, 450, 64:128] = 2.0         # k row 450 -> score 256 vs O(1) elsewhere
    qkv = _bf(qkv)
    ref = _attn_ref(qkv, H, True)
    got = ops.attention(T.from_numpy(qkv).cuda().bfloat16(), H).float().cpu().numpy()
    np.testing.assert_allclose(got, ref, atol=6e-3, rtol=2 ** -7)
    np.testing.assert_allclose(got[0, 17], qkv[0, 450, 128:192], atol=1e-2)   # row 17 == v[450]


@pytest.mark.parametrize("B,Tn,H", [(1, 32, 1), (2, 200, 2), (1, 1500, 2)])
def test_attention_f32(T, gww, B, Tn, H):
    from gw_whisper_amd import ops
    rng = np.random.default_rng(B * 1000 + Tn + H + 1)
    qkv = (rng.standard_normal((B, Tn, 3 * H * 64)) * 0.7).astype(np.float32)
    ref = _attn_ref(qkv, H, False)
    got = ops.attention(T.from_numpy(qkv).cuda(), H).cpu().numpy()
    np.testing.assert_allclose(got, ref, atol=2e-5, rtol=1e-4)


# ------------------------------------------------------------------ DoRA merge
@pytest.mark.parametrize("d_out,d_in,r", [(384, 384, 8), (768, 768, 16), (1536, 384, 8)])
def test_dora_merge(T, gww, d_out, d_in, r):
    from gw_whisper_amd import ops
    rng = np.random.default_rng(d_out + r)
    W0 = (rng.standard_normal((d_out, d_in)) / np.sqrt(d_in)).astype(np.float32)
    A, B, m = synth.dora_adapter(d_out, d_in, r, W0, seed=3)
    s = 32.0 / r
    ref = odora.dora_merge(W0.astype(np.float64), A.astype(np.float64), B.astype(np.float64), m.astype(np.float64), s)
    refn = odora.dora_weight_norm(W0.astype(np.float64), A.astype(np.float64), B.astype(np.float64), s)
    got, nrm = ops.dora_merge(*(T.from_numpy(t).cuda() for t in (W0, A, B, m)), s, return_norm=True)
    np.testing.assert_allclose(got.cpu().numpy(), ref, atol=2e-6, rtol=1e-5)
    np.testing.assert_allclose(nrm.cpu().numpy(), refn, rtol=1e-5)
    # identity at init: B = 0, m = ||W0||
    A0, B0, m0 = synth.dora_adapter(d_out, d_in, r, W0, seed=3, trained=False)
    got0 = ops.dora_merge(*(T.from_numpy(t).cuda() for t in (W0, A0, B0, m0)), s)
    np.testing.assert_allclose(got0.cpu().numpy(), W0, atol=1e-6, rtol=1e-6)


@pytest.mark.parametrize("B,Tn,d", [(2, 3000, 384), (3, 100, 384), (2, 257, 384), (1, 128, 512), (2, 129, 768), (1, 1, 1024),
                                    (300, 40, 384)])
def test_conv1_gelu_from_the_feature_layout(T, gww, B, Tn, d):
    """gww_conv1_gelu_bf16 (conv1_mel.hip: conv1 + GELU read straight from [B, 80, T], HF:modeling_whisper.py:619-620)
    against torch's fp64 Conv1d + erf GELU on the same bf16-rounded operands; ragged chunk tails (T % 128 != 0), a single
    sample, more chunks than workgroups; the padding rows 0 and T + 1 of every segment must be exact zeros."""
    from gw_whisper_amd import ops
    rng = np.random.default_rng(B * 7 + Tn + d)
    mel = T.from_numpy(rng.standard_normal((B, 80, Tn)).astype(np.float32) * 0.8)
    w = T.from_numpy((rng.standard_normal((d, 80, 3)) / np.sqrt(240)).astype(np.float32))
    b = T.from_numpy(rng.standard_normal(d).astype(np.float32) * 0.3)
    got = ops.conv1_gelu(mel.cuda(), w.cuda(), b.cuda())
    assert got.shape == (B, Tn + 2, d) and got.dtype == T.bfloat16
    got = got.float().cpu()
    assert T.count_nonzero(got[:, 0]) == 0 and T.count_nonzero(got[:, Tn + 1]) == 0
    r16 = lambda t: t.to(T.bfloat16).to(T.float64)
    ref = T.nn.functional.gelu(T.nn.functional.conv1d(r16(mel), r16(w), b.double(), padding=1)).transpose(1, 2)
    err = (got[:, 1:Tn + 1].double() - ref).abs()
    assert float((err - (2.0 ** -8) * ref.abs()).max()) < 1e-3, float(err.max())


def test_dora_merge_batch_equals_the_single_merges(T, gww):
    """gww_dora_merge_batch_f32: 45 modules of mixed shape and rank (more than one 40-op descriptor table) in one call,
    bit-identical to the per-module kernel and within the oracle's tolerance."""
    from gw_whisper_amd import ops
    shapes = [(384, 384, 8), (768, 768, 16), (1536, 384, 8), (384, 1536, 4), (512, 512, 32)] * 9
    items, refs = [], []
    for i, (d_out, d_in, r) in enumerate(shapes):
        rng = np.random.default_rng(100 + i)
        W0 = (rng.standard_normal((d_out, d_in)) / np.sqrt(d_in)).astype(np.float32)
        A, B, m = synth.dora_adapter(d_out, d_in, r, W0, seed=i)
        items.append(tuple(T.from_numpy(t).cuda() for t in (W0, A, B, m)) + (32.0 / r,))
        if i < 5:
            refs.append(odora.dora_merge(*(t.astype(np.float64) for t in (W0, A, B, m)), 32.0 / r))
    got = ops.dora_merge_batch(items)
    assert len(got) == len(items)
    for i, (it, (w, nrm)) in enumerate(zip(items, got)):
        w1, n1 = ops.dora_merge(*it[:4], it[4], return_norm=True)
        assert T.equal(w, w1) and T.equal(nrm, n1), i
    for ref, (w, _) in zip(refs, got):
        np.testing.assert_allclose(w.cpu().numpy(), ref, atol=2e-6, rtol=1e-5)
    assert ops.dora_merge_batch([]) == []


def test_mlp_pack_layout(T, gww):
    """Tile stream of the fused MLP, in the order the kernel consumes it over 64-column ffn chunks c':
    G1(0) | G1(1) G2(0) | G1(2) G2(1) | ... | G1(n-1) G2(n-2) | G2(n-1); fc1 tiles are swizzled [64 n][128 k] images,
    fc2 tiles [128 n][64 k] carry k with bits 2 / 3 swapped inside every 16-group.  The fc1 images hold W1' / 8 and the
    fc2 images 8 W2 (exact powers of two: the kernel's fc1 accumulators then hold S / 8, which lets the GELU clamp ride
    on an instruction modifier -- mlp_fused.hip, gelu_slice)."""
    from gw_whisper_amd import ops
    F, d = 256, 384
    w1 = T.arange(F * d, dtype=T.float32).reshape(F, d).remainder(251).cuda().bfloat16()
    w2 = (T.arange(d * F, dtype=T.float32).reshape(d, F).remainder(241) + 0.5).cuda().bfloat16()
    n = F // 64
    out = ops.mlp_pack(w1, w2).float().cpu().numpy().reshape(6 * n, 8192)
    w1n, w2n = w1.float().cpu().numpy(), w2.float().cpu().numpy()
    k = np.arange(64)
    sw = (k & ~12) | ((k & 4) << 1) | ((k & 8) >> 1)
    order = [("g1", 0, i) for i in range(3)]
    for blk in range(n):
        if blk + 1 < n:
            order += [("g1", blk + 1, i) for i in range(3)]
        order += [("g2", blk, i) for i in range(3)]
    assert len(order) == 6 * n
    for tile, (kind, cp, idx3) in enumerate(order):
        if kind == "g1":     # fc1: [64 n][128 k], chunk ^ (row & 15); rows 64 cp .., k-third idx3
            img = out[tile].reshape(64, 16, 8)
            for row in (0, 1, 17, 63):
                logical = np.stack([img[row, ch ^ (row & 15)] for ch in range(16)]).reshape(128)
                np.testing.assert_array_equal(logical, w1n[64 * cp + row, 128 * idx3:128 * idx3 + 128] / 8)
        else:                # fc2: [128 n2][64 k], chunk ^ ((row >> 1) & 7); n-group idx3, k = ffn columns of chunk cp
            img = out[tile].reshape(128, 8, 8)
            for row in (0, 1, 2, 77, 127):
                logical = np.stack([img[row, ch ^ ((row >> 1) & 7)] for ch in range(8)]).reshape(64)
                np.testing.assert_array_equal(logical, 8 * w2n[128 * idx3 + row, 64 * cp:64 * cp + 64][sw])


@pytest.mark.parametrize("with_qkv", [False, True], ids=["plain", "qkv"])
@pytest.mark.parametrize("M", [128, 1500, 777, 70000])
def test_attn_out_mlp_fused(T, gww, M, with_qkv):
    """The attention output projection fused IN FRONT of the MLP block (``gww_attn_out_mlp_fused_bf16``): it must produce
    what the unfused sequence produces -- out_proj as a stand-alone bf16 GEMM (delta rounded to bf16), the deferred
    residual add and ``mlp_fused`` -- to the last bf16 rounding of the delta: x_new against x + bf16(ctx Wo^T + bo) in
    fp64 (a delta element may round the other way: one bf16 ulp of the delta), outputs against the unfused kernels."""
    from gw_whisper_amd import ops
    d, F, NQ = 384, 1536, 1152
    rng = np.random.default_rng(M + 5)
    x = (rng.standard_normal((M, d)) * 2 + 0.3).astype(np.float32)
    x[::7] += 25.0
    ctx = _bf(rng.standard_normal((M, d)))
    wo = _bf(rng.standard_normal((d, d)) / np.sqrt(d))
    bo = rng.standard_normal(d).astype(np.float32)
    g = lambda n: (1 + 0.1 * rng.standard_normal(n)).astype(np.float32)
    sm = lambda n: (0.1 * rng.standard_normal(n)).astype(np.float32)
    lw, lb, lw1, lb1 = g(d), sm(d), g(d), sm(d)
    w1 = (rng.standard_normal((F, d)) / np.sqrt(d)).astype(np.float32)
    b1 = rng.standard_normal(F).astype(np.float32)
    w2 = (rng.standard_normal((d, F)) / np.sqrt(F)).astype(np.float32)
    b2 = rng.standard_normal(d).astype(np.float32)
    wq = (rng.standard_normal((NQ, d)) / np.sqrt(d)).astype(np.float32)
    bq = rng.standard_normal(NQ).astype(np.float32)
    c = lambda a: T.from_numpy(np.asarray(a)).cuda()
    w1f, u, cb = ops.ln_fold_weights(c(w1), c(lw), c(lb), c(b1))
    wqf, uq, cq = ops.ln_fold_weights(c(wq), c(lw1), c(lb1), c(bq))
    got, got_x = ops.attn_out_mlp_fused(c(x), c(ctx).bfloat16(), c(wo).bfloat16(), c(bo), w1f, c(w2).bfloat16(), u, cb, c(b2),
                                        qkv=(wqf, uq, cq) if with_qkv else None)
    # the delta the stand-alone out_proj emits, in fp64 then bf16
    delta = ctx.astype(np.float64) @ wo.astype(np.float64).T + bo
    x_new_ref = x.astype(np.float64) + _bf(delta).astype(np.float64)
    ulp = np.abs(delta) * 2.0 ** -7 + 1e-6
    if not with_qkv:
        assert (np.abs(got_x.cpu().numpy() - x_new_ref) <= ulp + 2e-5).all()
        assert np.abs(got_x.cpu().numpy() - x_new_ref).mean() < 1e-4        # almost every element rounds the same way
    # the unfused kernels on the same operands
    delta_dev = ops.gemm_astat(c(ctx).bfloat16(), c(wo).bfloat16(), c(bo))[:M].contiguous()
    if with_qkv:
        wt = ops.mlp_pack(w1f, c(w2).bfloat16(), wqf)
        ref, ref_x = ops.mlp_fused(c(x), delta_dev, wt, u, cb, c(b2), qkv=(uq, cq))
    else:
        wt = ops.mlp_pack(w1f, c(w2).bfloat16())
        ref, ref_x = ops.mlp_fused(c(x), delta_dev, wt, u, cb, c(b2))
    a, b = got.float().cpu().numpy(), ref.float().cpu().numpy()
    # a delta element that rounds the other way moves LayerNorm's input by one bf16 ulp of the delta: outputs agree to a
    # few bf16 ulps of themselves, the residual stream to that ulp
    assert np.abs(got_x.cpu().numpy() - ref_x.cpu().numpy()).max() <= (np.abs(delta).max() * 2.0 ** -7 + 1e-3) * (2 if with_qkv else 1)
    np.testing.assert_allclose(a, b, atol=6e-2, rtol=2 ** -6)
    assert np.sqrt(((a - b) ** 2).mean()) < 8e-3


def _block_operands(rng, M, d=384, F=1536, NQ=1152):
    x = (rng.standard_normal((M, d)) * 2 + 0.3).astype(np.float32)
    x[::7] += 25.0
    g = lambda n: (1 + 0.1 * rng.standard_normal(n)).astype(np.float32)
    sm = lambda n: (0.1 * rng.standard_normal(n)).astype(np.float32)
    return dict(x=x, ctx=_bf(rng.standard_normal((M, d))), wo=_bf(rng.standard_normal((d, d)) / np.sqrt(d)),
                bo=rng.standard_normal(d).astype(np.float32), lw=g(d), lb=sm(d), lw1=g(d), lb1=sm(d),
                w1=(rng.standard_normal((F, d)) / np.sqrt(d)).astype(np.float32), b1=rng.standard_normal(F).astype(np.float32),
                w2=_bf(rng.standard_normal((d, F)) / np.sqrt(F)), b2=rng.standard_normal(d).astype(np.float32),
                wq=(rng.standard_normal((NQ, d)) / np.sqrt(d)).astype(np.float32), bq=rng.standard_normal(NQ).astype(np.float32))


def _block_fp64(o):
    """x_mid, the bf16-rounded MLP delta and x_next of one block in fp64 (HF:modeling_whisper.py:396-407)."""
    delta1 = _bf(o["ctx"].astype(np.float64) @ o["wo"].astype(np.float64).T + o["bo"]).astype(np.float64)
    x_mid = o["x"].astype(np.float64) + delta1
    h = oenc.gelu(oenc.layer_norm(x_mid, o["lw"], o["lb"]) @ o["w1"].astype(np.float64).T + o["b1"])
    mlp = h @ o["w2"].astype(np.float64).T + o["b2"]
    return x_mid, mlp


@pytest.mark.parametrize("M", [128, 1500, 777, 9000])
def test_attn_out_mlp_qkv_fused_against_fp64(T, gww, M):
    """The dominant kernel of the forward, k_mlp_fused<1, true> (out_proj + LN2 + fc1 + GELU + fc2 + next LN1 + q/k/v),
    against fp64 end to end (round-2 review: its outputs had only been compared with other HIP kernels): x_next to the
    bf16 rounding of the two deltas, q/k/v to bf16 operand + output rounding of LayerNorm_1(x_next) Wqkv^T + b."""
    from gw_whisper_amd import ops
    o = _block_operands(np.random.default_rng(M + 11), M)
    c = lambda a: T.from_numpy(np.asarray(a)).cuda()
    w1f, u, cb = ops.ln_fold_weights(c(o["w1"]), c(o["lw"]), c(o["lb"]), c(o["b1"]))
    wqf, uq, cq = ops.ln_fold_weights(c(o["wq"]), c(o["lw1"]), c(o["lb1"]), c(o["bq"]))
    x_dev = c(o["x"])
    qkv, x_next = ops.attn_out_mlp_fused(x_dev, c(o["ctx"]).bfloat16(), c(o["wo"]).bfloat16(), c(o["bo"]), w1f,
                                         c(o["w2"]).bfloat16(), u, cb, c(o["b2"]), qkv=(wqf, uq, cq))
    assert T.equal(x_dev, c(o["x"]))                       # the wrapper hands the library a copy: x_next comes back over it
    x_mid, mlp = _block_fp64(o)
    x_next_ref = x_mid + mlp
    got_x = x_next.cpu().numpy().astype(np.float64)
    # each delta is rounded to bf16 before it is added (8 bits) and was computed from bf16 operands
    tol_x = np.abs(mlp) * 2.0 ** -7 + np.abs(x_mid - o["x"]) * 2.0 ** -7 + 4e-2
    assert (np.abs(got_x - x_next_ref) <= tol_x).all(), np.abs(got_x - x_next_ref).max()
    assert np.sqrt(((got_x - x_next_ref) ** 2).mean()) < 8e-3
    ref = oenc.layer_norm(got_x, o["lw1"], o["lb1"]) @ o["wq"].astype(np.float64).T + o["bq"]
    got = qkv.float().cpu().numpy()
    np.testing.assert_allclose(got, ref, atol=3e-2, rtol=2 ** -7)
    assert np.sqrt(((got - ref) ** 2).mean()) < 6e-3


@pytest.mark.parametrize("M", [128, 1500, 777, 9000])
def test_attn_out_mlp_final_layernorm_against_fp64(T, gww, M):
    """k_mlp_fused<3, true>: the LAST block with the encoder's final LayerNorm as its epilogue
    (HF:modeling_whisper.py:396-407, 642) against fp64; the fp32 output replaces delta + stand-alone LayerNorm."""
    from gw_whisper_amd import ops
    o = _block_operands(np.random.default_rng(M + 23), M)
    c = lambda a: T.from_numpy(np.asarray(a)).cuda()
    w1f, u, cb = ops.ln_fold_weights(c(o["w1"]), c(o["lw"]), c(o["lb"]), c(o["b1"]))
    y, x_mid_dev = ops.attn_out_mlp_final(c(o["x"]), c(o["ctx"]).bfloat16(), c(o["wo"]).bfloat16(), c(o["bo"]), w1f,
                                          c(o["w2"]).bfloat16(), u, cb, c(o["b2"]), c(o["lw1"]), c(o["lb1"]))
    x_mid, mlp = _block_fp64(o)
    assert np.abs(x_mid_dev.cpu().numpy() - x_mid).max() <= np.abs(x_mid - o["x"]).max() * 2.0 ** -7 + 1e-3
    # what the unfused path computes: LayerNorm(x_mid + bf16(mlp)) -- the kernel's own x_mid and delta rounding
    ref = oenc.layer_norm(x_mid_dev.cpu().numpy().astype(np.float64) + mlp, o["lw1"], o["lb1"])
    got = y.cpu().numpy().astype(np.float64)
    # the delta carries bf16 rounding (2^-8 relative) and bf16-operand error; LayerNorm divides by the row's sigma (~2.5)
    np.testing.assert_allclose(got, ref, atol=3e-2, rtol=0)
    assert np.sqrt(((got - ref) ** 2).mean()) < 4e-3
    # Since round 4 the residual stream stays in the kernel's output accumulators (fp32): neither delta is rounded to bf16 on
    # its way into it, so the result is CLOSER to fp64 than the stand-alone kernels' (bf16 delta + LayerNorm kernel), which it
    # used to reproduce bit for bit -- now it must agree with them to the two delta roundings they carry
    delta, x_mid2 = ops.attn_out_mlp_fused(c(o["x"]), c(o["ctx"]).bfloat16(), c(o["wo"]).bfloat16(), c(o["bo"]), w1f,
                                           c(o["w2"]).bfloat16(), u, cb, c(o["b2"]))
    dx = (x_mid2 - x_mid_dev).abs().cpu().numpy()
    assert (dx <= np.abs(x_mid - o["x"]) * 2.0 ** -8 + 1e-3).all(), dx.max()
    unfused = ops.layernorm(x_mid2 + delta.float(), c(o["lw1"]), c(o["lb1"]))
    assert (y - unfused).abs().max().item() < 3e-2
    ref64 = oenc.layer_norm(x_mid + mlp, o["lw1"], o["lb1"])
    assert np.sqrt(((got - ref64) ** 2).mean()) <= np.sqrt(((unfused.cpu().numpy() - ref64) ** 2).mean()) * 1.05 + 1e-4


@pytest.mark.parametrize("M", [128, 1500, 777, 70000])
def test_lnqkv_fused(T, gww, M):
    """LayerNorm + q / k / v projection of a residual stream without a pending delta (layer 0) on the fused MLP kernel's
    panel prologue and q / k / v tail (``gww_lnqkv_fused_bf16``) against fp64 LayerNorm + matmul; bf16 operand and
    output rounding set the tolerance (the stand-alone LN-fused GEMM is held to the same one)."""
    from gw_whisper_amd import ops
    rng = np.random.default_rng(M)
    d, NQ = 384, 1152
    x = (rng.standard_normal((M, d)) * 2 + rng.standard_normal((M, 1)) * 3).astype(np.float32)
    lw = (1 + 0.2 * rng.standard_normal(d)).astype(np.float32)
    lb = (0.1 * rng.standard_normal(d)).astype(np.float32)
    wq = (rng.standard_normal((NQ, d)) / np.sqrt(d)).astype(np.float32)
    bq = rng.standard_normal(NQ).astype(np.float32)
    c = lambda a: T.from_numpy(np.asarray(a)).cuda()
    wqf, uq, cq = ops.ln_fold_weights(c(wq), c(lw), c(lb), c(bq))
    wt = ops.mlp_pack(None, None, wqf)
    assert wt.numel() == NQ * d
    x_dev = c(x)
    got = ops.lnqkv_fused(x_dev, wt, uq, cq).float().cpu().numpy()
    assert np.array_equal(x_dev.cpu().numpy(), x)                      # x is only read
    x64 = x.astype(np.float64)
    mu, var = x64.mean(1, keepdims=True), x64.var(1, keepdims=True)
    ln = (x64 - mu) / np.sqrt(var + 1e-5) * lw + lb
    ref = ln @ wq.astype(np.float64).T + bq
    np.testing.assert_allclose(got, ref, atol=6e-2, rtol=2e-2)
    assert np.abs(got - ref).mean() < 6e-3


@pytest.mark.parametrize("M,F", [(128, 128), (1500, 1536), (777, 512), (4000, 1536), (70000, 1536)])
def test_mlp_fused(T, gww, M, F):
    """LayerNorm -> fc1 -> GELU -> fc2 of (x + delta) in one kernel (mlp_fused.hip) against fp64:
    HF:modeling_whisper.py:401-407 without the residual add (deferred to the consumer)."""
    from gw_whisper_amd import ops
    d = 384
    rng = np.random.default_rng(M + F)
    x = (rng.standard_normal((M, d)) * 2 + 0.3).astype(np.float32)
    x[::7] += 25.0
    dl = _bf(rng.standard_normal((M, d)) * 0.5)
    lw = (1 + 0.1 * rng.standard_normal(d)).astype(np.float32)
    lb = (0.1 * rng.standard_normal(d)).astype(np.float32)
    w1 = (rng.standard_normal((F, d)) / np.sqrt(d)).astype(np.float32)
    b1 = rng.standard_normal(F).astype(np.float32)
    w2 = (rng.standard_normal((d, F)) / np.sqrt(F)).astype(np.float32)
    b2 = rng.standard_normal(d).astype(np.float32)
    xn = x + dl
    h = oenc.gelu(oenc.layer_norm(xn.astype(np.float64), lw, lb) @ w1.astype(np.float64).T + b1)
    ref = h @ _bf(w2).astype(np.float64).T + b2
    c = lambda a: T.from_numpy(np.asarray(a)).cuda()
    w1f, u, cb = ops.ln_fold_weights(c(w1), c(lw), c(lb), c(b1))
    wt = ops.mlp_pack(w1f, c(w2).bfloat16())
    out, x_new = ops.mlp_fused(c(x), c(dl).bfloat16(), wt, u, cb, c(b2))
    np.testing.assert_array_equal(x_new.cpu().numpy(), xn.astype(np.float32))
    got = out.float().cpu().numpy()
    # bf16 operands twice (K = 384, then K = F) + bf16 output
    np.testing.assert_allclose(got, ref, atol=4e-2, rtol=2 ** -7)
    assert np.sqrt(((got - ref) ** 2).mean()) < 8e-3


@pytest.mark.parametrize("M", [128, 1500, 4000])
def test_mlp_fused_with_next_layers_qkv(T, gww, M):
    """mlp_fused with the NEXT layer's LayerNorm1 + q / k / v projection appended: x_next = x + delta + bf16(mlp),
    qkv = Linear_qkv(LayerNorm1(x_next)) -- against fp64 (HF:modeling_whisper.py:392-407 across the layer seam)."""
    from gw_whisper_amd import ops
    d, F, NQ = 384, 1536, 1152
    rng = np.random.default_rng(M)
    x = (rng.standard_normal((M, d)) * 2 + 0.3).astype(np.float32)
    x[::7] += 25.0
    dl = _bf(rng.standard_normal((M, d)) * 0.5)
    g = lambda n: (1 + 0.1 * rng.standard_normal(n)).astype(np.float32)
    sm = lambda n: (0.1 * rng.standard_normal(n)).astype(np.float32)
    lw, lb, lw1, lb1 = g(d), sm(d), g(d), sm(d)
    w1 = (rng.standard_normal((F, d)) / np.sqrt(d)).astype(np.float32)
    b1 = rng.standard_normal(F).astype(np.float32)
    w2 = (rng.standard_normal((d, F)) / np.sqrt(F)).astype(np.float32)
    b2 = rng.standard_normal(d).astype(np.float32)
    wq = (rng.standard_normal((NQ, d)) / np.sqrt(d)).astype(np.float32)
    bq = rng.standard_normal(NQ).astype(np.float32)
    c = lambda a: T.from_numpy(np.asarray(a)).cuda()
    w1f, u, cb = ops.ln_fold_weights(c(w1), c(lw), c(lb), c(b1))
    wqf, uq, cq = ops.ln_fold_weights(c(wq), c(lw1), c(lb1), c(bq))
    wt = ops.mlp_pack(w1f, c(w2).bfloat16(), wqf)
    qkv, x_next = ops.mlp_fused(c(x), c(dl).bfloat16(), wt, u, cb, c(b2), qkv=(uq, cq))
    # reference: the MLP delta exactly as the stand-alone kernel emits it (bf16), then the seam in fp64
    wt0 = ops.mlp_pack(w1f, c(w2).bfloat16())
    delta2, x_new = ops.mlp_fused(c(x), c(dl).bfloat16(), wt0, u, cb, c(b2))
    xn = x_new.cpu().numpy().astype(np.float64) + delta2.float().cpu().numpy().astype(np.float64)
    got_x = x_next.cpu().numpy()
    np.testing.assert_allclose(got_x, xn, atol=2e-5, rtol=1e-6)            # same bf16 delta, one fp32 add
    ref = oenc.layer_norm(got_x.astype(np.float64), lw1, lb1) @ wq.astype(np.float64).T + bq
    got = qkv.float().cpu().numpy()
    np.testing.assert_allclose(got, ref, atol=3e-2, rtol=2 ** -7)
    assert np.sqrt(((got - ref) ** 2).mean()) < 6e-3
