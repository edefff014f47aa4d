"""The training backward at every encoder width against float64: the DoRA step of two-layer encoders of whisper-base and
-medium width (the d = 512 route -- per-op forward, v4 / A-stationary / full-N dX GEMMs, the d = 512 multi-projection
DoRA kernel -- and the d = 1024 one, ``k_dora_grads<1024, 8>``) against fp64 autograd, and the backward building
blocks at the shapes the encoders run: LayerNorm backward at every d = 128 k, the DoRA-gradient kernels as the encoder
calls them (q / k / v sections of the packed qkv, log2-unit q scale), the attention backward at every head count and at
grids whose block count is not a multiple of 8, and the GELU-backward epilogue of the A-stationary GEMM.  Every
reference is evaluated in float64 on the same rounded inputs.  Needs an MI355X."""

import math

import numpy as np
import pytest

from gw_whisper_amd import synth
from oracle import logmel as olm
from tests.helpers import dora64

pytestmark = pytest.mark.gpu

LOG2E = 1.4426950408889634


@pytest.fixture(scope="module")
def T():
    import torch
    assert torch.cuda.is_available()
    return torch


def _bf(T, x):
    """float64 CPU copy of x rounded to bf16 (the value every bf16 operand of a kernel holds)."""
    return T.as_tensor(x).to(T.bfloat16).double()


# ------------------------------------------------------------------ encoder-level DoRA step, base and medium width
@pytest.mark.parametrize("mode", ["hidden", "last_token"])
@pytest.mark.parametrize("enc_name,dims", [("base_l2", (512, 2, 8, 2048)), ("medium_l2", (1024, 2, 16, 4096))])
def test_dora_step_matches_fp64_autograd(T, gww, enc_name, dims, mode):
    """DoRA (r 8, alpha 32) on q, k, v and out_proj of both layers, through ``last_hidden_state[:, -1]`` (with d_mel)
    and through ``last_token`` (the pooled last layer): every adapter gradient against fp64 autograd, per-tensor
    relative Frobenius error <= 3 % (5 % for the q / k adapters: test_dora_step_128_mels_matches_fp64_autograd)."""
    from gw_whisper_amd.encoder import WhisperConfig, WhisperEncoder
    from gw_whisper_amd.peft import LoraConfig, get_peft_model
    d, L, H, F = dims
    sd = synth.encoder_state_dict(d, L, H, F, seed=3)
    enc = WhisperEncoder.from_numpy_state_dict(sd, WhisperConfig(d, L, H, F), precision="bf16")
    targets = [f"layers.{i}.self_attn.{p}" for i in range(L) for p in ("q_proj", "k_proj", "v_proj", "out_proj")]
    peft = get_peft_model(enc, LoraConfig(use_dora=True, r=8, lora_alpha=32, target_modules=targets)).cuda()
    theta = {}
    with T.no_grad():
        for j, name in enumerate(targets):
            lin = peft.base_model.model.get_submodule(name)
            A, Bm, m = synth.dora_adapter(d, d, 8, sd[name + ".weight"], seed=70 + j)
            lin.lora_A["default"].weight.copy_(T.from_numpy(A))
            lin.lora_B["default"].weight.copy_(T.from_numpy(Bm))
            lin.lora_magnitude_vector["default"].weight.copy_(T.from_numpy(m))
            theta[name] = [T.from_numpy(x).double().requires_grad_(True) for x in (A, Bm, m)]
    mel = olm.log_mel(synth.strain_segments(2, seed=33))
    wl = np.random.default_rng(7).standard_normal((2, d))
    want_mel = mode == "hidden"
    mel_t = T.from_numpy(mel).cuda().requires_grad_(want_mel)
    out = peft(mel_t).last_hidden_state[:, -1, :] if mode == "hidden" else peft.last_token(mel_t)
    (out * T.from_numpy(wl).cuda().float()).sum().backward()

    mel64 = T.from_numpy(mel).double().requires_grad_(want_mel)
    (dora64(T, sd, theta, mel64, (d, L, H), 4.0)[:, -1, :] * T.from_numpy(wl)).sum().backward()
    worst = []
    for name in targets:
        lin = peft.base_model.model.get_submodule(name)
        got = [lin.lora_A["default"].weight.grad, lin.lora_B["default"].weight.grad,
               lin.lora_magnitude_vector["default"].weight.grad]
        for part, g_, r_ in zip("ABm", got, theta[name]):
            g_ = g_.double().cpu()
            assert T.isfinite(g_).all(), (name, part)
            rel = float(T.linalg.norm(g_ - r_.grad) / (T.linalg.norm(r_.grad) + 1e-30))
            worst.append((rel, f"{name}.{part}"))
            assert rel <= (0.05 if ("q_proj" in name or "k_proj" in name) else 0.03), (name, part, rel)
    worst.sort(reverse=True)
    print(enc_name, mode, "worst relative errors:", [(round(r, 4), n) for r, n in worst[:4]])
    assert all(p.grad is None for n, p in peft.named_parameters() if "lora_" not in n)
    if want_mel:
        rel_mel = float(T.linalg.norm(mel_t.grad.double().cpu() - mel64.grad) / T.linalg.norm(mel64.grad))
        print(enc_name, "d_mel relative error", round(rel_mel, 4))
        assert rel_mel <= 0.03


# ------------------------------------------------------------------ LayerNorm backward at every width
def _ln_rows(T, M, d, seed):
    g = T.Generator().manual_seed(seed)
    x = T.randn((M, d), generator=g, dtype=T.float64) * 2 + 0.4
    x[0] = 1e3 + T.randn(d, generator=g, dtype=T.float64)      # |mean| >> std: the mean must not swallow the spread
    if M > 1:
        x[M // 2] = 0.7                                          # a constant row: xhat = 0, dx = rstd (g dy - mean)
    return x.float(), g


@pytest.mark.parametrize("M", [1, 517, 3000])
@pytest.mark.parametrize("d", [128 * k for k in range(1, 11)])
def test_layernorm_backward_every_width(T, gww, d, M):
    """k_ln_bwd<d / 128, ...> for all ten widths: dy fp32 and bf16, plain and accumulating, with and without the bf16
    copy of dx, against the float64 formula on the same fp32 x and (rounded) dy, at the bounds of
    test_layernorm_backward."""
    from gw_whisper_amd import ops
    x, g = _ln_rows(T, M, d, 1000 * d + M)
    gamma = (1 + 0.1 * T.randn(d, generator=g, dtype=T.float64)).float()
    x64 = x.double()
    mu = x64.mean(1, keepdim=True)
    rstd = 1 / T.sqrt(((x64 - mu) ** 2).mean(1, keepdim=True) + 1e-5)
    xh = (x64 - mu) * rstd
    xd, gd = x.cuda(), gamma.cuda()
    for dy_f32 in (True, False):
        dy = T.randn((M, d), generator=g)
        if not dy_f32:
            dy = dy.bfloat16()
        gy = dy.double() * gamma.double()
        ref = rstd * (gy - gy.mean(1, keepdim=True) - xh * (gy * xh).mean(1, keepdim=True))
        dx, dxb = ops.layernorm_bwd(xd, gd, dy.cuda(), want_bf16=True)
        tag = f"dy {'fp32' if dy_f32 else 'bf16'}"
        T.testing.assert_close(dx.cpu().double(), ref, atol=2e-5, rtol=1e-4, msg=lambda m: f"{tag}: {m}")
        T.testing.assert_close(dxb.cpu().double(), ref, atol=1e-5, rtol=2 ** -8, msg=lambda m: f"{tag} bf16 copy: {m}")
        dx_only, none = ops.layernorm_bwd(xd, gd, dy.cuda())
        assert none is None and T.equal(dx_only, dx), tag
        base = T.randn((M, d), generator=g)
        ref2 = base.double() + ref
        for want_bf16 in (False, True):
            acc = base.cuda()
            _, accb = ops.layernorm_bwd(xd, gd, dy.cuda(), dx=acc, want_bf16=want_bf16)
            T.testing.assert_close(acc.cpu().double(), ref2, atol=3e-5, rtol=1e-4, msg=lambda m: f"{tag} accumulate: {m}")
            if want_bf16:
                # the copy is of the accumulated value
                assert T.equal(accb.cpu(), acc.cpu().bfloat16()), tag


# ------------------------------------------------------------------ DoRA gradients as the encoder calls them
def _dora_ref(T, x, dy_st, y_st, W0, bias_st, A, Bm, m, s, ysc):
    """float64 dA, dB of sum(dy_true * y) (norm detached) and dm from the stored (bf16) y the kernel reads:
    dm = sum_rows dy_st (y_st - b_st) / m, with its float64 absolute-value scale."""
    Wp = W0 + s * (Bm @ A)
    n = T.linalg.norm(Wp, dim=1)
    gdy = ysc * dy_st * (m / n)                      # g * dy_true
    dB = s * gdy.t() @ (x @ A.t())
    dA = s * (gdy @ Bm).t() @ x
    dm = (dy_st * (y_st - bias_st)).sum(0) / m
    dm_scale = ((dy_st * y_st).abs().sum(0) + bias_st.abs() * dy_st.abs().sum(0)) / m.abs()
    return dA, dB, dm, dm_scale


@pytest.mark.parametrize("M", [31, 777, 3000])
@pytest.mark.parametrize("d", [128, 384, 512, 768, 1024, 1280])
def test_dora_grads_on_packed_qkv_sections(T, gww, d, M):
    """``gww_dora_grads`` as encoder_train.hip calls it: x = LN1(h) [M, d], dy / y the q / k / v column sections (offsets 0,
    d, 2 d) of packed [M, 3 d] dqkv / qkv with ldy = 3 d, and the q section stored in log2 units (yscale =
    0.125 log2 e).  dA / dB at the bounds of test_dora_parameter_gradients.  dm against the same sums of the stored bf16
    y: products of bf16 values are exact in fp32, so only the fp32 summation over M rows and the atomics remain --
    every element within 1e-5 of its absolute-value sum (measured on MI355X: at most 1e-7).  A second run agrees with the first to fp32 summation noise
    (the kernels add with float atomics)."""
    from gw_whisper_amd import ops
    g = T.Generator().manual_seed(7 * d + M)
    s = 4.0
    x = _bf(T, T.randn((M, d), generator=g, dtype=T.float64))
    dy_all = _bf(T, T.randn((M, 3 * d), generator=g, dtype=T.float64) * 0.3)
    y_all = T.zeros((M, 3 * d), dtype=T.float64)
    secs = []
    for sec in range(3):
        ysc = 0.125 * LOG2E if sec == 0 else 1.0
        W0 = T.randn((d, d), generator=g, dtype=T.float64) / math.sqrt(d)
        A, Bm, m = (T.from_numpy(a).double() for a in synth.dora_adapter(d, d, 8, W0.float().numpy(), seed=4 + sec))
        bias = T.randn(d, generator=g, dtype=T.float64) * 0.1
        Wp = W0 + s * (Bm @ A)
        n = T.linalg.norm(Wp, dim=1)
        y_true = x @ ((m / n)[:, None] * Wp).t() + bias
        y_all[:, sec * d:(sec + 1) * d] = _bf(T, ysc * y_true)
        b_st = (ysc * bias).float()
        secs.append((sec, ysc, W0, A, Bm, m, n.float(), b_st))
    c = lambda t: t.float().cuda()
    xd, dyd, yd = c(x).bfloat16(), c(dy_all).bfloat16(), c(y_all).bfloat16()
    # mfma widths: bf16 weights and bf16 u = x A^T, v = dy (g B) (test_dora_parameter_gradients)
    tol = 5e-3 if d in (384, 512, 768) else 2e-3
    for sec, ysc, W0, A, Bm, m, n, b_st in secs:
        cols = slice(sec * d, (sec + 1) * d)
        dA_ref, dB_ref, dm_ref, dm_scale = _dora_ref(T, x, dy_all[:, cols], y_all[:, cols], W0, b_st.double(), A, Bm,
                                                     m, s, ysc)
        runs = [ops.dora_grads(xd, dyd, yd, c(b_st), ysc, s, c(A), c(Bm), c(m), c(n), col_off=sec * d) for _ in range(2)]
        dA, dB, dm = (t.cpu().double() for t in runs[0])
        T.testing.assert_close(dA, dA_ref, atol=tol * float(dA_ref.abs().max()), rtol=1e-3, msg=lambda e: f"dA {sec}: {e}")
        T.testing.assert_close(dB, dB_ref, atol=tol * float(dB_ref.abs().max()), rtol=1e-3, msg=lambda e: f"dB {sec}: {e}")
        err = (dm - dm_ref).abs()
        print(f"d {d} M {M} section {sec}: dm max error / abs-sum {float((err / dm_scale).max()):.2e}")
        assert (err <= 1e-5 * dm_scale).all(), (sec, float((err / dm_scale).max()))
        for a, b in zip(runs[0], runs[1]):
            assert float((a - b).abs().max()) <= 2e-5 * float(a.abs().max()), sec


# ------------------------------------------------------------------ attention backward
def _attn64(T, qkv, dctx, H, q_log2):
    """float64 ctx, lse [B, H, T] and dqkv of softmax(q k^T) v for bf16-valued qkv [B, T, 3 d] (q in log2 units when
    q_log2: the natural q is q / log2 e and dq is taken with respect to the stored q)."""
    B, Tn, d3 = qkv.shape
    d = d3 // 3
    q, k, v = (qkv[..., i * d:(i + 1) * d].reshape(B, Tn, H, 64).transpose(1, 2) for i in range(3))
    if q_log2:
        q = q / LOG2E
    do = dctx.reshape(B, Tn, H, 64).transpose(1, 2)
    ctx, lse, dq, dk, dv = [], [], [], [], []
    for b in range(B):                                  # one segment at a time: [H, T, T] score tensors
        s = q[b] @ k[b].transpose(-1, -2)
        l_ = T.logsumexp(s, -1, keepdim=True)
        p = T.exp(s - l_)
        o = p @ v[b]
        dp = do[b] @ v[b].transpose(-1, -2)
        ds = p * (dp - (do[b] * o).sum(-1, keepdim=True))
        ctx.append(o), lse.append(l_[..., 0]), dv.append(p.transpose(-1, -2) @ do[b])
        dq.append(ds @ k[b]), dk.append(ds.transpose(-1, -2) @ q[b])
    st = lambda ts: T.stack(ts).transpose(1, 2).reshape(B, Tn, d)
    dqs = st(dq) / (LOG2E if q_log2 else 1.0)
    return st(ctx), T.stack(lse), T.cat([dqs, st(dk), st(dv)], dim=2)


def _check_attention_bwd(T, qkv, dctx, H, q_log2):
    """forward (ctx, lse) and backward of the bf16 kernels against _attn64; the backward error is bounded per
    (segment, head, q / k / v section) by that slice's own largest entry (2e-2 of it at most, 3e-3 rms, the bounds of
    test_attention_backward), so a wrong head with small gradients cannot hide, and a repeated call is bit-identical."""
    from gw_whisper_amd import ops
    B, Tn, d3 = qkv.shape
    d = d3 // 3
    ctx_ref, lse_ref, dqkv_ref = _attn64(T, qkv, dctx, H, q_log2)
    q = qkv.float().cuda().bfloat16()
    if q_log2:
        ctx, lse = ops.attention_log2q(q, H, want_lse=True)
    else:
        ctx, lse = ops.attention_lse(q, H)
    assert T.isfinite(lse).all() and T.isfinite(ctx).all()
    # the bound of test_attention_backward; the natural-unit forward (the kernel-level entry point -- the encoder runs
    # the log2-unit one) measured 3.46e-3 at one row of 24 000 (B 2, T 1500, H 8, lse 14.5), more than the 1.1e-3 that
    # its sum of bf16-rounded P explains: measured bound 4e-3 there, as test_attention_log2q sets one for its lse
    T.testing.assert_close(lse.cpu().double(), lse_ref, atol=2e-3 if q_log2 else 4e-3, rtol=1e-4)
    T.testing.assert_close(ctx.cpu().double(), ctx_ref, atol=6e-3, rtol=2 ** -7)
    dc = dctx.float().cuda().bfloat16()
    dqkv = ops.attention_bwd(q, ctx, dc, lse, H, q_log2=q_log2)
    again = ops.attention_bwd(q, ctx, dc, lse, H, q_log2=q_log2)
    assert T.equal(dqkv, again), "the attention backward uses no atomics: a repeated call must be bit-identical"
    got = dqkv.cpu().double().reshape(B, Tn, 3, H, 64)
    ref = dqkv_ref.reshape(B, Tn, 3, H, 64)
    assert T.isfinite(got).all()
    err = (got - ref).abs()
    # [B, 3, H]; floored at 1e-3 of the section's largest entry: with one key (T = 1) dS and so dq, dk vanish
    scale = T.maximum(ref.abs().amax(dim=(1, 4)), 1e-3 * ref.abs().amax(dim=(0, 1, 3, 4))[None, :, None])
    max_err = err.amax(dim=(1, 4))
    rms_err = err.pow(2).mean(dim=(1, 4)).sqrt()
    worst = float((max_err / scale).max())
    bad = (max_err > 2e-2 * scale) | (rms_err > 3e-3 * scale)
    assert not bad.any(), [(b, "qkv"[sec], h, float(max_err[b, sec, h] / scale[b, sec, h]))
                           for b, sec, h in bad.nonzero().tolist()][:8]
    return worst


@pytest.mark.parametrize("q_log2", [False, True], ids=["natural_q", "log2_q"])
@pytest.mark.parametrize("B,Tn,H", [(2, 1500, 6), (2, 1500, 8), (2, 1500, 12), (2, 1500, 16), (2, 1500, 20),
                                    # ceil(T / 128) B H = 18, 9, 108, 45 blocks: the XCD reorder's tail branch
                                    (3, 129, 3), (1, 37, 9), (3, 1500, 3), (5, 333, 3),
                                    (1, 1, 2)])
def test_attention_backward_every_head_count(T, gww, B, Tn, H, q_log2):
    """The encoders' head counts (6, 8, 12, 16, 20 at T = 1500), grids whose block count is >= 8 and not a multiple
    of 8 (the blocks past 8 * (n / 8) keep their own index) and a single key (T = 1)."""
    g = T.Generator().manual_seed(B * 10000 + Tn * 10 + H)
    qkv = _bf(T, T.randn((B, Tn, 3 * H * 64), generator=g, dtype=T.float64) * 0.6)
    if q_log2:
        qkv[..., :H * 64] = _bf(T, qkv[..., :H * 64] * LOG2E)
    dctx = _bf(T, T.randn((B, Tn, H * 64), generator=g, dtype=T.float64) * 0.5)
    worst = _check_attention_bwd(T, qkv, dctx, H, q_log2)
    print(f"B {B} T {Tn} H {H} {'log2' if q_log2 else 'natural'} q: worst slice max error / slice max {worst:.2e}")


@pytest.mark.parametrize("q_log2", [False, True], ids=["natural_q", "log2_q"])
@pytest.mark.parametrize("case", ["offset-100", "offset-12", "offset+12", "offset+100", "spike"])
def test_attention_backward_score_offsets_and_spikes(T, gww, case, q_log2):
    """The forward tests' constructions (test_gpu_kernels.py) on head 0 of a 2 x 300 x 3 grid (18 blocks): every score
    of head 0 moved by +-12 / +-100, or a key far above the rest for one query (score 256) and a query whose scores
    are all very negative against it.  The backward re-forms P from the forward's lse: it must hold there too.
    The offset is carried by q (q[:, 0] = offset, k[:, 0] = 1: the same scores as the forward tests' k[:, 0] = offset).
    With the offset on the key side, dq's column 0 is offset * sum_j dS_ij, zero in exact arithmetic, and the bf16
    rounding of dS alone leaves up to 0.66 (+-100) / 0.08 (+-12) of that head's largest dq entry there (measured on
    MI355X) -- a property of any bf16 dS operand, not a kernel slip; dk and dv met the bounds in that form too."""
    g = T.Generator().manual_seed(11)
    B, Tn, H = 2, 300, 3
    d = H * 64
    qkv = T.randn((B, Tn, 3 * d), generator=g, dtype=T.float64) * 0.4
    if case == "spike":
        qkv[:, 17, :64] = 2.0
        qkv[:, 250, d:d + 64] = 2.0                       # key 250 of every segment: score 256 against query 17
        qkv[:, 100, :64] = -3.0
    else:
        qkv[:, :, 0] = float(case[len("offset"):])        # q[:, 0] = offset in head 0 ...
        qkv[:, :, d] = 1.0                                # ... and k[:, 0] = 1: every score of head 0 moves
    qkv = _bf(T, qkv)
    if q_log2:
        qkv[..., :d] = _bf(T, qkv[..., :d] * LOG2E)
    dctx = _bf(T, T.randn((B, Tn, d), generator=g, dtype=T.float64) * 0.5)
    worst = _check_attention_bwd(T, qkv, dctx, H, q_log2)
    print(f"{case} {'log2' if q_log2 else 'natural'} q: worst slice max error / slice max {worst:.2e}")


# ------------------------------------------------------------------ GELU-backward epilogue of the A-stationary GEMM
@pytest.mark.parametrize("inplace", [False, True], ids=["separate", "in_place"])
@pytest.mark.parametrize("M,N,K", [(M, N, 384) for M in (1, 777, 3000, 4500) for N in (128, 1536)]
                         + [(777, 1536, 256), (3000, 128, 256), (777, 1536, 512), (3000, 128, 512)])
def test_gemm_astat_gelu_backward_epilogue(T, gww, M, N, K, inplace):
    """EPI_DGELU, what every tiny training step runs for fc1's GELU: C = g * gelu'(a W^T + b) against float64 on the
    same bf16 a, W, g.  K = 384 is the form with the incoming-gradient loads issued early by inline asm; K = 256 / 512
    load it next to its use.  In place, C is the incoming gradient itself, padded to whole 256-row panels as in the
    encoder: rows below M must match, the padded rows may hold anything.  Two bf16 roundings (gelu' and the product):
    rtol 2^-7, plus 2e-5 |g| for the fp32 accumulation of z and the polynomial erf."""
    from gw_whisper_amd import _lib, ops
    g_ = T.Generator().manual_seed(M + N + K)
    a = _bf(T, T.randn((M, K), generator=g_, dtype=T.float64))
    w = _bf(T, T.randn((N, K), generator=g_, dtype=T.float64) * (1.5 / math.sqrt(K)))
    bias = (T.randn(N, generator=g_, dtype=T.float64) * 0.3).float()
    Mp = (M + 255) // 256 * 256
    gpad = _bf(T, T.randn((Mp, N), generator=g_, dtype=T.float64))
    gg = gpad[:M]
    z = a @ w.t() + bias.double()
    ref = gg * (0.5 * (1 + T.erf(z / math.sqrt(2))) + z * T.exp(-0.5 * z * z) / math.sqrt(2 * math.pi))
    ad, wd, bd = a.float().cuda().bfloat16(), w.float().cuda().bfloat16(), bias.cuda()
    if inplace:
        buf = gpad.float().cuda().bfloat16()
        out = ops.gemm_astat(ad, wd, bd, epilogue=_lib.EPI_DGELU, delta=buf, out=buf)
        assert out.data_ptr() == buf.data_ptr()
    else:
        gd = gg.float().cuda().bfloat16()
        keep = gd.clone()
        out = ops.gemm_astat(ad, wd, bd, epilogue=_lib.EPI_DGELU, delta=gd)
        assert T.equal(gd, keep), "the incoming gradient must not be written"
    got = out[:M].cpu().double()
    assert got.shape == (M, N) and T.isfinite(got).all()
    err = (got - ref).abs()
    bound = 2 ** -7 * ref.abs() + 2e-5 * gg.abs() + 1e-30
    assert (err <= bound).all(), (float((err / bound).max()), divmod(int((err / bound).argmax()), N))
