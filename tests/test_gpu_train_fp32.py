"""The exact-fp32 DoRA / LoRA training step (``WhisperEncoder(..., precision="fp32")``): the step against fp64 autograd
at every width and rank, its three kernels (attention forward with lse and backward, adapter gradients) against fp64,
determinism, ``.grad`` accumulation and the post-step re-pack, the bf16 step measured against it at full depth, the
harness flag and the refusals that stay.  Needs an MI355X."""

import json
import os
import subprocess
import sys

import numpy as np
import pytest

from gw_whisper_amd import synth
from oracle import logmel as olm
from tests.helpers import encoder64

pytestmark = pytest.mark.gpu

ALL = ("self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj", "self_attn.out_proj", "fc1", "fc2")
# relative Frobenius error of every adapter gradient and of d_mel against fp64 (the bf16 step: 3 - 8 %).  The issue's
# 2e-4 tightened to 1e-4: measured on MI355X, the worst tensor of every case below is 2.5e-5 (base_l2, r 1, LoRA, q_proj
# B), the worst d_mel 1.7e-6 (whisper-large at two layers)
BOUND = 1e-4


@pytest.fixture(scope="module")
def T():
    import torch
    assert torch.cuda.is_available()
    return torch


def _adapted64(T, sd, theta, mel, cfg, scaling, use_dora):
    """fp64 encoder with merged adapters: DoRA (peft: the weight norm enters detached) or plain LoRA W0 + s B A."""
    p = {k: T.from_numpy(v).double() for k, v in sd.items()}
    for name, (A, Bm, m) in theta.items():
        Wp = p[name + ".weight"] + scaling * (Bm @ A)
        p[name + ".weight"] = (m / T.linalg.norm(Wp, dim=1).detach())[:, None] * Wp if use_dora else Wp
    return encoder64(T, p, mel, cfg)


def _mel(n_mels, n_seg=2, seed=33):
    if n_mels == 80:
        return olm.log_mel(synth.strain_segments(n_seg, seed=seed))
    return (np.random.default_rng(seed).standard_normal((n_seg, n_mels, 3000)) * 0.5).astype(np.float32)


def _build(T, sd, dims, n_mels, precision, r, use_dora, targets, seed0=70):
    """peft model over a ``precision`` encoder with adapters on ``targets``, filled with the seeded trained values."""
    from gw_whisper_amd.encoder import WhisperConfig, WhisperEncoder
    from gw_whisper_amd.peft import LoraConfig, get_peft_model
    d, L, H, F = dims
    enc = WhisperEncoder.from_numpy_state_dict(sd, WhisperConfig(d, L, H, F, num_mel_bins=n_mels), precision=precision)
    peft = get_peft_model(enc, LoraConfig(use_dora=use_dora, r=r, lora_alpha=32, target_modules=targets)).cuda()
    theta = {}
    with T.no_grad():
        for j, name in enumerate(targets):
            lin = peft.base_model.model.get_submodule(name)
            W0 = sd[name + ".weight"]
            A, Bm, m = synth.dora_adapter(W0.shape[0], W0.shape[1], r, W0, seed=seed0 + j)
            lin.lora_A["default"].weight.copy_(T.from_numpy(A))
            lin.lora_B["default"].weight.copy_(T.from_numpy(Bm))
            if use_dora:
                lin.lora_magnitude_vector["default"].weight.copy_(T.from_numpy(m))
            theta[name] = [T.from_numpy(x).double().requires_grad_(True) for x in (A, Bm, m)]
    return peft, theta


def _grads(peft, targets, use_dora):
    out = {}
    for name in targets:
        lin = peft.base_model.model.get_submodule(name)
        parts = [("A", lin.lora_A["default"].weight), ("B", lin.lora_B["default"].weight)]
        if use_dora:
            parts.append(("m", lin.lora_magnitude_vector["default"].weight))
        for part, p in parts:
            out[f"{name}.{part}"] = p.grad
    return out


def _step_vs_fp64(T, dims, r, use_dora, mode, n_mels=80, seed=3, sd=None):
    """fp32 step, adapters on all six projections of every layer, one backward through ``last_hidden_state[:, -1]``
    (with d_mel) or ``last_token``; every adapter gradient against fp64 autograd.  Returns the worst relative error.
    ``sd``: the base weights (default: the seeded Gaussian ones)."""
    d, L, H, F = dims
    if sd is None:
        sd = synth.encoder_state_dict(d, L, H, F, seed=seed, n_mels=n_mels)
    targets = [f"layers.{i}.{p}" for i in range(L) for p in ALL]
    peft, theta = _build(T, sd, dims, n_mels, "fp32", r, use_dora, targets)
    mel = _mel(n_mels)
    wl = np.random.default_rng(7).standard_normal((2, d))
    want_mel = mode == "hidden"
    mel_t = T.from_numpy(mel).cuda().requires_grad_(want_mel)
    out = peft(mel_t).last_hidden_state[:, -1, :] if mode == "hidden" else peft.last_token(mel_t)
    (out * T.from_numpy(wl).cuda().float()).sum().backward()

    mel64 = T.from_numpy(mel).double().requires_grad_(want_mel)
    (_adapted64(T, sd, theta, mel64, (d, L, H), 32 / r, use_dora)[:, -1, :] * T.from_numpy(wl)).sum().backward()
    got = _grads(peft, targets, use_dora)
    worst = []
    for name in targets:
        for part, r_ in zip("ABm", theta[name]):
            if part == "m" and not use_dora:
                continue
            g_ = got[f"{name}.{part}"]
            assert g_ is not None, (name, part)
            g_ = g_.double().cpu()
            assert T.isfinite(g_).all(), (name, part)
            rel = float(T.linalg.norm(g_ - r_.grad) / (T.linalg.norm(r_.grad) + 1e-30))
            worst.append((rel, f"{name}.{part}"))
    worst.sort(reverse=True)
    rel_mel = None
    if want_mel:
        rel_mel = float(T.linalg.norm(mel_t.grad.double().cpu() - mel64.grad) / T.linalg.norm(mel64.grad))
    print(dims, n_mels, r, "dora" if use_dora else "lora", mode, "worst:", [(f"{x:.2e}", n) for x, n in worst[:3]],
          "d_mel:", rel_mel)
    assert all(p.grad is None for n, p in peft.named_parameters() if "lora_" not in n)
    assert worst[0][0] <= BOUND, worst[:3]
    if want_mel:
        assert rel_mel <= BOUND, rel_mel
    return worst[0][0]


ENCODERS = {"micro": (synth.ENCODER_SIZES["micro"], 80), "tiny": (synth.ENCODER_SIZES["tiny"], 80),
            "base_l2": ((512, 2, 8, 2048), 80), "large_l2": ((1280, 2, 20, 5120), 80),
            "large_v3_l2": ((1280, 2, 20, 5120), 128)}


@pytest.mark.parametrize("mode", ["hidden", "last_token"])
@pytest.mark.parametrize("enc_name", list(ENCODERS))
def test_fp32_step_matches_fp64(T, gww, enc_name, mode):
    """DoRA r 8 on all six projections of every layer; tiny runs the per-op path in fp32 (the fused d = 384 kernels are
    bf16-only).  Fails on a tree without the fp32 step: the first forward raised GwwError."""
    dims, n_mels = ENCODERS[enc_name]
    _step_vs_fp64(T, dims, 8, True, mode, n_mels=n_mels)


@pytest.mark.parametrize("use_dora", [True, False])
@pytest.mark.parametrize("r", [1, 4, 16, 64])
@pytest.mark.parametrize("enc_name", ["micro", "base_l2"])
def test_fp32_rank_sweep_matches_fp64(T, gww, enc_name, r, use_dora):
    """In fp32, r = 1 gets no looser bound."""
    dims, n_mels = ENCODERS[enc_name]
    _step_vs_fp64(T, dims, r, use_dora, "last_token" if r % 2 else "hidden", n_mels=n_mels)


@pytest.mark.parametrize("mode", ["hidden", "last_token"])
@pytest.mark.parametrize("dims", [(128, 2, 2, 512), (384, 2, 6, 1536), (512, 2, 8, 2048)], ids=lambda d: f"d{d[0]}")
def test_fp32_step_matches_fp64_on_whisper_like_weights(T, gww, dims, mode):
    """The same step on weights with a pretrained encoder's statistics (tests/whisper_like.py: residual-stream channels in
    the hundreds, LayerNorm gains 0.02 .. 4, fc1 pre-activations at +-30, sharpened attention) under the same bound: the
    LayerNorm backward's cancellation on outlier rows and the GELU derivative's tails are not reached by Gaussian weights.
    Measured on MI355X: worst tensor 8.7e-5 (d = 128), 4.0e-5 (d = 384), 2.8e-5 (d = 512), all k_proj of the last layer.
    (Before k_attn_bwd_dq_f32 accumulated dQ against the mean-centred keys, q_proj.A of the last layer measured 1.6e-4 at
    d = 128: the keys of a head share a component 4.8 times their spread there.)"""
    from tests.whisper_like import whisper_like_state_dict
    _step_vs_fp64(T, dims, 8, True, mode, sd=whisper_like_state_dict(*dims, seed=3))


# ------------------------------------------------------------------ attention kernels
def _attn64(T, qkv, dctx, H):
    """float64 softmax(q k^T) v with q as stored, its lse and the autograd dqkv."""
    B, Tn, d3 = qkv.shape
    d = d3 // 3
    x = qkv.double().clone().requires_grad_(True)
    sh = lambda t: t.reshape(B, Tn, H, 64).transpose(1, 2)
    q, k, v = sh(x[..., :d]), sh(x[..., d:2 * d]), sh(x[..., 2 * d:])
    s = q @ k.transpose(-1, -2)
    lse = T.logsumexp(s, dim=-1)
    ctx = (T.softmax(s, dim=-1) @ v).transpose(1, 2).reshape(B, Tn, d)
    (ctx * dctx.double()).sum().backward()
    return ctx.detach(), lse.detach(), x.grad


@pytest.mark.parametrize("dmode", ["dense", "pooled"])
@pytest.mark.parametrize("case", ["plain", "offset+12", "offset-100", "spike"])
@pytest.mark.parametrize("B,Tn,H", [(2, 1500, 6), (1, 77, 2), (3, 1, 16), (1, 1500, 20), (2, 77, 20), (1, 300, 2)])
def test_attention_fp32_kernels_vs_fp64(T, gww, B, Tn, H, case, dmode):
    """lse against fp64 logsumexp; ctx bit-identical to gww_attention_f32; dq / dk / dv within 1e-5 of the largest
    |reference| of their section; the pooled dctx (zero except at row T - 1) skips the dead query tiles; repeated calls
    give identical bits.  Two allowances, both properties of fp32 inputs rather than of the kernels (measured on MI355X):
      * offset -100: a score near -100 is itself rounded to ulp(100) = 7.6e-6 in fp32 before any product is formed, so P
        carries that relative error; dq / dk / dv then measure up to 2.1e-5 of their section maximum (bound 4e-5), ctx
        up to 1.5e-5 absolute (bound 4e-5).  Offsets of 12 stay within 2.8e-6.
      * T = 1: dS = P (dP - D) is zero in exact arithmetic, and dq, dk are the rounding noise of dP - D, two 64-term dot
        products in different orders: bounded by 64 eps |dO| |V| max(|q|, |k|) (measured 2.4e-5 at |q| = 12)."""
    from gw_whisper_amd import ops
    g = T.Generator().manual_seed(B * 1000 + Tn + H)
    d = H * 64
    qkv = T.randn((B, Tn, 3 * d), generator=g, dtype=T.float64) * 0.4
    if case == "spike" and Tn > 250:
        qkv[:, 17, :64] = 2.0
        qkv[:, 250, d:d + 64] = 2.0                       # key 250: score 256 against query 17
        qkv[:, 100, :64] = -3.0
    elif case.startswith("offset"):
        qkv[:, :, 0] = float(case[len("offset"):])        # every score of head 0 moved by the offset
        qkv[:, :, d] = 1.0
    qkv = qkv.float().double()
    dctx = (T.randn((B, Tn, d), generator=g, dtype=T.float64) * 0.5).float().double()
    if dmode == "pooled":
        dctx[:, :-1] = 0.0
    ctx_ref, lse_ref, dqkv_ref = _attn64(T, qkv, dctx, H)
    q = qkv.float().cuda()
    ctx, lse = ops.attention_lse_f32(q, H)
    assert T.equal(ctx, ops.attention(q, H)), "ctx of the lse entry must be bit-identical to gww_attention_f32"
    big = case == "offset-100"
    T.testing.assert_close(lse.cpu().double(), lse_ref, atol=2e-6, rtol=2e-6)
    T.testing.assert_close(ctx.cpu().double(), ctx_ref, atol=4e-5 if big else 1e-5, rtol=1e-5)
    dc = dctx.float().cuda()
    dqkv = ops.attention_bwd_f32(q, ctx, dc, lse, H)
    assert T.equal(dqkv, ops.attention_bwd_f32(q, ctx, dc, lse, H)), "no atomics: repeated calls are bit-identical"
    got = dqkv.cpu().double().reshape(B, Tn, 3, H, 64)
    ref = dqkv_ref.reshape(B, Tn, 3, H, 64)
    assert T.isfinite(got).all()
    worst = 0.0
    qk = float(qkv[..., :2 * d].abs().max())
    noise = 64 * 2.0 ** -24 * float(dctx.abs().max()) * float(qkv[..., 2 * d:].abs().max()) * qk if Tn == 1 else 0.0
    for sec in range(3):
        scale = float(ref[:, :, sec].abs().max())
        err = float((got[:, :, sec] - ref[:, :, sec]).abs().max())
        worst = max(worst, err / max(scale, 1e-30))
        assert err <= (4e-5 if big else 1e-5) * scale + noise + 1e-12, ("qkv"[sec], err, scale)
    print(f"B={B} T={Tn} H={H} {case} {dmode}: worst |err| / max|ref| = {worst:.2e}")


# ------------------------------------------------------------------ adapter-gradient kernel
def _ref_adapter(T, x, dy, y, A, Bm, m, n, b, s, ysc):
    """float64 on the fp32 operands the kernel sees (n: the fp32 row norms it is given)."""
    x, dy, y = x.double(), dy.double(), y.double()
    g = ysc * (m / n)
    u = x @ A.T
    v = (dy * g) @ Bm
    return s * v.T @ x, s * (dy * g).T @ u, ((dy * (y - b)).sum(0)) / m


@pytest.mark.parametrize("d", [384, 1280])
@pytest.mark.parametrize("kind", ["square", "fc1", "fc2"])
def test_adapter_grads_f32_vs_fp64(T, gww, d, kind):
    from gw_whisper_amd import ops
    d_in, d_out = {"square": (d, d), "fc1": (d, 4 * d), "fc2": (4 * d, d)}[kind]
    worst = 0.0
    for i, (M, r) in enumerate([(M, r) for M in (1, 31, 777, 3000) for r in (1, 8, 16, 64)]):
        g = T.Generator().manual_seed(1000 * d + i)
        pad = 4 * (i % 3)
        x = T.randn((M, d_in + pad), generator=g).float()
        dy = (T.randn((M, d_out + pad), generator=g) * 0.1).float()
        y = T.randn((M, d_out + pad), generator=g).float()
        W0 = T.randn((d_out, d_in), generator=g, dtype=T.float64) / d_in ** 0.5
        A = ((T.rand((r, d_in), generator=g, dtype=T.float64) - 0.5) * 2 / d_in ** 0.5).float().double()
        Bm = (T.randn((d_out, r), generator=g, dtype=T.float64) * 0.05).float().double()
        m = (T.linalg.norm(W0, dim=1) * (1 + 0.1 * T.randn(d_out, generator=g, dtype=T.float64))).float().double()
        b = (T.randn(d_out, generator=g, dtype=T.float64) * 0.1).float().double()
        ysc = 0.125 if i % 5 == 0 else 1.0
        s = 32.0 / r
        xc, dyc, yc = x.cuda()[:, :d_in], dy.cuda()[:, :d_out], y.cuda()[:, :d_out]
        n = T.linalg.norm(W0 + s * (Bm @ A), dim=1).float().double()
        f = lambda t: t.float().cuda()
        got = ops.adapter_grads_f32(xc, dyc, yc, f(b), ysc, s, f(A), f(Bm), f(m), f(n))
        refs = _ref_adapter(T, x[:, :d_in], dy[:, :d_out], y[:, :d_out], A, Bm, m, n, b, s, ysc)
        # M = 1: dA / dB are outer products of one row with u = x A^T / v = (g dy) B, r single dot products whose
        # cancellation (not the kernel) sets their relative error: there, measure against the same products of |.|
        # (fc1, d 384, r 1: 6.2e-5 of the signed result, measured on MI355X)
        if M == 1:
            ab = _ref_adapter(T, x[:, :d_in].abs(), dy[:, :d_out].abs(), y[:, :d_out], A.abs(), Bm.abs(), m, n, b, s, ysc)
            den = [T.linalg.norm(ab[0]), T.linalg.norm(ab[1]), T.linalg.norm(refs[2])]
        else:
            den = [T.linalg.norm(t) for t in refs]
        for name, g_, r_, dn in zip(("dA", "dB", "dm"), got, refs, den):
            rel = float(T.linalg.norm(g_.double().cpu() - r_) / (dn + 1e-30))
            worst = max(worst, rel)
            assert rel <= 1e-5, (kind, d, M, r, name, rel)
        if i % 4 == 0:
            again = ops.adapter_grads_f32(xc, dyc, yc, f(b), ysc, s, f(A), f(Bm), f(m), f(n))
            assert all(T.equal(a, b_) for a, b_ in zip(got, again)), (kind, d, M, r)
    print(f"adapter_grads_f32 {kind} d={d}: worst relative error {worst:.2e}")


# ------------------------------------------------------------------ determinism, accumulation, optimizer step
def test_fp32_step_determinism_accumulation_and_repack(T, gww):
    dims = synth.ENCODER_SIZES["micro"]
    d, L, H, F = dims
    sd = synth.encoder_state_dict(d, L, H, F, seed=5)
    targets = [f"layers.{i}.{p}" for i in range(L) for p in ALL]
    mel = T.from_numpy(_mel(80, 3, seed=9)).cuda()

    def step(peft):
        peft.last_token(mel).square().sum().backward()
        return {k: v.detach().clone() for k, v in _grads(peft, targets, True).items()}

    peft, _ = _build(T, sd, dims, 80, "fp32", 8, True, targets)
    one = step(peft)
    peft.zero_grad(set_to_none=True)
    assert all(T.equal(one[k], v) for k, v in step(peft).items()), "two identical steps give identical bits"
    two = step(peft)   # .grad exists: the backward accumulates into it
    assert all(T.equal(two[k], 2 * one[k]) for k in one)
    params = [p for n, p in peft.named_parameters() if "lora_" in n]
    opt = T.optim.AdamW(params, lr=1e-3)
    opt.step()
    with T.no_grad():
        after = peft.last_token(mel)
        fresh, _ = _build(T, sd, dims, 80, "fp32", 8, True, targets)
        fresh.load_state_dict(peft.state_dict())
        ref = fresh.last_token(mel)
        before_fresh, _ = _build(T, sd, dims, 80, "fp32", 8, True, targets)
        old = before_fresh.last_token(mel)
    assert T.equal(after, ref), "the next fp32 forward sees the stepped adapters"
    assert not T.equal(after, old)
    # ... and so does the next fp32 TRAINING forward (gww_encoder_train_forward_f32, autograd on), which reads the
    # same re-packed panels: equal to a fresh encoder's training forward on the stepped values
    train_after = peft.last_token(mel)
    train_ref = fresh.last_token(mel)
    train_old = before_fresh.last_token(mel)
    assert train_after.requires_grad and train_ref.requires_grad
    assert T.equal(train_after.detach(), train_ref.detach()), "the next fp32 training forward sees the stepped adapters"
    assert not T.equal(train_after.detach(), train_old.detach())


# ------------------------------------------------------------------ bf16 against fp32 at full depth
def _bf16_vs_fp32(T, name, n_seg=4):
    d, L, H, F = synth.ENCODER_SIZES[name]
    sd = synth.encoder_state_dict(d, L, H, F, seed=11)
    targets = [f"layers.{i}.{p}" for i in range(L) for p in ALL]
    mel = T.from_numpy(_mel(80, n_seg, seed=21)).cuda()
    wl = T.from_numpy(np.random.default_rng(3).standard_normal((n_seg, d))).cuda().float()
    got = {}
    for prec in ("bf16", "fp32"):
        peft, _ = _build(T, sd, (d, L, H, F), 80, prec, 8, True, targets)
        (peft.last_token(mel) * wl).sum().backward()
        got[prec] = {k: v.double().cpu() for k, v in _grads(peft, targets, True).items()}
        del peft
    rel = {k: float(T.linalg.norm(got["bf16"][k] - got["fp32"][k]) / (T.linalg.norm(got["fp32"][k]) + 1e-30))
           for k in got["fp32"]}
    return rel


def _report(rel):
    worst = sorted(((v, k) for k, v in rel.items()), reverse=True)
    for v, k in worst[:8]:
        print(f"  {k}: {v:.4f}")
    return worst


def test_bf16_step_against_fp32_whisper_tiny(T, gww):
    """Full whisper-tiny, 4 segments, all-linear DoRA r 8: the bf16 step's gradients lie within the bf16 bounds (3 %,
    5 % for q / k) of the fp32 step's."""
    rel = _bf16_vs_fp32(T, "tiny")
    _report(rel)
    for k, v in rel.items():
        assert v <= (0.05 if ("q_proj" in k or "k_proj" in k) else 0.03), (k, v)


def test_bf16_step_against_fp32_whisper_small(T, gww):
    """whisper-small (12 layers), 4 segments, all-linear DoRA r 8: the bf16 error at this depth, per tensor.  Measured on
    MI355X: worst 15.8 % (layers.7 q_proj A), then 13.1 % (layers.10 k_proj A), every tensor other than q / k below
    11 %; bound 25 %, a 1.6x margin (DESIGN.md "Training in fp32")."""
    rel = _bf16_vs_fp32(T, "small")
    worst = _report(rel)
    assert all(np.isfinite(v) for v in rel.values())
    assert worst[0][0] <= SMALL_BOUND, worst[:4]


SMALL_BOUND = 0.25


# ------------------------------------------------------------------ harness and refusals
def test_run_train_precision_fp32(T, gww, tmp_path):
    from gw_whisper_amd.encoder import WhisperConfig, WhisperEncoder
    from gw_whisper_amd.peft import PeftModel
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = str(tmp_path)
    r = subprocess.run([sys.executable, os.path.join(root, "harness", "run_train.py"), "--precision", "fp32",
                        "--synthetic", "64", "--encoder", "micro", "--batch-size", "16", "--num-epochs", "1",
                        "--models-path", out + "/m", "--log-dir", out + "/l"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    recs = [json.loads(l) for l in open(out + "/l/train_log.jsonl")]
    assert recs and all(np.isfinite(x["train_loss"]) for x in recs)
    enc = WhisperEncoder(WhisperConfig.named("micro"), precision="fp32")
    peft = PeftModel.from_pretrained(enc, out + "/m/lora_weights_8_32", is_trainable=True).cuda()
    assert any("lora_" in n for n, _ in peft.named_parameters())


def test_full_finetune_stays_bf16_only(T, gww):
    from gw_whisper_amd._lib import GwwError
    from gw_whisper_amd.encoder import WhisperConfig, WhisperEncoder
    with pytest.raises(GwwError):
        WhisperEncoder(WhisperConfig.named("micro"), precision="fp32").enable_full_finetune()
