"""Adapters on every encoder linear layer and at every rank 1..64: the fc1 / fc2 adapter gradients of the three backward
paths (per-op, fused whisper-tiny, pooled last layer) and ranks other than 8 on the attention projections, against fp64
autograd; the adapter-gradient kernel (``ops.adapter_grads``) against fp64 at the [d, d], [4d, d] and [d, 4d] shapes;
MLP-only adapters; the training harness with ``--lora-rank`` / ``--lora-targets``.  Needs an MI355X."""

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


def _step_vs_fp64(T, dims, r, use_dora, mode, seed=3):
    """Adapters on all six projections of every layer; one backward through ``last_hidden_state[:, -1]`` (with d_mel)
    or ``last_token``; every adapter gradient against fp64 autograd (relative Frobenius error)."""
    from gw_whisper_amd.encoder import WhisperConfig, WhisperEncoder
    from gw_whisper_amd.peft import LoraConfig, get_peft_model
    d, L, H, F = dims
    alpha = 32
    sd = synth.encoder_state_dict(d, L, H, F, seed=seed)
    enc = WhisperEncoder.from_numpy_state_dict(sd, WhisperConfig(d, L, H, F), precision="bf16")
    targets = [f"layers.{i}.{p}" for i in range(L) for p in ALL]
    peft = get_peft_model(enc, LoraConfig(use_dora=use_dora, r=r, lora_alpha=alpha, target_modules=targets)).cuda()
    theta = {}
    with T.no_grad():
        for j, name in enumerate(targets):
            lin = peft.base_model.model.get_submodule(name)
            W0 = sd[name + ".weight"]
            A, Bm, m = synth.dora_adapter(W0.shape[0], W0.shape[1], r, W0, seed=70 + j)
            lin.lora_A["default"].weight.copy_(T.from_numpy(A))
            lin.lora_B["default"].weight.copy_(T.from_numpy(Bm))
            if use_dora:
                lin.lora_magnitude_vector["default"].weight.copy_(T.from_numpy(m))
            theta[name] = [T.from_numpy(x).double().requires_grad_(True) for x in (A, Bm, m)]
    mel = olm.log_mel(synth.strain_segments(2, seed=33))
    wl = np.random.default_rng(7).standard_normal((2, d))
    want_mel = mode == "hidden"
    mel_t = T.from_numpy(mel).cuda().requires_grad_(want_mel)
    out = peft(mel_t).last_hidden_state[:, -1, :] if mode == "hidden" else peft.last_token(mel_t)
    (out * T.from_numpy(wl).cuda().float()).sum().backward()

    mel64 = T.from_numpy(mel).double().requires_grad_(want_mel)
    (_adapted64(T, sd, theta, mel64, (d, L, H), alpha / r, use_dora)[:, -1, :] * T.from_numpy(wl)).sum().backward()
    worst = []
    for name in targets:
        lin = peft.base_model.model.get_submodule(name)
        got = [lin.lora_A["default"].weight.grad, lin.lora_B["default"].weight.grad]
        if use_dora:
            got.append(lin.lora_magnitude_vector["default"].weight.grad)
        for part, g_, r_ in zip("ABm", got, theta[name]):
            assert g_ is not None, (name, part)
            g_ = g_.double().cpu()
            assert T.isfinite(g_).all(), (name, part)
            rel = float(T.linalg.norm(g_ - r_.grad) / (T.linalg.norm(r_.grad) + 1e-30))
            worst.append((rel, f"{name}.{part}"))
            bound = 0.05 if ("q_proj" in name or "k_proj" in name) else 0.03
            # r = 1: one rank direction, nothing averages the bf16 rounding of the upstream gradient (measured up to
            # 5.7 % on fc2 / q_proj A); the kernel itself is held to 2 % on its own operands below
            assert rel <= (0.08 if r == 1 else bound), (name, part, rel)
    worst.sort(reverse=True)
    print(dims, r, "dora" if use_dora else "lora", mode, "worst:", [(round(x, 4), n) for x, n in worst[:3]])
    assert all(p.grad is None for n, p in peft.named_parameters() if "lora_" not in n)
    if want_mel:
        rel_mel = float(T.linalg.norm(mel_t.grad.double().cpu() - mel64.grad) / T.linalg.norm(mel64.grad))
        assert rel_mel <= 0.03, rel_mel


ENCODERS = {"micro": synth.ENCODER_SIZES["micro"], "tiny": synth.ENCODER_SIZES["tiny"], "base_l2": (512, 2, 8, 2048),
            "small_l2": (768, 2, 12, 3072), "medium_l2": (1024, 2, 16, 4096), "large_l2": (1280, 2, 20, 5120)}


@pytest.mark.parametrize("mode", ["hidden", "last_token"])
@pytest.mark.parametrize("enc_name", list(ENCODERS))
def test_all_linear_dora_step_matches_fp64(T, gww, enc_name, mode):
    """DoRA r 8 on q, k, v, out_proj, fc1 and fc2 of every layer: tiny runs the fused path, the others the per-op
    one; last_token runs the pooled last layer."""
    _step_vs_fp64(T, ENCODERS[enc_name], 8, True, mode)


@pytest.mark.parametrize("use_dora", [True, False])
@pytest.mark.parametrize("r", [1, 4, 12, 16, 32, 64])
@pytest.mark.parametrize("enc_name", ["micro", "base_l2"])
def test_rank_sweep_matches_fp64(T, gww, enc_name, r, use_dora):
    _step_vs_fp64(T, ENCODERS[enc_name], r, use_dora, "last_token" if r % 2 else "hidden")


# ------------------------------------------------------------------ the kernel
def _kernel_case(T, M, d_in, d_out, r, seed, stride_pad=0, ysc=1.0):
    g = T.Generator().manual_seed(seed)
    x = (T.randn((M, d_in + stride_pad), generator=g)).bfloat16()
    dy = (T.randn((M, d_out + stride_pad), generator=g) * 0.1).bfloat16()
    y = (T.randn((M, d_out + stride_pad), generator=g)).bfloat16()
    W0 = T.randn((d_out, d_in), generator=g, dtype=T.float64) / d_in ** 0.5
    A = (T.rand((r, d_in), generator=g, dtype=T.float64) - 0.5) * 2 / d_in ** 0.5
    Bm = T.randn((d_out, r), generator=g, dtype=T.float64) * 0.05
    m = T.linalg.norm(W0, dim=1) * (1 + 0.1 * T.randn(d_out, generator=g, dtype=T.float64))
    b = T.randn(d_out, generator=g, dtype=T.float64) * 0.1
    return x, dy, y, W0, A, Bm, m, b


def _kernel_ref(T, x, dy, y, W0, A, Bm, m, b, s, ysc):
    """float64 on the operands the matrix cores see: A and (g B) rounded to bf16 for u and v (a single row at r = 1
    otherwise measures the cancellation of one dot product, not the kernel)."""
    x, dy, y = x.double(), dy.double(), y.double()
    n = T.linalg.norm(W0 + s * (Bm @ A), dim=1)
    g = ysc * (m / n)
    gdy = dy * g
    rb = lambda t: t.to(T.bfloat16).double()
    u = x @ rb(A).T
    v = dy @ rb(g[:, None] * Bm)
    dB = s * gdy.T @ u
    dA = s * v.T @ x
    dm = ((dy * (y - b)).sum(0)) / m
    return dA, dB, dm, n


@pytest.mark.parametrize("d", [128, 384, 512, 768, 1024, 1280])
@pytest.mark.parametrize("kind", ["square", "fc1", "fc2"])
def test_adapter_grads_kernel_vs_fp64(T, gww, d, kind):
    from gw_whisper_amd import ops
    d_in, d_out = {"square": (d, d), "fc1": (d, 4 * d), "fc2": (4 * d, d)}[kind]
    cases = [(M, r) for M in (1, 31, 777, 3000) for r in (1, 8, 16, 64)]
    for i, (M, r) in enumerate(cases):
        if M == 3000 and d >= 1024 and r in (1, 8):
            continue   # the long-M cases at the widest shapes: r 16 / 64 cover them
        pad = 8 * (i % 3)
        ysc = 0.125 if i % 5 == 0 else 1.0
        x, dy, y, W0, A, Bm, m, b = _kernel_case(T, M, d_in, d_out, r, seed=1000 * d + i, stride_pad=pad)
        xc, dyc, yc = x.cuda()[:, :d_in], dy.cuda()[:, :d_out], y.cuda()[:, :d_out]   # rows strided by the padding
        x, dy, y = x[:, :d_in], dy[:, :d_out], y[:, :d_out]
        s = 32.0 / r
        dA, dB, dm, n = _kernel_ref(T, x, dy, y, W0, A, Bm, m, b, s, ysc)
        if pad:
            assert xc.stride(0) == d_in + pad
        f = lambda t: t.float().cuda()
        got = ops.adapter_grads(xc, dyc, yc, f(b), ysc, s, f(A), f(Bm), f(m), f(n))
        for name, g_, r_ in zip(("dA", "dB", "dm"), got, (dA, dB, dm)):
            g_ = g_.double().cpu()
            rel = float(T.linalg.norm(g_ - r_) / (T.linalg.norm(r_) + 1e-30))
            assert rel <= 0.02, (kind, d, M, r, name, rel)
        if i % 4 == 0:   # repeated calls: identical bits
            again = ops.adapter_grads(xc, dyc, yc, f(b), ysc, s, f(A), f(Bm), f(m), f(n))
            assert all(T.equal(a, b_) for a, b_ in zip(got, again)), (kind, d, M, r)


def test_adapter_grads_rank_limit(T, gww):
    from gw_whisper_amd import ops
    from gw_whisper_amd._lib import GwwError
    x, dy, y, W0, A, Bm, m, b = _kernel_case(T, 64, 128, 512, 65, seed=5)
    f = lambda t: t.float().cuda()
    with pytest.raises(GwwError, match="64"):
        ops.adapter_grads(x.cuda(), dy.cuda(), y.cuda(), f(b), 1.0, 0.5, f(A), f(Bm), f(m), f(m))


# ------------------------------------------------------------------ MLP-only adapters
@pytest.mark.parametrize("enc_name", ["tiny", "base"])
def test_mlp_only_adapters_train_and_repack(T, gww, enc_name):
    """target_modules=["fc1", "fc2"]: autograd runs, every adapter parameter gets a finite nonzero gradient, and after
    one AdamW step the next forward equals a fresh encoder loaded with the stepped adapter values."""
    from gw_whisper_amd.encoder import WhisperConfig, WhisperEncoder
    from gw_whisper_amd.peft import LoraConfig, get_peft_model
    d, L, H, F = synth.ENCODER_SIZES[enc_name]
    L = min(L, 4)
    sd = synth.encoder_state_dict(d, L, H, F, seed=5)

    def build():
        enc = WhisperEncoder.from_numpy_state_dict(sd, WhisperConfig(d, L, H, F), precision="bf16")
        peft = get_peft_model(enc, LoraConfig(use_dora=True, r=8, lora_alpha=32, target_modules=["fc1", "fc2"])).cuda()
        for n, p in peft.named_parameters():
            p.requires_grad = "lora" in n
        return peft

    peft = build()
    with T.no_grad():
        for n, p in peft.named_parameters():
            if "lora_B" in n:
                p.copy_(0.02 * T.randn_like(p))
    mel = T.from_numpy(olm.log_mel(synth.strain_segments(2, seed=9))).cuda()
    params = [p for p in peft.parameters() if p.requires_grad]
    assert len(params) == 3 * 2 * L
    opt = T.optim.AdamW(params, lr=1e-3)
    out = peft.last_token(mel)
    out.square().sum().backward()
    for n, p in peft.named_parameters():
        if p.requires_grad:
            assert p.grad is not None and T.isfinite(p.grad).all() and float(p.grad.abs().max()) > 0, n
    opt.step()
    with T.no_grad():
        after = peft(mel).last_hidden_state
        fresh = build()
        fresh.load_state_dict(peft.state_dict())
        ref = fresh(mel).last_hidden_state
    assert T.equal(after, ref)


# ------------------------------------------------------------------ harness
def test_run_train_rank_and_targets(T, gww, tmp_path):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = str(tmp_path)
    base = [sys.executable, os.path.join(root, "harness", "run_train.py"), "--synthetic", "96", "--encoder", "micro",
            "--batch-size", "16", "--learning-rate", "1e-3", "--lora-rank", "16",
            "--lora-targets", "layers.*.fc1", "layers.*.self_attn.v_proj"]
    r = subprocess.run(base + ["--num-epochs", "3", "--models-path", out + "/m1", "--log-dir", out + "/l1"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    recs = [json.loads(l) for l in open(out + "/l1/train_log.jsonl")]
    assert recs[-1]["train_loss"] < recs[0]["train_loss"]
    cfg = json.load(open(out + "/m1/lora_weights_16_32/adapter_config.json"))
    assert cfg["r"] == 16
    assert sorted(cfg["target_modules"]) == sorted(f"layers.{i}.{p}" for i in range(2) for p in ("fc1", "self_attn.v_proj"))
    r = subprocess.run(base + ["--num-epochs", "1", "--models-path", out + "/m2", "--log-dir", out + "/l2",
                               "--load_model_path", out + "/m1", "--load_lora_weights", "lora_weights_16_32",
                               "--load_dense_weights", "dense_layers_16_32.pth"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    second = [json.loads(l) for l in open(out + "/l2/train_log.jsonl")]
    assert np.isfinite(second[0]["train_loss"]) and second[0]["train_loss"] < recs[0]["train_loss"]
    cfg2 = json.load(open(out + "/m2/lora_weights_16_32/adapter_config.json"))
    assert cfg2["r"] == 16 and sorted(cfg2["target_modules"]) == sorted(cfg["target_modules"])
