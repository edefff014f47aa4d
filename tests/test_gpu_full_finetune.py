"""Full fine-tuning on the GPU (Signal_vs_Noise/src/train.py:243-247 ``--method full_finetune``): the weight-gradient
GEMM and the LayerNorm gain / bias gradients against fp64, every base-parameter gradient of the encoder backward
against fp64 autograd of a float64 torch restatement of the HF Whisper encoder, an AdamW step that re-packs every
weight group, and the harness end to end.  Needs an MI355X."""

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

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def T():
    import torch
    assert torch.cuda.is_available()
    return torch


def _bf16(T, shape, seed, scale=1.0):
    g = T.Generator(device="cuda").manual_seed(seed)
    return (T.randn(shape, generator=g, device="cuda") * scale).bfloat16()


def _check_wgrad(T, dy, x, dw, db=None, alpha=1.0, dw0=None):
    """error <= 1e-3 of sum_m |dy| |x| per element (fp64 matmul of the same bf16 values)."""
    dy64, x64 = dy.double(), x.double()
    ref = alpha * dy64.t() @ x64
    bound = abs(alpha) * dy64.abs().t() @ x64.abs()
    if dw0 is not None:
        ref = ref + dw0.double()
    err = (dw.double() - ref).abs()
    assert (err <= 1e-3 * bound + 1e-6).all(), float((err / (bound + 1e-30)).max())
    if db is not None:
        dbr = alpha * dy64.sum(0)
        dbb = abs(alpha) * dy64.abs().sum(0)
        assert ((db.double() - dbr).abs() <= 1e-3 * dbb + 1e-6).all()


@pytest.mark.parametrize("M,N,K", [(96000, 1152, 384), (96000, 384, 384), (96000, 1536, 384), (96000, 384, 1536),
                                   (64, 384, 384), (64, 1536, 384), (3001, 128, 512)])
def test_wgrad_matches_fp64(T, gww, M, N, K):
    from gw_whisper_amd import ops
    dy = _bf16(T, (M, N), M + N, 0.5)
    x = _bf16(T, (M, K), M + K + 1)
    dw, db = ops.gemm_wgrad(dy, x, db=True)
    _check_wgrad(T, dy, x, dw, db)


def test_wgrad_accumulates_and_is_bit_reproducible(T, gww):
    from gw_whisper_amd import ops
    M, N, K = 20000, 384, 1536
    dy = _bf16(T, (M, N), 5, 0.5)
    x = _bf16(T, (M, K), 6)
    dw0 = T.randn((N, K), device="cuda")
    db0 = T.randn((N,), device="cuda")
    dw, db = ops.gemm_wgrad(dy, x, dw=dw0.clone(), db=db0.clone(), alpha=0.18)
    _check_wgrad(T, dy, x, dw, alpha=0.18, dw0=dw0)
    assert ((db.double() - db0.double() - 0.18 * dy.double().sum(0)).abs()
            <= 1e-3 * 0.18 * dy.double().abs().sum(0) + 1e-5).all()
    dw2, db2 = ops.gemm_wgrad(dy, x, dw=dw0.clone(), db=db0.clone(), alpha=0.18)
    assert T.equal(dw, dw2) and T.equal(db, db2)   # fixed-order reduction: identical bits


def test_wgrad_strided_conv_views(T, gww):
    """conv2 = dz2^T view(c1, ldx = 2 d, K = 3 d) and conv1 = dz1^T view(melT, ldx = 80, K = 256), the views the
    forward GEMMs read; the junk row of every segment carries zero gradient."""
    from gw_whisper_amd import ops
    B, Tn, d, C = 3, 1500, 384, 80
    Tin = 2 * Tn
    # conv2: M2 = B (T + 1) rows, row b (T + 1) + t reads c1 rows 2 t .. 2 t + 2 of the padded token-major c1
    M2 = B * (Tn + 1)
    c1 = _bf16(T, (2 * M2 + 2, d), 11)
    dz2 = _bf16(T, (M2, d), 12, 0.5).view(B, Tn + 1, d)
    dz2[:, Tn] = 0
    dz2 = dz2.reshape(M2, d)
    view2 = c1.as_strided((M2, 3 * d), (2 * d, 1))
    dw, db = ops.gemm_wgrad(dz2, view2, db=True, k=3 * d)
    _check_wgrad(T, dz2, view2, dw, db)
    # conv1: M1 = B (Tin + 2) rows, row m reads melT[m .. m + 3) (80 channels each) + 16 padding columns
    M1 = B * (Tin + 2)
    melT = _bf16(T, (M1 * C + 256,), 13)
    dz1 = _bf16(T, (M1, d), 14, 0.5).view(B, Tin + 2, d)
    dz1[:, Tin:] = 0
    dz1 = dz1.reshape(M1, d)
    view1 = melT.as_strided((M1, 256), (C, 1))
    dw1, db1 = ops.gemm_wgrad(dz1, view1, db=True, k=256)
    _check_wgrad(T, dz1, view1, dw1, db1)


def test_wgrad_rejects_bad_strides_and_shapes(T, gww):
    from gw_whisper_amd import ops
    dy = _bf16(T, (100, 128), 1)
    x = _bf16(T, (100, 132), 2)
    with pytest.raises(gww.GwwError, match="multiples of 8"):
        ops.gemm_wgrad(dy, x[:, :128].as_strided((99, 128), (129, 1)), rows=99)
    with pytest.raises(gww.GwwError, match="multiple of 64"):
        ops.gemm_wgrad(_bf16(T, (100, 96), 3), x[:, :128].contiguous())
    with pytest.raises(gww.GwwError, match="multiple of 16"):
        ops.gemm_wgrad(dy, x[:, :120].contiguous())


@pytest.mark.parametrize("d", [128, 384, 512, 768, 1024, 1280])
@pytest.mark.parametrize("dy_f32", [True, False])
def test_layernorm_param_grads_match_fp64(T, gww, d, dy_f32):
    from gw_whisper_amd import ops
    M = 3001
    g = T.Generator(device="cuda").manual_seed(d)
    x = T.randn((M, d), generator=g, device="cuda") * 2 + 0.5
    dy = T.randn((M, d), generator=g, device="cuda")
    if not dy_f32:
        dy = dy.bfloat16()
    dg0 = T.randn(d, device="cuda")
    dgamma, dbeta = ops.layernorm_param_grads(x, dy, dgamma=dg0.clone())
    x64, dy64 = x.double(), dy.double()
    xhat = (x64 - x64.mean(1, keepdim=True)) / T.sqrt(x64.var(1, unbiased=False, keepdim=True) + 1e-5)
    ref_g, ref_b = (dy64 * xhat).sum(0) + dg0.double(), dy64.sum(0)
    bound = (dy64.abs() * xhat.abs()).sum(0)
    assert ((dgamma.double() - ref_g).abs() <= 1e-4 * bound + 1e-5).all()
    assert ((dbeta.double() - ref_b).abs() <= 1e-4 * dy64.abs().sum(0) + 1e-5).all()
    again = ops.layernorm_param_grads(x, dy, dgamma=dg0.clone())
    assert T.equal(again[0], dgamma) and T.equal(again[1], dbeta)


# two-layer encoders of whisper-base / -small / -medium width: every kernel route of those widths at a small cost
_SIZES = dict(synth.ENCODER_SIZES, base_l2=(512, 2, 8, 2048), small_l2=(768, 2, 12, 3072), medium_l2=(1024, 2, 16, 4096))


@pytest.mark.parametrize("mode", ["hidden", "last_token"])
@pytest.mark.parametrize("enc_name", ["micro", "tiny", "base_l2", "small_l2", "medium_l2"])
def test_every_base_gradient_matches_fp64_autograd(T, gww, enc_name, mode):
    """loss.backward() through the fully fine-tuned HIP encoder: every base parameter's gradient against fp64 autograd
    (per-tensor relative Frobenius error <= 3 %, the bf16-vs-fp64 bound of the DoRA tests), two central finite-difference
    directions of the fp64 loss, and d_mel requested in the same step (hidden mode)."""
    from gw_whisper_amd.encoder import WhisperConfig, WhisperEncoder
    d, L, H, F = _SIZES[enc_name]
    sd = synth.encoder_state_dict(d, L, H, F, seed=3)
    mel = olm.log_mel(synth.strain_segments(2, seed=33))
    enc = WhisperEncoder.from_numpy_state_dict(sd, WhisperConfig(d, L, H, F), precision="bf16").cuda()
    enc.enable_full_finetune()
    for p in enc.parameters():
        p.requires_grad = True
    # the loss of the DoRA tests: a weighted sum of token T - 1, read from the full last_hidden_state (every row of
    # every layer below the last runs dense) or from the pooled last_token step
    wl = np.random.default_rng(7).standard_normal((2, d))
    want_mel = mode == "hidden"
    mel_t = T.from_numpy(mel).cuda().requires_grad_(want_mel)
    out = enc(mel_t).last_hidden_state[:, -1, :] if mode == "hidden" else enc.last_token(mel_t)
    (out * T.from_numpy(wl).cuda().float()).sum().backward()
    names = [n for n, _ in enc.named_parameters()]
    got = {n: p.grad.double().cpu() for n, p in enc.named_parameters()}

    p64 = {k: T.from_numpy(v).double().requires_grad_(True) for k, v in sd.items()}
    mel64 = T.from_numpy(mel).double().requires_grad_(want_mel)
    wl64 = T.from_numpy(wl)

    def loss64(params, m):
        h = encoder64(T, params, m, (d, L, H))
        return (h[:, -1, :] * wl64).sum()

    l64 = loss64(p64, mel64)
    l64.backward()
    assert set(names) == set(p64)
    worst = []
    for n in names:
        ref = p64[n].grad
        rel = float(T.linalg.norm(got[n] - ref) / (T.linalg.norm(ref) + 1e-30))
        worst.append((rel, n))
        assert T.isfinite(got[n]).all(), n
    worst.sort(reverse=True)
    print(enc_name, mode, "worst relative Frobenius errors:", [(round(r, 4), n) for r, n in worst[:5]])
    # q_proj / k_proj gradients reach the weights only through the softmax backward, whose P and dS operands are bf16
    # (attention_bwd.hip): for whisper-tiny's last layer they measure 3.5 %; every other tensor stays within 3 %
    for rel, n in worst:
        assert rel <= (0.05 if ("q_proj" in n or "k_proj" in n) else 0.03), (n, rel, worst[:5])
    if want_mel:
        rel = float(T.linalg.norm(mel_t.grad.double().cpu() - mel64.grad) / T.linalg.norm(mel64.grad))
        assert rel <= 0.03, rel
    # two central finite-difference directions of the fp64 loss over all base parameters
    with T.no_grad():
        for trial in range(2):
            g = np.random.default_rng(100 + trial)
            dirs = {k: T.from_numpy(g.standard_normal(v.shape)) * float(v.detach().pow(2).mean().sqrt() + 1e-6)
                    for k, v in p64.items()}
            eps = 1e-4
            plus = {k: v.detach() + eps * dirs[k] for k, v in p64.items()}
            minus = {k: v.detach() - eps * dirs[k] for k, v in p64.items()}
            fd = float(loss64(plus, mel64.detach()) - loss64(minus, mel64.detach())) / (2 * eps)
            an = sum(float((got[k] * dirs[k]).sum()) for k in names)
            S = np.sqrt(sum(float(((got[k] * dirs[k]) ** 2).sum()) for k in names))
            print(f"direction {trial}: analytic(HIP, bf16) {an:.5f}  finite-difference(fp64) {fd:.5f}")
            assert abs(an - fd) < 0.03 * max(abs(fd), S) + 2e-3, (an, fd, S)


def test_adamw_step_repacks_every_weight_group(T, gww):
    """After one AdamW step on a fully fine-tuned whisper-tiny (pooled, as the classifiers train), the encoder computes
    what a fresh encoder built from its state_dict() computes: every changed group was re-packed."""
    from gw_whisper_amd.encoder import WhisperConfig, WhisperEncoder
    d, L, H, F = synth.ENCODER_SIZES["tiny"]
    sd = synth.encoder_state_dict(d, L, H, F, seed=5)
    cfg = WhisperConfig(d, L, H, F)
    enc = WhisperEncoder.from_numpy_state_dict(sd, cfg, precision="bf16").cuda().enable_full_finetune()
    for p in enc.parameters():
        p.requires_grad = True
    opt = T.optim.AdamW([p for p in enc.parameters() if p.requires_grad], lr=1e-3)
    mel = T.from_numpy(olm.log_mel(synth.strain_segments(4, seed=8))).cuda()
    with T.no_grad():
        before = enc(mel).last_hidden_state.clone()
    loss = enc.last_token(mel).pow(2).mean()
    loss.backward()
    assert all(p.grad is not None and T.isfinite(p.grad).all() for p in enc.parameters())
    opt.step()
    opt.zero_grad()
    with T.no_grad():
        after = enc(mel).last_hidden_state
        fresh = WhisperEncoder(cfg, precision="bf16").cuda()
        fresh.load_state_dict(enc.state_dict())
        ref = fresh(mel).last_hidden_state
    diff = float((after - ref).abs().max())
    moved = float((after - before).abs().max())
    assert diff < 2e-2, diff                 # same weights: equal within the bf16 forward tolerance
    assert moved > 10 * max(diff, 1e-3), (moved, diff)


def test_full_finetune_refuses_adapters(T, gww):
    from gw_whisper_amd.encoder import WhisperConfig, WhisperEncoder
    from gw_whisper_amd.peft import LoraConfig, get_peft_model
    d, L, H, F = synth.ENCODER_SIZES["micro"]
    enc = WhisperEncoder.from_numpy_state_dict(synth.encoder_state_dict(d, L, H, F, seed=1), WhisperConfig(d, L, H, F))
    enc.cuda().enable_full_finetune()
    get_peft_model(enc, LoraConfig(use_dora=True, r=8, lora_alpha=32, target_modules=["layers.0.self_attn.q_proj"]))
    for p in enc.parameters():
        p.requires_grad = True
    mel = T.from_numpy(olm.log_mel(synth.strain_segments(1, seed=2))).cuda()
    with pytest.raises(gww.GwwError, match="adapters"):
        enc(mel)


def test_run_train_full_finetune_end_to_end(T, gww, tmp_path):
    """run_train.py --method full_finetune: exits 0 with finite losses, saves the encoder with the HF encoder keys, and
    the saved model.safetensors reloads through --encoder-weights to the same forward."""
    from safetensors.torch import load_file

    from gw_whisper_amd.encoder import WhisperConfig, WhisperEncoder
    models, logs = tmp_path / "models", tmp_path / "logs"
    cmd = [sys.executable, os.path.join(ROOT, "harness", "run_train.py"), "--method", "full_finetune", "--synthetic", "64",
           "--encoder", "micro", "--num-epochs", "2", "--batch-size", "16", "--models-path", str(models),
           "--log-dir", str(logs)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    recs = [json.loads(x) for x in open(logs / "train_log.jsonl")]
    assert len(recs) == 2 and all(np.isfinite(x["train_loss"]) and np.isfinite(x["val_loss"]) for x in recs)
    out_dir = models / "lora_weights_8_32"
    cfg = json.load(open(out_dir / "config.json"))
    d, L, H, F = synth.ENCODER_SIZES["micro"]
    assert (cfg["d_model"], cfg["encoder_layers"], cfg["encoder_attention_heads"], cfg["encoder_ffn_dim"]) == (d, L, H, F)
    sd = load_file(str(out_dir / "model.safetensors"))
    ref_keys = set(WhisperEncoder(WhisperConfig(d, L, H, F)).state_dict())
    assert set(sd) == ref_keys
    init = synth.encoder_state_dict(d, L, H, F, seed=42)
    assert any(not np.array_equal(sd[k].numpy(), init[k]) for k in ("conv1.weight", "layers.0.fc1.weight",
                                                                  "embed_positions.weight"))
    # the reload path of --encoder-weights (harness: load_state_dict(load_file(...))) gives the trained encoder, not the
    # seeded initial one
    mel = T.from_numpy(olm.log_mel(synth.strain_segments(2, seed=4))).cuda()
    trained = WhisperEncoder(WhisperConfig(d, L, H, F)).cuda()
    trained.load_state_dict(sd)
    initial = WhisperEncoder.from_numpy_state_dict(init, WhisperConfig(d, L, H, F)).cuda()
    with T.no_grad():
        a = trained(mel).last_hidden_state
        c = initial(mel).last_hidden_state
    assert T.isfinite(a).all() and float((a - c).abs().max()) > 1e-2
    r2 = subprocess.run(cmd[:-4] + ["--num-epochs", "1", "--encoder-weights", str(out_dir / "model.safetensors"),
                                    "--models-path", str(tmp_path / "m2"), "--log-dir", str(tmp_path / "l2")],
                        capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r2.returncode == 0, r2.stderr[-4000:]
