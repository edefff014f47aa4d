"""GPU checks of the binary head step inside a training step, and of the single-detector trainer
(harness/run_train.py --detectors 1, the counterpart of the reference's Signal_vs_Noise/src/sd_train.py).

The step test holds the rule of tests/test_gpu_binary_head.py to a whole DoRA step: from one state, the micro encoder
(d = 128, precision fp32, DoRA on q / k / v) produces its pooled tokens, and the head runs three ways on them -- the HIP
step (``binary.head_bce_with_logits``), the torch fp32 head it replaces (``classifier(pooled)`` + ``BCEWithLogitsLoss``)
and binary_helpers.head64 in fp64.  The head gradients are compared with the fp64 ones directly; the adapter gradients of
each are what the same exact-fp32 encoder backward makes of that head's pooled-token gradient, the fp64 side's being its
pooled-token gradient rounded to fp32 once.  For every gradient: relative Frobenius error of HIP <= 2 x torch's +
20 * 2^-24."""

import json
import os
import subprocess
import sys

import numpy as np
import pytest

from . import binary_helpers as bh

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS20 = 20.0 * 2.0 ** -24


@pytest.fixture(scope="module")
def T():
    import torch
    assert torch.cuda.is_available()
    return torch


def _rel(a, ref):
    d = float((a.double() - ref.double()).norm())
    n = float(ref.double().norm())
    return 0.0 if d == 0.0 else d / n if n > 0 else float("inf")


def _model(T, detectors):
    """harness/run_train.py's construction on the micro encoder: DoRA (r = 8, alpha = 32) on q / k / v, lora_B seeded
    away from its zero initialisation so that every adapter gradient is non-trivial."""
    import fnmatch
    from gw_whisper_amd import models, synth
    from gw_whisper_amd.encoder import WhisperConfig, WhisperEncoder
    from gw_whisper_amd.peft import LoraConfig, get_peft_model
    T.manual_seed(0)                  # peft's lora_A initialisation draws from the global generator
    d, L, H, F = synth.ENCODER_SIZES["micro"]
    enc = WhisperEncoder(WhisperConfig.named("micro"), precision="fp32")
    enc.load_state_dict({k: T.from_numpy(v) for k, v in synth.encoder_state_dict(d, L, H, F, seed=5).items()})
    names = [n for n, _ in enc.named_modules()]
    matched = [m for p in ("layers.*.self_attn.q_proj", "layers.*.self_attn.k_proj", "layers.*.self_attn.v_proj")
               for m in fnmatch.filter(names, p)]
    assert len(matched) == 3 * L
    peft = get_peft_model(enc, LoraConfig(use_dora=True, r=8, lora_alpha=32, target_modules=matched)).cuda()
    for name, p in peft.named_parameters():
        p.requires_grad = "lora" in name
    cls = models.one_channel_ligo_binary_classifier if detectors == 1 else models.two_channel_ligo_binary_classifier
    model = cls(peft).cuda()
    layout = bh.ONE if detectors == 1 else bh.TWO
    sd = synth.head_state_dict([d * detectors, *bh.WIDTHS[layout], 1], seed=9)
    model.classifier.load_state_dict({k: T.from_numpy(v) for k, v in sd.items()})
    with T.no_grad():
        gen = T.Generator().manual_seed(2)
        for n_, p_ in model.encoder.named_parameters():
            if "lora_B" in n_:
                p_.copy_(0.05 * T.randn(p_.shape, generator=gen))
    return model.train(), layout


@pytest.mark.parametrize("detectors", [1, 2])
def test_one_dora_step_hip_head_against_torch_head(T, gww, detectors):
    """B = 6 segments, micro encoder, both --detectors values.  Measured on MI355X, worst gradient, HIP / torch: head 3.3e-7 / 2.3e-7
    (one detector), 3.2e-7 / 1.7e-7 (two); adapters 6.5e-7 / 4.7e-7 (one), 1.3e-6 / 6.1e-7 (two: layers.1 k_proj lora_A);
    loss 9.6e-9 / 9.6e-9."""
    from gw_whisper_amd import binary, ops, synth
    model, layout = _model(T, detectors)
    B = 6
    mels = tuple(ops.logmel(T.from_numpy(synth.strain_segments(B, seed=11 + i)).cuda()) for i in range(detectors))
    # five signals and one noise label: the pooled tokens of noise segments are close to one another and every sigmoid is
    # close to 1/2, so with balanced labels each gradient would be sum_i dz_i h_i with sum_i dz_i ~ 0 -- a cancellation
    # residue whose relative error (1e-5 for the torch head as for the HIP one) says nothing about either head
    y = T.tensor([[1.], [1.], [0.], [1.], [1.], [1.]], device="cuda")
    trainable = {n: p for n, p in model.named_parameters() if p.requires_grad}
    head_keys = [k for k in trainable if k.startswith("classifier.")]
    adapter_keys = [k for k in trainable if not k.startswith("classifier.")]
    assert len(head_keys) == 2 * (len(bh.WIDTHS[layout]) + 1) and any("lora_A" in k for k in adapter_keys)
    assert any("magnitude" in k for k in adapter_keys)

    def grads(loss_of):
        """gradients of every trainable parameter for loss_of(pooled) -> a scalar (or a (pooled, gradient) pair)"""
        for p in trainable.values():
            p.grad = None
        pooled = model.pooled(*mels)
        out = loss_of(pooled)
        if isinstance(out, tuple):
            out[0].backward(out[1])
        else:
            out.backward()
        return pooled.detach().clone(), {k: (None if p.grad is None else p.grad.detach().clone()) for k, p in trainable.items()}

    state = {}

    def hip(pooled):
        state["hip"], logits = binary.head_bce_with_logits(model.classifier, pooled, y)
        assert not logits.requires_grad and tuple(logits.shape) == (B, 1)
        return state["hip"]

    def torch_head(pooled):
        state["torch"] = T.nn.BCEWithLogitsLoss()(model.classifier(pooled), y)
        return state["torch"]

    def fp64(pooled):
        params = [trainable[k] for k in head_keys]
        assert [k[len("classifier."):] for k in head_keys] == list(bh.param_keys(layout))
        l64, _, _, _, dx64, g64, margin = bh.head64(pooled, params, y)
        assert margin >= bh.MARGIN, f"a hidden pre-activation of the step's own pooled tokens is {margin:.2e} from zero"
        state["fp64"], state["g64"] = l64, dict(zip(head_keys, g64))
        return pooled, dx64.to(T.float32)

    x_h, g_h = grads(hip)
    x_t, g_t = grads(torch_head)
    x_r, g_r = grads(fp64)
    assert T.equal(x_h, x_t) and T.equal(x_h, x_r)      # one state: the encoder forward is the same in all three
    assert tuple(x_h.shape) == (B, 128 * detectors)
    g_r.update(state["g64"])
    l_h, l_t, l_r = (float(state[k].detach()) for k in ("hip", "torch", "fp64"))
    e_h, e_t = abs(l_h - l_r) / l_r, abs(l_t - l_r) / l_r
    print(f"detectors {detectors}: loss rel err hip {e_h:.2e} torch {e_t:.2e}")
    assert e_h <= 2 * e_t + EPS20
    for k in head_keys + adapter_keys:
        assert g_h[k] is not None and bool(T.isfinite(g_h[k]).all()), k
        e_h, e_t = _rel(g_h[k], g_r[k]), _rel(g_t[k], g_r[k])
        print(f"detectors {detectors}: {k:70s} rel err hip {e_h:.2e} torch {e_t:.2e}")
        assert e_h <= 2 * e_t + EPS20, (k, e_h, e_t)


def test_single_detector_trainer_end_to_end(T, gww, tmp_path):
    """harness/run_train.py --detectors 1 --head-step hip on 64 synthetic segments in a fresh child process: the four
    artefacts, the saved head under the reference's keys and shapes, a finite loss and AUC in the log."""
    from gw_whisper_amd import models
    mp, ld = str(tmp_path / "models"), str(tmp_path / "logs")
    cmd = [sys.executable, os.path.join(ROOT, "harness", "run_train.py"), "--detectors", "1", "--head-step", "hip", "--synthetic",
           "64", "--batch-size", "16", "--num-epochs", "1", "--encoder", "micro", "--models-path", mp, "--log-dir", ld]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    for prefix in ("", "best_"):
        assert os.path.isfile(os.path.join(mp, f"{prefix}lora_weights_8_32", "adapter_config.json"))
        assert os.path.isfile(os.path.join(mp, f"{prefix}lora_weights_8_32", "adapter_model.safetensors"))
        sd = T.load(os.path.join(mp, f"{prefix}dense_layers_8_32.pth"), map_location="cpu")
        assert list(sd) == list(bh.param_keys(bh.ONE))
        assert [tuple(sd[f"{2 * i}.weight"].shape) for i in range(5)] == [(512, 128), (256, 512), (128, 256), (64, 128), (1, 64)]
        enc = type("Enc", (), {"config": type("Cfg", (), {"d_model": 128})()})()
        models.one_channel_ligo_binary_classifier(enc).classifier.load_state_dict(sd)
    recs = [json.loads(l) for l in open(os.path.join(ld, "train_log.jsonl"))]
    assert len(recs) == 1 and recs[0]["epoch"] == 1
    for k in ("train_loss", "val_loss", "val_auc"):
        assert np.isfinite(recs[0][k]), (k, recs[0])
    assert 0.0 <= recs[0]["val_auc"] <= 1.0 and recs[0]["train_loss"] > 0 and recs[0]["val_loss"] > 0
    assert "Epoch 1/1" in r.stdout
