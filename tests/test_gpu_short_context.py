"""Encoders of a context other than 1500 tokens (``WhisperConfig(max_source_positions=T)``) on the GPU: T = 16 (B 1), 50
(B 5: ragged below one key tile and one row panel), 100 (B 3, M = 300), 128 and 512 (t_in 1024, where the stem shortcut's
guard flips), at widths 128 (micro), 384 (the fused-block route) and 512 (two layers, the generic route).  Forward in
fp32 and bf16 against ``tests.helpers.encoder64`` under the bounds of test_gpu_encoder.py::test_named_sizes_match_oracle
and against HF's float64 encoder (tests/golden/short_context_hf.npz); pooling and batch independence; per-layer outputs;
the stem shortcut; the DoRA, full fine-tuning and fp32 training steps against fp64 autograd under the criteria of their
own test files."""

import json
import os
import subprocess
import sys

import numpy as np
import pytest

import gw_whisper_amd
from gw_whisper_amd import synth
from tests.helpers import dora64, encoder64

pytestmark = pytest.mark.gpu

WIDTHS = {128: (128, 2, 2, 512), 384: (384, 2, 6, 1536), 512: (512, 2, 8, 2048)}
SHAPES = [(16, 1), (50, 5), (100, 3), (128, 2), (512, 2)]      # (T, B)
_REF = {}


@pytest.fixture(scope="module")
def T():
    import torch
    assert torch.cuda.is_available()
    return torch


def features(seed, B, Tn, n_mels=80):
    """Seeded stand-in for log-mel features [B, n_mels, 2 T] in the range Whisper's normalised log-mel takes."""
    return np.clip(np.random.default_rng(seed).standard_normal((B, n_mels, 2 * Tn)) * 0.5, -1.5, 1.5).astype(np.float32)


def weights(d, Tn, seed=5):
    dd, L, H, F = WIDTHS[d]
    sd = synth.encoder_state_dict(dd, L, H, F, seed=seed)
    sd["embed_positions.weight"] = sd["embed_positions.weight"][:Tn].copy()
    return sd


def build(T, d, Tn, precision, seed=5, sd=None):
    from gw_whisper_amd.encoder import WhisperConfig, WhisperEncoder
    dd, L, H, F = WIDTHS[d]
    sd = weights(d, Tn, seed) if sd is None else sd
    return WhisperEncoder.from_numpy_state_dict(sd, WhisperConfig(dd, L, H, F, max_source_positions=Tn), precision=precision).cuda()


def reference(T, d, Tn, B):
    """encoder64 of the seeded weights and features, computed once per case (float64 numpy, read-only)."""
    key = (d, Tn, B)
    if key not in _REF:
        dd, L, H, F = WIDTHS[d]
        p = {k: T.from_numpy(v).double() for k, v in weights(d, Tn).items()}
        with T.no_grad():
            ref = encoder64(T, p, T.from_numpy(features(100 + Tn, B, Tn)).double(), (dd, L, H)).numpy()
        ref.setflags(write=False)
        _REF[key] = ref
    return _REF[key]


# ---------------------------------------------------------------------------------------------------- forward
@pytest.mark.parametrize("Tn,B", SHAPES)
@pytest.mark.parametrize("d", sorted(WIDTHS))
def test_forward_matches_fp64(T, gww, d, Tn, B):
    """fp32 within 1e-3 of the float64 restatement, bf16 within 0.15 (mean 6e-3); last_token is the last row of the full
    forward (fp32: 1e-5, bf16: the pooled-forward bound 0.06 of test_gpu_encoder.py)."""
    ref = reference(T, d, Tn, B)
    x = T.from_numpy(features(100 + Tn, B, Tn)).cuda()
    enc = build(T, d, Tn, "fp32")
    with T.no_grad():
        out32 = enc(x).last_hidden_state
        last32 = enc.last_token(x)
    assert out32.shape == (B, Tn, WIDTHS[d][0])
    e32 = float(np.abs(out32.cpu().numpy() - ref).max())
    assert float((last32 - out32[:, -1]).abs().max()) <= 1e-5
    enc.precision = "bf16"
    with T.no_grad():
        out16 = enc(x).last_hidden_state
        last16 = enc.last_token(x)
    T.cuda.synchronize()
    err16 = np.abs(out16.cpu().numpy() - ref)
    e_pool = float((last16 - out16[:, -1]).abs().max())
    print(f"d {d} T {Tn} B {B}: fp32 {e32:.3e}  bf16 max {err16.max():.3e} mean {err16.mean():.3e}  pooled {e_pool:.3e}")
    assert e32 < 1e-3
    assert err16.max() < 0.15 and err16.mean() < 6e-3
    assert e_pool < 0.06


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_t100_matches_hf_float64(T, gww, golden, precision):
    """HF's own WhisperEncoder in float64 with max_source_positions 100 (tools/make_golden_frontend.py)."""
    g = golden("short_context_hf.npz")
    d, L, H, F, Tn, wseed, iseed = (int(v) for v in g["config"])
    assert (d, L, H, F) == WIDTHS[128] and Tn == 100
    enc = build(T, 128, Tn, precision, seed=wseed)
    with T.no_grad():
        out = enc(T.from_numpy(features(iseed, 2, Tn)).cuda()).last_hidden_state.cpu().numpy()
    err = np.abs(out - g["last_hidden_state"])
    print(f"T 100 vs HF float64 [{precision}]: max {err.max():.3e} mean {err.mean():.3e}")
    assert (err.max() < 1e-3) if precision == "fp32" else (err.max() < 0.15 and err.mean() < 6e-3)


@pytest.mark.parametrize("d,Tn", [(128, 50), (384, 50), (384, 100), (512, 100)])
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_a_segment_does_not_depend_on_its_batch(T, gww, d, Tn, precision):
    """A segment's rows and its pooled token are bit-identical whatever its neighbours in the batch hold, and equal to
    the segment run alone (another launch geometry) within fp32 rounding (1e-5) or the pooled-forward bound (0.06)."""
    x = T.from_numpy(features(7, 5, Tn)).cuda()
    y = x.clone()
    y[0], y[1], y[3], y[4] = 1.5, -1.5, x[2], 0.0
    enc = build(T, d, Tn, precision)
    tol = 1e-5 if precision == "fp32" else 0.06
    with T.no_grad():
        full, pooled = enc(x).last_hidden_state, enc.last_token(x)
        other, pooled_other = enc(y).last_hidden_state, enc.last_token(y)
        assert T.equal(full[2], other[2]) and T.equal(pooled[2], pooled_other[2])
        assert T.equal(other[3], other[2]) and T.equal(pooled_other[3], pooled_other[2])
        for i in (0, 4):
            assert float((enc(x[i:i + 1]).last_hidden_state[0] - full[i]).abs().max()) <= tol
            assert float((enc.last_token(x[i:i + 1])[0] - pooled[i]).abs().max()) <= tol


def test_length_errors_keep_hf_wording(T, gww):
    enc = build(T, 128, 50, "bf16")
    with pytest.raises(ValueError, match="to be of length 100, but found 3000"):
        enc(T.zeros(1, 80, 3000, device="cuda"))
    from gw_whisper_amd.encoder import WhisperConfig, WhisperEncoder
    for bad in (15, 1501):
        with pytest.raises(ValueError, match="max_source_positions"):
            WhisperEncoder(WhisperConfig(128, 2, 2, 512, max_source_positions=bad))


# ---------------------------------------------------------------------------------------------------- outputs
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("d,Tn", [(128, 100), (384, 100), (384, 128), (512, 128)])
def test_per_layer_outputs_against_fp64(T, gww, d, Tn, precision):
    """attentions[l] against the float64 softmax of LN1(hidden_states[l])'s q . k, hidden_states[l + 1] against a float64
    layer applied to hidden_states[l]: the bounds of test_gpu_encoder_outputs.py::test_full_geometry_against_fp64."""
    from tests.test_gpu_encoder_outputs import FP64_ATT, FP64_HID, _check_rows, _layer64
    dd, L, H, F = WIDTHS[d]
    B = 3
    enc = build(T, d, Tn, precision)
    p = {k: T.from_numpy(v).double().cuda() for k, v in weights(d, Tn).items()}
    x = T.from_numpy(features(41, B, Tn)).cuda()
    with T.no_grad():
        o = enc(x, output_hidden_states=True, output_attentions=True)
        plain = enc(x).last_hidden_state
        assert T.equal(o.last_hidden_state, plain) and len(o.hidden_states) == L + 1 and len(o.attentions) == L
        ea, eh = [], []
        for l in range(L):
            assert o.attentions[l].shape == (B, H, Tn, Tn) and o.hidden_states[l].shape == (B, Tn, dd)
            xn, P = _layer64(T, p, l, o.hidden_states[l].double(), H, final=(l == L - 1))
            ea.append(float((o.attentions[l].double() - P).abs().max()))
            eh.append(float((o.hidden_states[l + 1].double() - xn).abs().max() / xn.abs().max()))
            _check_rows(T, o.attentions[l])
    print(f"d {d} T {Tn} {precision}: attn abs {['%.2e' % e for e in ea]}  hidden rel {['%.2e' % e for e in eh]}")
    assert max(ea) < FP64_ATT[precision] and max(eh) < FP64_HID[precision]


def test_attentions_need_a_context_of_a_multiple_of_four(T, gww):
    enc = build(T, 128, 50, "bf16")
    x = T.from_numpy(features(3, 1, 50)).cuda()
    with T.no_grad():
        with pytest.raises(gw_whisper_amd.GwwError, match="max_source_positions % 4"):
            enc(x, output_attentions=True)
        assert len(enc(x, output_hidden_states=True).hidden_states) == 3     # hidden states alone need no such length


# ---------------------------------------------------------------------------------------------------- stem shortcut
def constant_tail(B, Tn, live=200):
    x = features(11, B, Tn)
    x[:, :, live:] = x[:, :, live:live + 1]          # every row bitwise constant from frame `live` on
    return x


def test_stem_shortcut_at_t512_is_bit_identical(T, gww):
    """t_in 1024 is the shortest input the shortcut takes: constant-tail features give the same bits through it and with
    it switched off, and the flag says which ran; features with a live tail run the full stem."""
    enc = build(T, 384, 512, "bf16")
    x = T.from_numpy(constant_tail(3, 512)).cuda()
    with T.no_grad():
        a = enc(x).last_hidden_state.clone()
        assert enc.stem_shortcut_flags(3) == (1, -1)
        la = enc.last_token(x).clone()
        enc.set_stem_shortcut(False)
        b = enc(x).last_hidden_state
        assert enc.stem_shortcut_flags(3) == (-1, -1)
        assert T.equal(a, b) and T.equal(la, enc.last_token(x))
        enc.set_stem_shortcut(True)
        enc(T.from_numpy(features(12, 3, 512)).cuda())
        assert enc.stem_shortcut_flags(3) == (0, -1)


@pytest.mark.parametrize("Tn", [128, 500])
def test_below_t_in_1024_the_full_stem_runs(T, gww, Tn):
    enc = build(T, 384, Tn, "bf16")
    x = T.from_numpy(constant_tail(2, Tn, live=40)).cuda()
    with T.no_grad():
        a = enc(x).last_hidden_state.clone()
        assert enc.stem_shortcut_flags(2) == (-1, -1)            # does not apply: no detection, the full stem
        enc.set_stem_shortcut(False)
        assert T.equal(a, enc(x).last_hidden_state)


# ---------------------------------------------------------------------------------------------------- training
def _adapted(T, d, Tn, precision, sd):
    from gw_whisper_amd.peft import LoraConfig, get_peft_model
    dd, L, H, F = WIDTHS[d]
    enc = build(T, d, Tn, precision, sd=sd).cpu()
    targets = [f"layers.{i}.self_attn.{p}" for i in range(L) for p in ("q_proj", "k_proj", "v_proj", "out_proj")]
    peft = get_peft_model(enc, LoraConfig(use_dora=True, r=8, lora_alpha=32, target_modules=targets)).cuda()
    theta = {}
    with T.no_grad():
        for j, name in enumerate(targets):
            lin = peft.base_model.model.get_submodule(name)
            A, Bm, m = synth.dora_adapter(dd, dd, 8, sd[name + ".weight"], seed=70 + j)
            lin.lora_A["default"].weight.copy_(T.from_numpy(A))
            lin.lora_B["default"].weight.copy_(T.from_numpy(Bm))
            lin.lora_magnitude_vector["default"].weight.copy_(T.from_numpy(m))
            theta[name] = [T.from_numpy(v).double().requires_grad_(True) for v in (A, Bm, m)]
    return peft, theta, targets


def _dora_step(T, d, Tn, mode, precision):
    """One DoRA step (r 8, alpha 32, q / k / v / out_proj of both layers) against fp64 autograd: (worst per-tensor
    relative Frobenius errors [(rel, name)], d_mel's or None)."""
    dd, L, H, F = WIDTHS[d]
    sd = weights(d, Tn, seed=3)
    peft, theta, targets = _adapted(T, d, Tn, precision, sd)
    mel = features(33, 2, Tn)
    wl = np.random.default_rng(7).standard_normal((2, dd))
    want_mel = mode == "hidden"
    mel_t = T.from_numpy(mel).cuda().requires_grad_(want_mel)
    out = peft(mel_t).last_hidden_state[:, -1, :] if mode == "hidden" else peft.last_token(mel_t)
    (out * T.from_numpy(wl).cuda().float()).sum().backward()
    mel64 = T.from_numpy(mel).double().requires_grad_(want_mel)
    (dora64(T, sd, theta, mel64, (dd, L, H), 4.0)[:, -1, :] * T.from_numpy(wl)).sum().backward()
    worst = []
    for name in targets:
        lin = peft.base_model.model.get_submodule(name)
        got = [lin.lora_A["default"].weight.grad, lin.lora_B["default"].weight.grad,
               lin.lora_magnitude_vector["default"].weight.grad]
        for part, g_, r_ in zip("ABm", got, theta[name]):
            g_ = g_.double().cpu()
            assert T.isfinite(g_).all(), (name, part)
            worst.append((float(T.linalg.norm(g_ - r_.grad) / (T.linalg.norm(r_.grad) + 1e-30)), f"{name}.{part}"))
    worst.sort(reverse=True)
    assert all(p.grad is None for n, p in peft.named_parameters() if "lora_" not in n)
    rel_mel = float(T.linalg.norm(mel_t.grad.double().cpu() - mel64.grad) / T.linalg.norm(mel64.grad)) if want_mel else None
    print(f"d {d} T {Tn} {mode} {precision}: worst {[(round(r, 5), n) for r, n in worst[:3]]}  d_mel {rel_mel}")
    return worst, rel_mel


@pytest.mark.parametrize("mode", ["hidden", "last_token"])
@pytest.mark.parametrize("Tn", [50, 100])
@pytest.mark.parametrize("d", [128, 384])
def test_dora_step_matches_fp64_autograd(T, gww, d, Tn, mode):
    """The criterion of test_gpu_backward_widths.py: 3 % relative Frobenius error per tensor, 5 % for the q / k adapters,
    d_mel within 3 %."""
    worst, rel_mel = _dora_step(T, d, Tn, mode, "bf16")
    for rel, name in worst:
        assert rel <= (0.05 if ("q_proj" in name or "k_proj" in name) else 0.03), (name, rel)
    assert rel_mel is None or rel_mel <= 0.03


def test_fp32_training_step_at_t100(T, gww):
    """precision='fp32' at T = 100 under test_gpu_train_fp32.py's BOUND (1e-4 per tensor, d_mel included)."""
    from tests.test_gpu_train_fp32 import BOUND
    for mode in ("hidden", "last_token"):
        worst, rel_mel = _dora_step(T, 128, 100, mode, "fp32")
        assert worst[0][0] <= BOUND, worst[:3]
        assert rel_mel is None or rel_mel <= BOUND


def test_full_finetune_step_at_t100(T, gww):
    """Every base gradient of the fused-route width at T = 100 against fp64 autograd, under the criterion of
    test_gpu_full_finetune.py::test_every_base_gradient_matches_fp64_autograd (3 %, 5 % for q_proj / k_proj, d_mel 3 %)."""
    dd, L, H, F = WIDTHS[384]
    sd = weights(384, 100, seed=3)
    enc = build(T, 384, 100, "bf16", sd=sd)
    enc.enable_full_finetune()
    for p in enc.parameters():
        p.requires_grad = True
    mel = features(33, 2, 100)
    wl = np.random.default_rng(7).standard_normal((2, dd))
    mel_t = T.from_numpy(mel).cuda().requires_grad_(True)
    (enc(mel_t).last_hidden_state[:, -1, :] * T.from_numpy(wl).cuda().float()).sum().backward()
    p64 = {k: T.from_numpy(v).double().requires_grad_(True) for k, v in sd.items()}
    mel64 = T.from_numpy(mel).double().requires_grad_(True)
    (encoder64(T, p64, mel64, (dd, L, H))[:, -1, :] * T.from_numpy(wl)).sum().backward()
    worst = []
    for n, p in enc.named_parameters():
        got = p.grad.double().cpu()
        assert T.isfinite(got).all(), n
        worst.append((float(T.linalg.norm(got - p64[n].grad) / (T.linalg.norm(p64[n].grad) + 1e-30)), n))
    worst.sort(reverse=True)
    print("full fine-tune T 100 worst:", [(round(r, 4), n) for r, n in worst[:5]])
    for rel, n in worst:
        assert rel <= (0.05 if ("q_proj" in n or "k_proj" in n) else 0.03), (n, rel)
    assert float(T.linalg.norm(mel_t.grad.double().cpu() - mel64.grad) / T.linalg.norm(mel64.grad)) <= 0.03


# ---------------------------------------------------------------------------------------------------- end to end
def _logit(p):
    p = np.asarray(p, np.float64)
    return np.log(p) - np.log1p(-p)


def test_run_train_and_evaluation_with_a_configured_front_end(T, gww, tmp_path):
    """run_train.py on 2 s chunks at 2048 Hz (n_fft 128, hop 16, mel band to 1024 Hz: T = 128) with the micro encoder for
    two epochs: finite losses and both configuration files beside the adapter.  Then run_evaluation.py on the saved model,
    which learns the front end and the context from those two files alone, against the validation logits computed HERE from
    the saved weights with the configuration written out by hand (``ops.logmel(config=...)`` + an encoder of
    ``max_source_positions`` 128), per logit:
      * all 64 segments in run_evaluation's own batching: the same kernels in the same launch geometry on the same numbers,
        so what is left is fp32 rounding of the score (sigmoid and back), 1e-5 -- the figure this file holds equal fp32
        launches to;
      * the 13 validation segments in the trainer's batching (one batch of 13 against one of 64): the forward bound of another
        launch geometry, 0.06 per logit (test_a_segment_does_not_depend_on_its_batch);
      * the trainer's logged validation loss is the mean BCE of those 13 logits: BCE is 1-Lipschitz in the logit, so the
        same 0.06 ties the logits computed here to the trainer's.
    The evaluation's log line must name T = 128 and the 2048 Hz extractor.  (Measured on one MI355X: 5.9e-8 and 9.7e-8
    per logit, the two losses equal to six digits; the logits span -0.059 .. -0.001, and a front end that ignored the saved
    band -- the 8000 Hz one, printed below -- lands 3.7e-2 away, so it is the first bound that tells the two apart.)"""
    import dataclasses
    import importlib.util
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = str(tmp_path)
    fe = ["--sampling-rate", "2048", "--n-fft", "128", "--hop-length", "16", "--chunk-length", "2", "--mel-fmax", "1024"]
    r = subprocess.run([sys.executable, os.path.join(root, "harness", "run_train.py"), "--synthetic", "64", "--encoder", "micro",
                        "--num-epochs", "2", "--models-path", out + "/m", "--log-dir", out + "/l", *fe],
                       capture_output=True, text=True, timeout=600, cwd=root)
    assert r.returncode == 0, r.stdout + r.stderr
    log = [json.loads(l) for l in open(out + "/l/train_log.jsonl")]
    assert len(log) == 2 and all(np.isfinite(e["train_loss"]) and np.isfinite(e["val_loss"]) for e in log)
    adapter = out + "/m/lora_weights_8_32"
    assert sorted(os.listdir(adapter)) == ["adapter_config.json", "adapter_model.safetensors", "config.json",
                                           "preprocessor_config.json"]
    with open(adapter + "/config.json") as f:
        assert json.load(f)["max_source_positions"] == 128
    with open(adapter + "/preprocessor_config.json") as f:
        pre = json.load(f)
    assert (pre["sampling_rate"], pre["n_fft"], pre["hop_length"], pre["chunk_length"], pre["max_frequency"]) == \
        (2048, 128, 16, 2, 1024.0)
    r = subprocess.run([sys.executable, os.path.join(root, "harness", "run_evaluation.py"), "--synthetic", "64", "--model_type",
                        "2D", "--num_bootstrap", "5", "--encoder", "micro", "--out_dir", out + "/e", "--lora_weights_path",
                        adapter, "--dense_layers_path", out + "/m/dense_layers_8_32.pth"],
                       capture_output=True, text=True, timeout=600, cwd=root)
    assert r.returncode == 0, r.stdout + r.stderr
    z = np.load(out + "/e/ROC_curve_SNR_0_2D.npz")
    assert z["all_raw_preds"].shape == (64,) and np.isfinite(z["all_raw_preds"]).all()
    rec = [json.loads(l) for l in open(out + "/e/eval_log.jsonl")]
    assert len(rec) == 1
    assert (rec[0]["max_source_positions"], rec[0]["sampling_rate"], rec[0]["n_fft"], rec[0]["hop_length"], rec[0]["n_frames"],
            rec[0]["max_frequency"]) == (128, 2048, 128, 16, 256, 1024.0)

    # the saved model rebuilt here; nothing below reads preprocessor_config.json or config.json
    from gw_whisper_amd import ops
    from gw_whisper_amd.encoder import WhisperConfig, WhisperEncoder
    from gw_whisper_amd.models import two_channel_ligo_binary_classifier
    from gw_whisper_amd.peft import PeftModel
    spec = importlib.util.spec_from_file_location("_harness_run_train", os.path.join(root, "harness", "run_train.py"))
    run_train = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(run_train)
    h1, l1, labels, _ = run_train.synthetic_dataset(64, 42, 2048)
    assert np.array_equal(labels, z["all_labels"])
    d, L, H, F = synth.ENCODER_SIZES["micro"]
    enc = WhisperEncoder(dataclasses.replace(WhisperConfig.named("micro"), max_source_positions=128), precision="bf16")
    enc.load_state_dict({k: T.from_numpy(v) for k, v in synth.encoder_state_dict(d, L, H, F, seed=42, n_mels=80).items()})
    model = two_channel_ligo_binary_classifier(PeftModel.from_pretrained(enc, adapter).cuda(), num_classes=1).cuda()
    model.classifier.load_state_dict(T.load(out + "/m/dense_layers_8_32.pth", map_location="cuda"))
    model.eval()

    def logits(idx, config):
        with T.no_grad():
            mel = ops.logmel(T.from_numpy(np.concatenate((h1[idx], l1[idx]))).cuda(), n_mels=80, config=config)
            assert mel.shape == (2 * len(idx), 80, 256)
            return model(mel[:len(idx)], mel[len(idx):]).double().reshape(-1).cpu().numpy()

    cfg = ops.FrontendConfig(80, 2048, 128, 16, 2 * 2048, 0.0, 1024.0)
    val_idx = np.random.default_rng(42).permutation(64)[:int(round(64 * 0.2))]      # run_train.py's split, seed 42
    got = _logit(z["all_raw_preds"])
    ref_all, ref_val = logits(np.arange(64), cfg), logits(val_idx, cfg)
    e_all, e_val = np.abs(got - ref_all), np.abs(got[val_idx] - ref_val)
    y = labels[val_idx].astype(np.float64)
    bce = float(np.mean(np.logaddexp(0.0, ref_val) - y * ref_val))
    # how far a front end that ignores the saved files lands: HF's 8000 Hz band at this rate (printed, not asserted)
    wrong = np.abs(got - logits(np.arange(64), ops.FrontendConfig(80, 2048, 128, 16, 2 * 2048, 0.0, 8000.0)))
    print(f"logits: spread (std) {ref_all.std():.3e}, range {ref_all.min():.4f} .. {ref_all.max():.4f}; run_evaluation vs rebuilt: "
          f"same batching max {e_all.max():.3e}, trainer's batching max {e_val.max():.3e}; with the 8000 Hz band max "
          f"{wrong.max():.3e}; trainer val_loss {log[-1]['val_loss']:.6f}, from the rebuilt logits {bce:.6f}")
    assert e_all.max() <= 1e-5
    assert e_val.max() <= 0.06
    assert abs(bce - log[-1]["val_loss"]) <= 0.06
