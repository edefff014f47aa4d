"""Step level: the gradients of a batch are the sum of the gradients of its segments.  The kernel tests of
tests/test_gpu_backward_exact.py cannot see the driver in encoder_train.hip -- the ``rows`` it passes to the reductions, the
junk rows of the conv im2col views, the pooled / sparse-dctx path of ``last_token``.  A fixed linear loss on a batch of two
different segments is run through the backward, then on each segment alone (M = 128 token rows against 64):
  1. the forward outputs and d_mel of the batch equal those of the single runs bit for bit (the kernels are
     row-independent);
  2. for every parameter tensor ||g(batch) - (g(seg0) + g(seg1))||_F <= 2e-3 ||g(batch)||_F, the sum formed in fp64.  With
     128 token rows one lost or doubled row moves a weight gradient by about 1 / sqrt(128) = 9e-2 of its norm; the bound is
     a fortieth of that, and the only legitimate difference is fp32 reassociation.
Micro (d 128) and tiny-width (d 384) encoders cut to a context of 64, full fine-tuning and DoRA on q / k / v / out_proj,
``hidden`` and ``last_token``.  Measured on one MI355X: forward and d_mel bit-identical in all eight cases, worst residual
1.34e-7 (``layer_norm.bias``, micro, full, hidden): profiles/backward_exact.md.  Needs an MI355X."""

import numpy as np
import pytest

from gw_whisper_amd import synth

pytestmark = pytest.mark.gpu

WIDTHS = {128: synth.ENCODER_SIZES["micro"], 384: (384, 2, 6, 1536)}
CONTEXT = 64
BOUND = 2e-3


@pytest.fixture(scope="module")
def T():
    import torch
    assert torch.cuda.is_available()
    return torch


def _features(seed, B):
    """Two different segments of log-mel-like features [B, 80, 2 T]."""
    return np.clip(np.random.default_rng(seed).standard_normal((B, 80, 2 * CONTEXT)) * 0.5, -1.5, 1.5).astype(np.float32)


def _model(T, d, method, precision):
    """(module to call, {name: trainable parameter})."""
    from gw_whisper_amd.encoder import WhisperConfig, WhisperEncoder
    from gw_whisper_amd.peft import LoraConfig, get_peft_model
    dd, L, H, F = WIDTHS[d]
    sd = synth.encoder_state_dict(dd, L, H, F, seed=3)
    enc = WhisperEncoder.from_numpy_state_dict(sd, WhisperConfig(dd, L, H, F), precision=precision).with_context(CONTEXT)
    if method == "full":
        enc = enc.cuda()
        enc.enable_full_finetune()
        for p in enc.parameters():
            p.requires_grad = True
        return enc, dict(enc.named_parameters())
    targets = [f"layers.{i}.self_attn.{p}" for i in range(L) for p in ("q_proj", "k_proj", "v_proj", "out_proj")]
    peft = get_peft_model(enc, LoraConfig(use_dora=True, r=8, lora_alpha=32, target_modules=targets)).cuda()
    with T.no_grad():
        for j, name in enumerate(targets):
            lin = peft.base_model.model.get_submodule(name)
            A, Bm, m = synth.dora_adapter(dd, dd, 8, sd[name + ".weight"], seed=70 + j)
            lin.lora_A["default"].weight.copy_(T.from_numpy(A))
            lin.lora_B["default"].weight.copy_(T.from_numpy(Bm))
            lin.lora_magnitude_vector["default"].weight.copy_(T.from_numpy(m))
    return peft, {n: p for n, p in peft.named_parameters() if "lora_" in n}


def _step(T, model, params, mel, wl, mode):
    """(forward output, d_mel or None, {name: fp64 gradient}) of sum(out * wl)."""
    for p in params.values():
        p.grad = None
    want_mel = mode == "hidden"
    mel_t = mel.clone().requires_grad_(want_mel)
    out = model(mel_t).last_hidden_state if mode == "hidden" else model.last_token(mel_t)
    (out * wl).sum().backward()
    T.cuda.synchronize()
    return (out.detach().clone(), mel_t.grad.detach().clone() if want_mel else None,
            {n: p.grad.detach().double().cpu() for n, p in params.items()})


def _additivity(T, d, method, mode, precision):
    """(forward and d_mel bit-identical?, [(residual, name)] worst first)."""
    model, params = _model(T, d, method, precision)
    mel = T.from_numpy(_features(33, 2)).cuda()
    dd = WIDTHS[d][0]
    rng = np.random.default_rng(7)
    wl = T.from_numpy(rng.standard_normal((CONTEXT, dd) if mode == "hidden" else (dd,)).astype(np.float32)).cuda()
    out_b, dmel_b, g_b = _step(T, model, params, mel, wl, mode)
    same, g_sum = True, None
    for i in range(2):
        out_i, dmel_i, g_i = _step(T, model, params, mel[i:i + 1], wl, mode)
        same = same and T.equal(out_i[0], out_b[i]) and (dmel_b is None or T.equal(dmel_i[0], dmel_b[i]))
        g_sum = g_i if g_sum is None else {n: g_sum[n] + g_i[n] for n in g_sum}
    res = []
    for n, g in g_b.items():
        assert T.isfinite(g).all() and float(T.linalg.norm(g)) > 0, n
        res.append((float(T.linalg.norm(g - g_sum[n]) / T.linalg.norm(g)), n))
    res.sort(reverse=True)
    print(f"d {d} {method} {mode} {precision}: forward / d_mel bit-identical {same}; worst additivity residuals "
          f"{[(f'{r:.2e}', n) for r, n in res[:3]]}")
    return same, res


@pytest.mark.parametrize("mode", ["hidden", "last_token"])
@pytest.mark.parametrize("method", ["full", "dora"])
@pytest.mark.parametrize("d", sorted(WIDTHS))
def test_gradients_add_over_segments(T, gww, d, method, mode):
    same, res = _additivity(T, d, method, mode, "bf16")
    assert same, "the forward output or d_mel of a segment depends on its batch"
    assert res[0][0] <= BOUND, res[:5]
