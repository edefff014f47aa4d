"""Per-layer outputs of the HIP encoder (``output_hidden_states`` / ``output_attentions``, gww_encoder_forward_outputs
and the attention-probability kernel attention_probs.hip) against HF's eager encoder, against float64 layers built
from the encoder's own weights, and against the plain forward bit for bit.  Needs an MI355X."""

import numpy as np
import pytest

from gw_whisper_amd import synth

pytestmark = pytest.mark.gpu

# Bounds.  fp32 is the parity path: f32-input MFMA scores, expf softmax.  bf16: the scores come from the bf16 q / k
# the forward feeds its own attention (8 mantissa bits: a relative error of up to 2^-9 in each operand, i.e. an absolute
# score error of ~|s| 2^-8, and a probability error of about p times that), and every layer GEMM rounds its operands
# to bf16 the same way, so the residual stream after a layer is off by a few 1e-3 of its scale.
# Measured maxima on an MI355X (-s prints them), and the bounds (about 3x to 40x above them):
#   HF golden, fp32: hidden 1.3e-6 relative, attention 2.6e-8      -> 1e-5, 1e-6
#   HF golden, bf16: hidden 3.6e-3 relative, attention 1.4e-4      -> 1e-2, 1e-3
#   fp64 layers, fp32: hidden 1.5e-6 relative, attention 9.6e-8    -> 1e-5, 1e-6
#   fp64 layers, bf16: hidden 3.3e-3 relative, attention 4.0e-4    -> 1e-2, 2e-3
#   fp64 layers at d 1280, H 20 (two layers, B 1), fp32: hidden 2.0e-6 relative, attention 1.7e-7  -> the same 1e-5, 1e-6
#   fp64 layers at d 1280, H 20 (two layers, B 1), bf16: hidden 3.2e-3 relative, attention 4.8e-4  -> the same 1e-2, 2e-3
# The absolute attention bounds are loose against a typical entry of 5e-4: tests/test_gpu_attention_maps.py holds the
# map kernel itself to a relative bound per entry.
HF_HID_F32, HF_ATT_F32 = 1e-5, 1e-6
HF_HID_BF16, HF_ATT_BF16 = 1e-2, 1e-3
FP64_HID = {"fp32": 1e-5, "bf16": 1e-2}
FP64_ATT = {"fp32": 1e-6, "bf16": 2e-3}


@pytest.fixture(scope="module")
def T():
    import torch
    assert torch.cuda.is_available()
    return torch


def _features(seed, batch=2):
    """tools/make_golden_outputs.py input_features(): seeded stand-in for normalised log-mel features."""
    rng = np.random.default_rng(seed)
    return np.clip(rng.standard_normal((batch, 80, 3000)) * 0.5, -1.5, 1.5).astype(np.float32)


def _enc(T, d, L, H, F, seed, precision):
    from gw_whisper_amd.encoder import WhisperConfig, WhisperEncoder
    sd = synth.encoder_state_dict(int(d), int(L), int(H), int(F), seed=int(seed))
    enc = WhisperEncoder.from_numpy_state_dict(sd, WhisperConfig(int(d), int(L), int(H), int(F)), precision=precision)
    return enc.cuda(), sd


def _p64(T, sd):
    return {k: T.from_numpy(v).cuda().double() for k, v in sd.items()}


def _attn64(T, p, i, x, H):
    """HF eager attention weights of layer i on its input x (float64): softmax(q k^T) with q = (LN1(x) Wq^T + bq) / 8."""
    F_ = T.nn.functional
    g = lambda n: p[f"layers.{i}.{n}"]
    B, Tn, d = x.shape
    h = F_.layer_norm(x, (d,), g("self_attn_layer_norm.weight"), g("self_attn_layer_norm.bias"), 1e-5)
    sh = lambda t: t.view(B, Tn, H, d // H).transpose(1, 2)
    q = sh((h @ g("self_attn.q_proj.weight").t() + g("self_attn.q_proj.bias")) * 0.125)
    k = sh(h @ g("self_attn.k_proj.weight").t())
    return T.softmax(q @ k.transpose(-1, -2), dim=-1), h


def _layer64(T, p, i, x, H, final=False):
    """One HF encoder layer in float64 on x [B, T, d]; (x_next, attention weights).  final: + the encoder's LayerNorm."""
    F_ = T.nn.functional
    g = lambda n: p[f"layers.{i}.{n}"]
    B, Tn, d = x.shape
    P, h = _attn64(T, p, i, x, H)
    v = (h @ g("self_attn.v_proj.weight").t() + g("self_attn.v_proj.bias")).view(B, Tn, H, d // H).transpose(1, 2)
    a = (P @ v).transpose(1, 2).reshape(B, Tn, d)
    x = x + a @ g("self_attn.out_proj.weight").t() + g("self_attn.out_proj.bias")
    h = F_.layer_norm(x, (d,), g("final_layer_norm.weight"), g("final_layer_norm.bias"), 1e-5)
    x = x + F_.gelu(h @ g("fc1.weight").t() + g("fc1.bias")) @ g("fc2.weight").t() + g("fc2.bias")
    if final:
        x = F_.layer_norm(x, (d,), p["layer_norm.weight"], p["layer_norm.bias"], 1e-5)
    return x, P


def _check_rows(T, at):
    """every probability >= 0, every row sums to 1 within 1e-5"""
    assert float(at.min()) >= 0.0
    err = float((at.double().sum(-1) - 1.0).abs().max())
    assert err < 1e-5, err


# ---------------------------------------------------------------------------------------------- 1. HF golden
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("name", ["tiny", "base"])
def test_outputs_match_hf_golden(T, gww, golden, name, precision):
    """Reduced 2-layer encoders at tiny geometry (the fused whisper-tiny path in bf16) and base geometry (generic path)
    against HF's eager WhisperEncoder (tools/make_golden_outputs.py): hidden states at the golden rows relative to each
    tensor's max |x|, attention rows (batch item 0, every head, 4 query rows, all 1500 keys) absolute."""
    g = golden("encoder_outputs.npz")
    d, L, H, F, wseed, iseed = (int(v) for v in g[f"{name}_config"])
    enc, _ = _enc(T, d, L, H, F, wseed, precision)
    mel = T.from_numpy(_features(iseed)).cuda()
    with T.no_grad():
        o = enc(mel, output_hidden_states=True, output_attentions=True)
    assert len(o.hidden_states) == L + 1 and len(o.attentions) == L
    rows, qrows = g["rows"], g["qrows"]
    eh = []
    for i in range(L + 1):
        ref = g[f"{name}_hidden{i}"]
        eh.append(float(np.abs(o.hidden_states[i][:, rows].cpu().numpy() - ref).max() / np.abs(ref).max()))
    ea = [float(np.abs(o.attentions[l][0][:, qrows].cpu().numpy() - g[f"{name}_attn{l}"]).max()) for l in range(L)]
    print(f"{name} {precision}: hidden rel {['%.2e' % e for e in eh]}  attn abs {['%.2e' % e for e in ea]}")
    th, ta = (HF_HID_F32, HF_ATT_F32) if precision == "fp32" else (HF_HID_BF16, HF_ATT_BF16)
    assert max(eh) < th and max(ea) < ta


# ------------------------------------------------------------------------------------ 2. full geometry vs fp64
# the two-layer cut of whisper-large's width: 20 heads, i.e. a 3840-element qkv row and, in the attention slab, a second
# layer that starts 20 maps in
WIDE2 = (1280, 2, 20, 5120)


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("name", ["tiny", "base", "wide2"])
def test_full_geometry_against_fp64(T, gww, name, precision):
    """whisper-tiny (fused path in bf16) and whisper-base (generic path), B = 3, and two layers at whisper-large's width
    (H = 20), B = 1: attentions[l] against the float64 softmax of LN1(hidden_states[l])'s q . k, hidden_states[l + 1]
    against a float64 layer applied to hidden_states[l] (relative to its max |x|; the last one with the final
    LayerNorm), and every map row a distribution."""
    d, L, H, F = WIDE2 if name == "wide2" else synth.ENCODER_SIZES[name]
    B = 1 if name == "wide2" else 3
    enc, sd = _enc(T, d, L, H, F, 5, precision)
    p = _p64(T, sd)
    mel = T.from_numpy(_features(41, B)).cuda()
    with T.no_grad():
        o = enc(mel, output_hidden_states=True, output_attentions=True)
        ea, eh = [], []
        for l in range(L):
            assert o.attentions[l].shape == (B, H, 1500, 1500) and o.attentions[l].dtype == T.float32
            assert o.hidden_states[l].shape == (B, 1500, d) and o.hidden_states[l].dtype == T.float32
            xn, P = _layer64(T, p, l, o.hidden_states[l].double(), H, final=(l == L - 1))
            ea.append(float((o.attentions[l].double() - P).abs().max()))
            eh.append(float((o.hidden_states[l + 1].double() - xn).abs().max() / xn.abs().max()))
            del P, xn
            _check_rows(T, o.attentions[l])
    print(f"{name} {precision} vs fp64: attn abs {['%.2e' % e for e in ea]}  hidden rel {['%.2e' % e for e in eh]}")
    assert max(ea) < FP64_ATT[precision] and max(eh) < FP64_HID[precision]


# ------------------------------------------------------------------------------------------- 3. bit identity
@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_last_hidden_state_bit_identical(T, gww, precision, split):
    """With both outputs requested, last_hidden_state equals the plain forward's bit for bit (the new entry only adds
    stores and launches).  B = 64: the smallest batch the split engages at (two halves of kSplitMin = 32)."""
    d, L, H, F = synth.ENCODER_SIZES["tiny"]
    enc, _ = _enc(T, d, L, H, F, 7, precision)
    enc.set_split(split)
    mel = T.from_numpy(_features(43, 64)).cuda()
    with T.no_grad():
        plain = enc(mel).last_hidden_state
        o = enc(mel, output_hidden_states=True, output_attentions=True)
        assert T.equal(o.last_hidden_state, plain)
        assert o.hidden_states[-1] is o.last_hidden_state
        del o
        a = enc(mel, output_attentions=True)
        assert a.hidden_states is None and T.equal(a.last_hidden_state, plain)
        del a
        h = enc(mel, output_hidden_states=True)
        assert h.attentions is None and T.equal(h.last_hidden_state, plain)


def test_split_equals_unsplit_for_every_output(T, gww):
    """whisper-tiny, bf16, B = 65 (odd: halves of 32 and 33): split on and off give the same bits in every output."""
    d, L, H, F = synth.ENCODER_SIZES["tiny"]
    enc, _ = _enc(T, d, L, H, F, 7, "bf16")
    mel = T.from_numpy(_features(47, 65)).cuda()
    with T.no_grad():
        enc.set_split(False)
        a = enc(mel, output_hidden_states=True, output_attentions=True)
        enc.set_split(True)
        b = enc(mel, output_hidden_states=True, output_attentions=True)
        assert T.equal(a.last_hidden_state, b.last_hidden_state)
        for x, y in zip(a.hidden_states, b.hidden_states):
            assert T.equal(x, y)
        for x, y in zip(a.attentions, b.attentions):
            assert T.equal(x, y)


@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_repeated_calls_identical(T, gww, precision):
    d, L, H, F = synth.ENCODER_SIZES["tiny"]
    enc, _ = _enc(T, d, L, H, F, 7, precision)
    mel = T.from_numpy(_features(53, 3)).cuda()
    with T.no_grad():
        a = enc(mel, output_hidden_states=True, output_attentions=True)
        b = enc(mel, output_hidden_states=True, output_attentions=True)
    for x, y in zip(a.to_tuple()[1] + a.to_tuple()[2], b.to_tuple()[1] + b.to_tuple()[2]):
        assert T.equal(x, y)


# ----------------------------------------------------------------------------------------------------- 4. API
def test_return_dict_false_is_hf_tuple(T, gww):
    """HF's encoder returns tuple(v for v in (last_hidden_state, hidden_states, attentions) if v is not None)."""
    d, L, H, F = synth.ENCODER_SIZES["micro"]
    enc, _ = _enc(T, d, L, H, F, 3, "fp32")
    mel = T.from_numpy(_features(59, 2)).cuda()
    with T.no_grad():
        ref = enc(mel, output_hidden_states=True, output_attentions=True)
        t = enc(mel, output_hidden_states=True, output_attentions=True, return_dict=False)
        assert isinstance(t, tuple) and len(t) == 3
        assert t[0].shape == (2, 1500, d) and T.equal(t[0], ref.last_hidden_state)
        assert isinstance(t[1], tuple) and len(t[1]) == L + 1 and all(x.shape == (2, 1500, d) for x in t[1])
        assert isinstance(t[2], tuple) and len(t[2]) == L and all(x.shape == (2, H, 1500, 1500) for x in t[2])
        assert t[1][-1] is t[0]
        t = enc(mel, output_attentions=True, return_dict=False)
        assert len(t) == 2 and len(t[1]) == L and t[1][0].shape == (2, H, 1500, 1500)
        t = enc(mel, output_hidden_states=True, return_dict=False)
        assert len(t) == 2 and len(t[1]) == L + 1
        t = enc(mel, return_dict=False)
        assert len(t) == 1 and T.equal(t[0], ref.last_hidden_state)
        assert ref[0] is ref.last_hidden_state


def test_config_defaults_are_honoured(T, gww):
    d, L, H, F = synth.ENCODER_SIZES["micro"]
    enc, _ = _enc(T, d, L, H, F, 3, "fp32")
    mel = T.from_numpy(_features(59, 1)).cuda()
    with T.no_grad():
        o = enc(mel)
        assert o.hidden_states is None and o.attentions is None
        enc.config.output_hidden_states = True
        enc.config.output_attentions = True
        o = enc(mel)
        assert len(o.hidden_states) == L + 1 and len(o.attentions) == L
        o = enc(mel, output_attentions=False)
        assert o.attentions is None and len(o.hidden_states) == L + 1
        enc.config.return_dict = False
        t = enc(mel)
        assert isinstance(t, tuple) and len(t) == 3
        assert not isinstance(enc(mel, return_dict=True), tuple)


def test_dora_peft_model_passes_flags_and_maps_use_merged_weights(T, gww):
    """get_peft_model(use_dora=True) on q_proj / k_proj with non-trivial A, B, m: the flags pass through PeftModel and
    the maps are the float64 softmax built from the merged weights (fp32 parity path)."""
    from gw_whisper_amd.peft import LoraConfig, get_peft_model
    from oracle import dora as odora
    d, L, H, F = synth.ENCODER_SIZES["micro"]
    enc, sd = _enc(T, d, L, H, F, 3, "fp32")
    targets = [f"layers.{i}.self_attn.{p}" for i in range(L) for p in ("q_proj", "k_proj")]
    peft = get_peft_model(enc, LoraConfig(use_dora=True, r=8, lora_alpha=32, target_modules=targets)).cuda()
    sd2 = dict(sd)
    with T.no_grad():
        for j, name in enumerate(targets):
            lin = peft.base_model.model.get_submodule(name)
            W0 = sd[name + ".weight"]
            A, B, m = synth.dora_adapter(d, d, 8, W0, seed=70 + j)
            lin.lora_A["default"].weight.copy_(T.from_numpy(A))
            lin.lora_B["default"].weight.copy_(T.from_numpy(B))
            lin.lora_magnitude_vector["default"].weight.copy_(T.from_numpy(m))
            sd2[name + ".weight"] = odora.dora_merge(W0.astype(np.float64), A.astype(np.float64), B.astype(np.float64),
                                                     m.astype(np.float64), 4.0)
        mel = T.from_numpy(_features(61, 2)).cuda()
        o = peft(mel, output_hidden_states=True, output_attentions=True)
        p2, p0 = _p64(T, sd2), _p64(T, sd)
        for l in range(L):
            P, _ = _attn64(T, p2, l, o.hidden_states[l].double(), H)
            P0, _ = _attn64(T, p0, l, o.hidden_states[l].double(), H)
            assert float((P - P0).abs().max()) > 1e-3, "the adapter must actually change the maps"
            err = float((o.attentions[l].double() - P).abs().max())
            assert err < 1e-5, err


def test_flags_under_autograd_with_trainable_adapters_raise(T, gww):
    from gw_whisper_amd import GwwError
    from gw_whisper_amd.peft import LoraConfig, get_peft_model
    d, L, H, F = synth.ENCODER_SIZES["micro"]
    enc, _ = _enc(T, d, L, H, F, 3, "bf16")
    targets = [f"layers.{i}.self_attn.{p}" for i in range(L) for p in ("q_proj", "v_proj")]
    peft = get_peft_model(enc, LoraConfig(use_dora=True, r=8, lora_alpha=32, target_modules=targets)).cuda()
    mel = T.from_numpy(_features(67, 1)).cuda()
    for kw in ({"output_hidden_states": True}, {"output_attentions": True}):
        with pytest.raises(GwwError, match="inference only"):
            peft(mel, **kw)
    with T.no_grad():
        o = peft(mel, output_attentions=True)
    assert len(o.attentions) == L


@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_batch_one_and_odd_batch(T, gww, precision):
    """B = 1 and B = 5: item 0 of the batch of 5 against the batch of 1, and every map row a distribution."""
    d, L, H, F = synth.ENCODER_SIZES["tiny"]
    enc, _ = _enc(T, d, L, H, F, 9, precision)
    mel = T.from_numpy(_features(71, 5)).cuda()
    with T.no_grad():
        a = enc(mel[:1], output_hidden_states=True, output_attentions=True)
        b = enc(mel, output_hidden_states=True, output_attentions=True)
    assert a.attentions[0].shape == (1, H, 1500, 1500) and b.attentions[0].shape == (5, H, 1500, 1500)
    tol = 1e-5 if precision == "fp32" else 1e-2
    for x, y in zip(a.hidden_states, b.hidden_states):
        assert float((x[0] - y[0]).abs().max() / y[0].abs().max()) < tol
    for x, y in zip(a.attentions, b.attentions):
        assert float((x[0] - y[0]).abs().max()) < tol
        _check_rows(T, y)
