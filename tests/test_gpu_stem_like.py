"""The conv-stem backward per element on impulse gradients: k_stem_dz2 / k_stem_dz1 / k_stem_dmel
and their _f32 twins, the transposed-panel GEMMs and weight-gradient calls of Step::stem_backward, and k_pos_grad, against
the fp64 derivative of gelu(conv2(gelu(conv1(mel)))) contracted with the device's own d_x0.  A one-layer encoder with
zero out_proj and fc2 is the identity above the stem, so a d_hidden that is live at chosen (segment, token) pairs is an
impulse into the stem and nothing above it enters the comparison.  Bound per element: c S (the conv gradients: c S + E),
exactly zero where S = 0
(tests/stem_like.py; c is measured on the CPU by tests/test_stem_like_host.py, never on the kernels).  Needs an MI355X."""

import numpy as np
import pytest

from tests import stem_like as sl

pytestmark = pytest.mark.gpu

ALL = sl.table() + [(sl.POOLED_CASE, "pooled")]
# field of gww_enc_grads -> parameter
FIELDS = {"conv1_w": "conv1.weight", "conv1_b": "conv1.bias", "conv2_w": "conv2.weight", "conv2_b": "conv2.bias",
          "pos": "embed_positions.weight"}
_ENC = {}


@pytest.fixture(scope="module")
def T():
    import torch
    assert torch.cuda.is_available()
    return torch


def _build(T, case, regime, precision):
    from gw_whisper_amd.encoder import WhisperConfig, WhisperEncoder
    d, C, Tn, B = sl.CASES[case]
    H, F = sl.WIDTHS[d]
    cfg = WhisperConfig(d, 1, H, F, num_mel_bins=C, max_source_positions=Tn)
    sd = {k: v.copy() for k, v in sl.weights(case, regime).items()}   # (the shared arrays are read-only)
    return WhisperEncoder.from_numpy_state_dict(sd, cfg, precision=precision).cuda()


def _encoder(T, case, regime, precision):
    """The frozen encoder of a case, built once."""
    key = (case, regime, precision)
    if key not in _ENC:
        _ENC[key] = _build(T, case, regime, precision)
    return _ENC[key]


def _inputs(T, case, pattern):
    mel = T.from_numpy(np.array(sl.features(case))).cuda().contiguous()
    d_hidden = T.from_numpy(sl.impulse(case, pattern)).cuda().contiguous()
    return mel, d_hidden


def _live(case, pattern):
    return sl.live_mask(case, pattern)


def _check_impulse(T, case, pattern, d_x0):
    """The precondition: d_x0 is finite, exactly zero on the dead rows and not zero on the live ones."""
    live = T.from_numpy(_live(case, pattern)).cuda()
    assert bool(T.isfinite(d_x0).all())
    assert bool((d_x0[~live] == 0).all()), "a dead row of d_x0 is not exactly zero: the encoder is not the identity above the stem"
    assert bool((d_x0[live].abs().amax(-1) > 0).all())


def _assert_within(precision, case, pattern, regime, got, x0, names):
    """got {name: tensor} against the fp64 reference built from the device's d_x0; the message names the worst element."""
    import torch
    sd, mel = sl.weights(case, regime), sl.features(case)
    g = x0.cpu().numpy()
    ref = sl.reference(torch, sd, mel, g)
    S, Sf = sl.scales(torch, sd, mel, g, precision, weight_grads=names != ("d_mel",))
    fails = []
    for name in names:
        a = got[name].double().cpu().numpy()
        r = sl.ratios(name, a, ref[name], S[name], Sf[name]).max()
        c = sl.c_bound(precision, name, case)
        print(f"{precision} case {case} {pattern} {regime} {name}: worst ratio {r:.3e} (c = {c:.3e})")
        msg = sl.compare(name, a, ref[name], S[name], Sf[name], c)
        if msg:
            fails.append(msg)
    assert not fails, f"case {case} {pattern} {regime} {precision}:\n" + "\n".join(fails)


@pytest.mark.parametrize("precision", ["bf16", "fp32"])
@pytest.mark.parametrize("regime", sl.REGIMES)
@pytest.mark.parametrize("case,pattern", ALL)
def test_d_mel_per_element(T, gww, case, pattern, regime, precision):
    """d_mel of gww_encoder_train_backward[_f32]: within c S per element, exactly zero where no term reaches, a second
    call bit-identical, and with d_x0 also requested bit-identical to the d_mel-only call."""
    enc = _encoder(T, case, regime, precision)
    mel, d_hidden = _inputs(T, case, pattern)
    pooled = pattern == "pooled"
    x0, d_mel = sl.c_step(T, enc, mel, pooled, d_hidden, True, True)
    _check_impulse(T, case, pattern, x0)
    _, only = sl.c_step(T, enc, mel, pooled, d_hidden, False, True)
    _, again = sl.c_step(T, enc, mel, pooled, d_hidden, False, True)
    assert T.equal(only, again), "d_mel differs between two calls"
    assert T.equal(only, d_mel), "d_mel differs when d_x0 is also requested"
    _assert_within(precision, case, pattern, regime, {"d_mel": d_mel}, x0, ("d_mel",))


def _zero_grads(T, case, base=None):
    d, C, Tn, B = sl.CASES[case]
    shapes = {"conv1_w": (d, C, 3), "conv1_b": (d,), "conv2_w": (d, d, 3), "conv2_b": (d,), "pos": (Tn, d)}
    if base is None:
        return {f: T.zeros(s, dtype=T.float32, device="cuda") for f, s in shapes.items()}
    rng = np.random.default_rng(base)
    return {f: T.from_numpy(rng.integers(-4, 5, s).astype(np.float32)).cuda() for f, s in shapes.items()}


@pytest.mark.parametrize("regime", sl.REGIMES)
@pytest.mark.parametrize("case,pattern", ALL)
def test_conv_and_position_gradients_per_element(T, gww, case, pattern, regime):
    """gww_encoder_train_backward_full with a gww_enc_grads that holds the stem's five tensors only: conv1 / conv2 weight
    and bias gradients and embed_positions per element; rows of dead tokens and taps that only ever see a pad row are
    exactly zero (S = 0 there); d_mel of the same call is bit-identical to the plain entry's."""
    enc = _encoder(T, case, regime, "bf16")
    mel, d_hidden = _inputs(T, case, pattern)
    pooled = pattern == "pooled"
    grads = _zero_grads(T, case)
    x0, d_mel = sl.c_step(T, enc, mel, pooled, d_hidden, True, True, grads=grads)
    _check_impulse(T, case, pattern, x0)
    _, plain = sl.c_step(T, enc, mel, pooled, d_hidden, False, True)
    assert T.equal(plain, d_mel), "d_mel differs between the plain and the full entry"
    got = {FIELDS[f]: g for f, g in grads.items()}
    live = T.from_numpy(_live(case, pattern).any(0)).cuda()
    assert bool((got["embed_positions.weight"][~live] == 0).all()), "embed_positions row of a dead token is not zero"
    if pattern in ("first", "seg1"):   # token 0 alone: tap 0 of conv2 reads the pad row in front of the segment
        assert bool((got["conv2.weight"][:, :, 0] == 0).all()), "conv2 tap 0 sees only a pad row and is not zero"
    _assert_within("bf16", case, pattern, regime, got, x0, tuple(FIELDS.values()))


@pytest.mark.parametrize("case,pattern", [(2, p) for p in sl.patterns_of(2)] + [(2, "pooled"), (4, "dense"), (4, "last")])
def test_module_route_gives_the_same_gradients(T, gww, case, pattern):
    """enable_full_finetune() and p.grad: the gradients autograd receives are checked like the C entry's, against the d_x0
    of a c_step call with the same d_hidden; the two routes' d_mel are bit-identical, which ties them to one d_x0."""
    enc = _build(T, case, "synth", "bf16").enable_full_finetune()
    for p in enc.parameters():
        p.requires_grad = True
    mel, d_hidden = _inputs(T, case, pattern)
    pooled = pattern == "pooled"
    mel_t = mel.clone().requires_grad_(True)
    out = enc.last_token(mel_t) if pooled else enc(mel_t).last_hidden_state
    out.backward(d_hidden)
    got = {n: enc.get_parameter(n).grad for n in FIELDS.values()}
    x0, d_mel = sl.c_step(T, enc, mel, pooled, d_hidden, True, True)
    _check_impulse(T, case, pattern, x0)
    assert T.equal(mel_t.grad, d_mel), "d_mel differs between the module route and the C entry"
    _assert_within("bf16", case, pattern, "synth", got, x0, tuple(FIELDS.values()))


def test_gradients_accumulate_into_prefilled_buffers(T, gww):
    """The entry accumulates: buffers pre-filled with small integers hold base + gradient -- the gradient of a call into
    zeroed buffers, up to the one fp32 rounding of the sum -- and keep the base exactly where no term reaches."""
    case, pattern = 2, "seg1"
    enc = _encoder(T, case, "synth", "bf16")
    mel, d_hidden = _inputs(T, case, pattern)
    zero = _zero_grads(T, case)
    x0, _ = sl.c_step(T, enc, mel, False, d_hidden, True, False, grads=zero)
    base = _zero_grads(T, case, base=5)
    acc = {f: b.clone() for f, b in base.items()}
    x0b, _ = sl.c_step(T, enc, mel, False, d_hidden, True, False, grads=acc)
    assert T.equal(x0, x0b)
    for f in FIELDS:
        exact = base[f].double() + zero[f].double()
        err = (acc[f].double() - exact).abs()
        ulp = 2.0 ** -23 * exact.abs()
        worst = int(T.argmax(err - ulp))
        assert bool((err <= ulp).all()), (f, worst, float(err.flatten()[worst]), float(exact.flatten()[worst]))
        assert bool((acc[f][zero[f] == 0] == base[f][zero[f] == 0]).all()), f
        assert bool((zero[f] != 0).any()), f
    # and the gradient itself is the checked one
    _assert_within("bf16", case, pattern, "synth", {FIELDS[f]: g for f, g in zero.items()}, x0, tuple(FIELDS.values()))
