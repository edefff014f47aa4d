"""The constant-tail shortcut of the bf16 inference stem (csrc/stem_tail.hip; needs an MI355X, -m gpu).

Every comparison is between the shortcut switched on and off in the same process (``set_stem_shortcut``) and is exact:
``torch.equal`` on the int32 view of the fp32 outputs, so that -0 / +0 and NaN payloads count too.  ``stem_shortcut_flags``
reads back what the device decided: 1 = the compact stem ran, 0 = the full one.
"""

import numpy as np
import pytest

from gw_whisper_amd import synth
from tests.guard import encoder_arena_row_bytes, run_contract

pytestmark = pytest.mark.gpu

TC = 256            # csrc/common.h: kStemTc; the detected range is [TC - 6, 3000)
SPLIT_MIN = 32      # csrc/encoder.hip: kSplitMin


@pytest.fixture(scope="module")
def T():
    import torch
    assert torch.cuda.is_available()
    return torch


_ENC = {}


def _encoder(name):
    """One encoder per size for the whole module (real widths and depths of whisper-tiny / -base)."""
    if name not in _ENC:
        from gw_whisper_amd.encoder import WhisperConfig, WhisperEncoder
        sd = synth.named_encoder_state_dict(name, seed=11)
        _ENC[name] = WhisperEncoder.from_numpy_state_dict(sd, WhisperConfig.named(name), precision="bf16").cuda()
    enc = _ENC[name]
    enc.set_split(False)
    enc.set_stem_shortcut(True)
    return enc


def _logmel(T, batch, seconds, seed=1000):
    from gw_whisper_amd import ops
    wave = synth.strain_segments(batch, seed=seed, n_samples=int(16000 * seconds))
    return ops.logmel(T.from_numpy(wave).cuda())


def _bits_equal(T, a, b):
    return a.shape == b.shape and T.equal(a.contiguous().view(T.int32), b.contiguous().view(T.int32))


def _outputs(enc, mel, outputs=True):
    """Everything the three entry points return that the stem feeds: last_hidden_state, the pooled last token, and
    hidden_states[0] (the stem's own output) / [-1] of gww_encoder_forward_outputs."""
    out = {"last_hidden_state": enc.forward_raw(mel, want_hidden=True, want_last=False)[0],
           "last_token": enc.forward_raw(mel, want_hidden=False, want_last=True)[1]}
    both = enc.forward_raw(mel, want_hidden=True, want_last=True)
    out["both.hidden"], out["both.last"] = both
    if outputs:
        _, hs, _ = enc.forward_outputs_raw(mel, True, False)
        out["hidden_states[0]"], out["hidden_states[-1]"] = hs[0].clone(), hs[-1].clone()
    return out


def _compare(T, enc, mel, want_flags, outputs=True):
    B = mel.shape[0]
    enc.set_stem_shortcut(True)
    on = _outputs(enc, mel, outputs)
    flags = enc.stem_shortcut_flags(B)
    assert flags == want_flags, f"device flags {flags}, expected {want_flags}"
    enc.set_stem_shortcut(False)
    off = _outputs(enc, mel, outputs)
    assert enc.stem_shortcut_flags(B) == (-1, -1)
    enc.set_stem_shortcut(True)
    for k in on:
        assert _bits_equal(T, on[k], off[k]), f"{k}: shortcut on and off differ (B = {B})"
    return on


@pytest.mark.parametrize("seconds", [1.0, 1.5])
@pytest.mark.parametrize("B", [1, 3, 64])
@pytest.mark.parametrize("name", ["tiny", "base"])
def test_shortcut_taken(T, name, B, seconds):
    """Log-mel of seeded 1 s and 1.5 s strain: the flag reads 1 and every output is bit-identical to the full stem's."""
    enc = _encoder(name)
    on = _compare(T, enc, _logmel(T, B, seconds), (1, -1))
    assert bool(T.isfinite(on["last_hidden_state"]).all())


@pytest.mark.parametrize("B", [2 * SPLIT_MIN, 2 * SPLIT_MIN + 3])
@pytest.mark.parametrize("name", ["tiny", "base"])
def test_shortcut_taken_split(T, name, B):
    """Split mode: one flag per half batch, each in that half's workspace; and a batch whose second half alone is dense
    takes the shortcut in the first half only."""
    enc = _encoder(name)
    enc.set_split(True)
    mel = _logmel(T, B, 1.0)
    on = _compare(T, enc, mel, (1, 1), outputs=(name == "tiny"))
    mixed = mel.clone()
    mixed[B - 1, 17, 1500] += 0.25
    _compare(T, enc, mixed, (1, 0), outputs=False)
    enc.set_split(False)
    plain = enc.forward_raw(mel)[0]
    assert _bits_equal(T, on["last_hidden_state"], plain), "split and unsplit forwards differ"


@pytest.mark.parametrize("seg", ["first", "last"])
@pytest.mark.parametrize("t", [TC - 6, TC - 5, 1500, 2999])
def test_fallback_one_element(T, t, seg):
    """ONE changed element inside the detected range, in the first / last segment: the flag reads 0, results are equal."""
    enc = _encoder("tiny")
    mel = _logmel(T, 3, 1.0)
    b = 0 if seg == "first" else 2
    mel[b, 41, t] += 0.125
    _compare(T, enc, mel, (0, -1), outputs=(t == TC - 6))


@pytest.mark.parametrize("seg", ["first", "last"])
@pytest.mark.parametrize("t", [TC - 6, TC - 5, 1500, 2999])
@pytest.mark.parametrize("kind", ["sign_of_zero", "nan"])
def test_fallback_bit_patterns(T, kind, t, seg):
    """The comparison is on bit patterns: a tail of +0 with one -0 in it, and a tail with one NaN in it, are not constant.
    (A tail that is +0 throughout is: the control below.)"""
    enc = _encoder("tiny")
    mel = _logmel(T, 3, 1.0)
    b = 0 if seg == "first" else 2
    if kind == "sign_of_zero":
        mel[b, 5, TC - 6:] = 0.0
        if t == TC - 6 and seg == "first":
            _compare(T, enc, mel, (1, -1), outputs=False)     # control: still constant, still the shortcut
        mel[b, 5, t] = -0.0
        assert float(mel[b, 5, t]) == 0.0 and bool(T.signbit(mel[b, 5, t]))
    else:
        mel[b, 5, t] = float("nan")
    _compare(T, enc, mel, (0, -1), outputs=False)


def test_fallback_long_and_dense(T):
    """Log-mel of 3 s strain (302 live frames) and dense random features take the full stem."""
    enc = _encoder("tiny")
    _compare(T, enc, _logmel(T, 3, 3.0), (0, -1))
    rng = np.random.default_rng(7)
    dense = np.clip(rng.standard_normal((3, 80, 3000)) * 0.5, -1.5, 1.5).astype(np.float32)
    _compare(T, enc, T.from_numpy(dense).cuda(), (0, -1))
    for name in ("base",):
        _compare(T, _encoder(name), T.from_numpy(dense).cuda(), (0, -1), outputs=False)


@pytest.mark.parametrize("name", ["tiny", "base"])
def test_boundary_element_outside_the_range(T, name):
    """An element changed at t = TC - 7, the last frame in front of the detected range, still takes the shortcut and still
    matches: it reaches conv1 frames <= TC - 6 and tokens <= TC / 2 - 3, which the compact stem computes from the data."""
    enc = _encoder(name)
    mel = _logmel(T, 3, 1.0)
    ref = enc.forward_raw(mel)[0].clone()
    for b in (0, 2):
        mel[b, :, TC - 7] += 0.5
    on = _compare(T, enc, mel, (1, -1))
    assert not T.equal(on["last_hidden_state"], ref), "the changed frame did not reach the output"


@pytest.mark.parametrize("name", ["tiny", "base"])
def test_memory_contract(T, name):
    """The forward under guard bands with the workspace re-allocated under the guard (filled with NaN, 3.39e38 and 0 in
    turn), shortcut on: nothing is written outside the contract and the outputs do not depend on the fill, so no stale or
    uninitialised row of c1 / the compact buffers is read.  B = 3 and 5: the compact c1 ends inside / between 256-row panels."""
    from gw_whisper_amd._lib import PREC_BF16, lib
    enc = _encoder(name)
    d, _, _, F = synth.ENCODER_SIZES[name]
    for B in (3, 5):
        mel = _logmel(T, B, 1.0, seed=1000 + B)

        def case(g):
            enc._ws = None
            pm = g.place(mel)
            h, l = enc.forward_raw(pm, want_hidden=True, want_last=True)
            assert g.owns(enc._ws), "the encoder's workspace did not come from the guard"
            assert enc._ws.numel() == lib().gww_encoder_workspace_bytes(enc._handle, B, PREC_BF16)
            assert enc.stem_shortcut_flags(B) == (1, -1)
            (p,) = enc.forward_raw(pm, want_hidden=False, want_last=True)[1:]
            return {"hidden": h, "last": l, "pooled": p}
        r = run_contract(case, arena_row_bytes=encoder_arena_row_bytes(d, F))
        enc._ws = None
        enc.set_stem_shortcut(False)
        want_h, want_l = enc.forward_raw(mel, want_hidden=True, want_last=True)
        want_p = enc.forward_raw(mel, want_hidden=False, want_last=True)[1]
        enc.set_stem_shortcut(True)
        assert _bits_equal(T, r["hidden"], want_h) and _bits_equal(T, r["last"], want_l)
        assert _bits_equal(T, r["pooled"], want_p)
