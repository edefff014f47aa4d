"""The Whisper-like generators and yardsticks of tests/whisper_like.py, on the CPU: the generated encoder really has the
outlier statistics the GPU tests rely on, and the algebra the LayerNorm-folded kernels document stays inside the bounds
those tests assert -- so a GPU failure is a finding about a kernel, not about the bound."""

import numpy as np
import pytest

from gw_whisper_amd import synth
from oracle import encoder as oenc
from oracle import logmel as olm

from . import whisper_like as wl

M, K, N = 300, 384, 1152


@pytest.fixture(scope="module")
def mel():
    return olm.log_mel(synth.strain_segments(1, seed=21))


@pytest.mark.parametrize("dims", [(384, 2, 6, 1536), (512, 2, 8, 2048)], ids=lambda d: f"d{d[0]}")
def test_generated_encoder_has_outlier_statistics(mel, dims):
    """The last layer's residual stream: a few channels in the hundreds on a bulk of order one, rows whose sigma the outliers
    set, and a bf16 emulation error of the order the Gaussian weights give (the encoder is hard, not ill-posed)."""
    d, L, H, F = dims
    sd = wl.whisper_like_state_dict(d, L, H, F, seed=7)
    sd2 = wl.whisper_like_state_dict(d, L, H, F, seed=7)
    assert all(v.dtype == np.float32 and np.array_equal(v, sd2[k]) for k, v in sd.items())
    cfg = oenc.EncCfg(d, L, H, F)
    ref, stages = oenc.encoder_forward(sd, mel, cfg, dtype=np.float64, return_stages=True)
    x = stages[f"l{L - 1}.out"][0]
    amax, sig, med = np.abs(x).max(), np.median(x.std(axis=1)), np.median(np.abs(x))
    emu = oenc.encoder_forward(sd, mel, cfg, dtype=np.float64, emulate_bf16=True)
    rms_emu = np.sqrt(((emu - ref) ** 2).mean())
    print(f"whisper-like d={d}: max|x| {amax:.0f}, median row sigma {sig:.2f}, median |x| {med:.2f}, "
          f"bf16 emulation rms {rms_emu:.2e}, output rms {np.sqrt((ref ** 2).mean()):.3f}")
    assert amax >= 100
    assert sig >= 4
    assert med <= 3
    assert 4e-4 <= rms_emu <= 3e-3
    # fc1 pre-activations reach the tens: the |z| >= 8 branch of the fused GELUs is executed by the encoder tests
    oc = wl.outlier_channels(d)
    assert np.abs(x[:, oc]).min() > 20 and oc[0] < wl.PREFIX <= oc[1]


@pytest.fixture(scope="module")
def families():
    rng = np.random.default_rng(2024)
    fam = wl.activation_families(rng, M, K)
    W = (rng.standard_normal((N, K)) / np.sqrt(K)).astype(np.float32)
    bias = rng.standard_normal(N).astype(np.float32)
    return fam, W, bias


def test_families_are_what_they_say(families):
    fam, _, _ = families
    amp = {k: wl.noise_bound(*v, np.zeros((1, K), np.float32), None)[0] for k, v in fam.items()}
    assert np.median(amp["gauss"]) < 1.03 and amp["out_late"].max() < 1.01  # the prefix represents the row
    assert amp["out_in32"].min() > 1.03 and amp["slope"].min() > 1.4 and amp["block32"].min() > 2.4
    # a prefix mean lies at most sqrt((K - 32) / 32) row sigma from the row mean
    worst = np.sqrt(1 + (K - wl.PREFIX) / wl.PREFIX / 2)
    assert all(a.max() <= worst + 1e-9 for a in amp.values())
    assert amp["block32"].max() > 0.95 * worst                              # ... and block32 all but attains it
    x = fam["nearconst"][0].astype(np.float64)
    assert x.var(axis=1).max() < wl.LN_EPS
    cr = wl.constant_rows(fam["degenerate"][0])
    assert cr[0::3].all() and cr[1::3].all() and not cr[2::3].any()
    g = fam["gains"][1]
    assert (g < 0).sum() == K // 4 and np.abs(g).max() / np.abs(g).min() > 100


@pytest.mark.parametrize("gelu", [False, True], ids=["linear", "gelu"])
@pytest.mark.parametrize("family", wl.FAMILIES)
def test_documented_algebra_meets_the_bounds(families, family, gelu):
    """bf16(x - prefix mean), exact fp32 one-pass statistics, rstd (a W'^T - mean' u) + cb: inside both bounds on every
    family (measured: rms 0.3 .. 0.8 of the limit, per-element excess below 7 of the 10 allowed)."""
    fam, W, bias = families
    x, g, b = fam[family]
    out = wl.emulate_prefix_shift(x, g, b, W, bias, gelu=gelu)
    assert np.isfinite(out).all()
    r_rms, r_el, ok_rms, ok_el = wl.check_folded_projection(out, x, g, b, W, bias, gelu=gelu)
    print(f"emulation {family} gelu={gelu}: rms / limit {r_rms:.3f}, worst element excess / (amp b) {r_el:.2f}")
    assert ok_rms and ok_el
    cr = wl.constant_rows(x)
    if cr.any():
        _, _, cb = wl.folded(g, b, W, bias)
        ref = oenc.gelu(cb) if gelu else cb
        np.testing.assert_allclose(out[cr], np.broadcast_to(ref, out[cr].shape), rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("family,shift", [("out_col0", "first"), ("nearconst", "none")])
def test_the_bounds_catch_a_worse_shift(families, family, shift):
    """Shifting by the row's first element breaks the rms bound when that element is an outlier, no shift at all when the
    row's spread is far below its mean.  (On the other families neither regression shows in the emulation: their rows have
    a mean of order sigma and no outlier in column 0.)"""
    fam, W, bias = families
    x, g, b = fam[family]
    out = wl.emulate_prefix_shift(x, g, b, W, bias, shift=shift)
    r_rms, r_el, ok_rms, ok_el = wl.check_folded_projection(out, x, g, b, W, bias)
    print(f"emulation {family} shift={shift}: rms / limit {r_rms:.3f}, worst element excess / (amp b) {r_el:.2f}")
    assert not ok_rms
