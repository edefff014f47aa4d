"""The inputs, the yardstick and the error model of tests/test_gpu_logmel_like.py, held to what those tests assume, and the
host twin of the front end on the same inputs (no GPU).

Conditions on the fp64 oracle and the numpy restatements alone: the band-limited families put a large share of their live
elements on the clamp floor and a large share above it (white noise does not), the ideal-fp32 restatement reproduces the
GAMMA constants every GPU limit is a multiple of, and the HuggingFace extractor's own output (tests/golden/logmel_like.npz,
tools/make_golden.py logmel_like) is inside the bound the kernel is held to.  Figures measured here are in DESIGN.md
section 24."""

import numpy as np
import pytest
import torch

from gw_whisper_amd import ops

from . import logmel_like as ll
from .test_logmel_host import TOL

CASES = [(f, m) for f in ll.FAMILIES for m in ll.N_MELS]
BAND_LIMITED = ("resampled2048", "resampled4096", "burst", "line60")
HF_WITHIN_TOL = ("white",)      # the only family on which HF itself is within TOL of exact arithmetic (0.95e-6, 7.7e-6)


def golden_on_case(g, family, n_mels, b, case):
    """(HF's values float64 [n, n_mels, c], the frames c they are of) among the frames the case holds."""
    key = f"{family}_m{n_mels}_b{b}"
    cols = g[key + "_cols"] if key + "_cols" in g.files else np.arange(ll.FRAMES_1S)
    keep = cols < case.frames
    return g[key + "_frames"][:, :, keep].astype(np.float64), cols[keep]


def test_the_resample_is_scipys():
    import scipy.signal as scipy_signal
    rng = np.random.default_rng(0)
    for n, num in ((2048, 16000), (4096, 16000), (1581, 12351), (61440, 480000)):
        x = rng.standard_normal((2, n))
        assert np.abs(ll.fft_resample(x, num) - scipy_signal.resample(x, num, axis=-1)).max() <= 1e-12, (n, num)


def test_generator_is_deterministic_and_the_families_are_what_they_say():
    for f in ll.FAMILIES:
        a, b = ll.batches(f), ll.batches(f)
        assert all(x.dtype == np.float32 and np.array_equal(x, y) for x, y in zip(a, b))
        assert all(x.shape[0] <= 4 for x in a)
    assert [x.shape for x in ll.batches("ragged")] == [(1, n) for n in ll.RAGGED_N]
    lad = ll.batches("ladder")[0].astype(np.float64)
    for i, k in enumerate(ll.LADDER_K):
        assert np.array_equal(lad[i], lad[0] * 2.0 ** k)                 # exact scalings
    mixed = ll.batches("mixed")[0]
    assert not mixed[2].any() and 1e-4 < np.abs(mixed[1]).max() < 1e-2
    r = ll.batches("resampled2048")[0].astype(np.float64)
    spec = np.abs(np.fft.rfft(r, axis=-1))                               # 1 Hz per bin
    assert spec[:, 1100:].max() < 1e-5 * spec[:, :1000].max()            # nothing above the old Nyquist frequency
    assert 0.8 < r.std() < 1.2
    assert 900 < np.abs(ll.batches("line60")[0]).max() < 1010 and 250 < np.abs(ll.batches("burst")[0]).max() < 310


@pytest.mark.parametrize("n_mels", ll.N_MELS)
def test_the_clamp_acts_on_band_limited_strain_and_not_on_white(n_mels):
    """Coverage conditions.  Measured (unclamped, clamped) shares of the live elements, 80 / 128 mels: resampled2048
    0.466 / 0.457 unclamped, resampled4096 0.635 / 0.631, burst 0.350 / 0.351, line60 0.357 / 0.348; white 1.000 / 1.000
    (nothing clamped); the 2^-17 item of the ladder has 10294 / 16643 elements on the 1e-10 clamp."""
    for f in BAND_LIMITED:
        un, cl = ll.shares(f, n_mels)
        print(f"{f} {n_mels}: unclamped {un:.3f}, clamped {cl:.3f}")
        assert un >= 0.10 and cl >= 0.10, f
    un, cl = ll.shares("white", n_mels)
    print(f"white {n_mels}: unclamped {un:.3f}, clamped {cl:.3f}")
    assert 1.0 - un <= 0.02
    lad = ll.cases("ladder", n_mels)[0]
    k17 = ll.LADDER_K.index(-17)
    assert lad.floor[k17] < -10.0 and int(lad.at_1e10[k17].sum()) > 1000
    assert not lad.at_1e10[0].any()


@pytest.mark.parametrize("family,n_mels", CASES)
def test_ideal_fp32_reproduces_gamma(family, n_mels):
    g = ll.gamma(family, n_mels)
    print(f'    ("{family}", {n_mels}): {g:.3e},')
    assert abs(g / ll.GAMMA[(family, n_mels)] - 1) <= 0.1


@pytest.mark.parametrize("family,n_mels", CASES)
def test_hf_is_inside_the_bound_the_kernel_is_held_to(golden, family, n_mels):
    """|HF - oracle| <= LIMIT x GAMMA x e_model on every element the oracle leaves unclamped: the reference's own
    extractor is an fp32 computation too (on another window table, torch.hann_window).  Measured |HF - oracle| /
    (GAMMA e_model), worst element, 80 / 128 mels: white 1.01 / 1.35, resampled2048 1.07 / 0.72, resampled4096 1.03 / 1.37,
    burst 1.62 / 1.46, line60 1.00 / 0.80, line500 1.17 / 1.47, ladder 0.90 / 0.85, mixed 0.77 / 0.79, ragged 0.69 / 0.52;
    as an absolute error 0.95e-6 (white, 80) .. 1.3e-4 (line500, 128)."""
    g = golden("logmel_like.npz")
    worst, worst_abs = 0.0, 0.0
    for b, c in enumerate(ll.cases(family, n_mels)):
        hf, cols = golden_on_case(g, family, n_mels, b, c)
        err = np.abs(hf - c.out[:, :, cols])
        un = c.unclamped[:, :, cols]
        assert un.any()
        worst = max(worst, float((err / c.e_model[:, :, cols])[un].max()) / ll.GAMMA[(family, n_mels)])
        worst_abs = max(worst_abs, float(err.max()))
        # the clamped elements and the dead frames: the floor is the maximum's, whose bound is e_max
        lim = ll.LIMIT * ll.GAMMA[(family, n_mels)] * c.e_max
        assert (np.abs(g[f"{family}_m{n_mels}_b{b}_pad_value"] - c.pad) <= lim).all()
        far = c.clamped[:, :, cols]
        assert (err[far] <= np.broadcast_to(lim[:, None, None], err.shape)[far]).all()
    print(f"{family} {n_mels}: HF worst |err| / (GAMMA e_model) = {worst:.2f}, max |err| = {worst_abs:.2e}")
    assert worst <= ll.LIMIT


@pytest.mark.parametrize("family,n_mels", CASES)
def test_host_twin_against_its_restatement_and_hf(golden, family, n_mels):
    """ops.logmel_host within 4 x max |ideal_host - oracle| of the oracle on every element (that maximum: 0.8e-7 .. 1.9e-7,
    3.6e-7 on the ladder, whose 2^-17 item has outputs near -1.5; the twin's own error measured the same figures), its dead
    frames one constant; against HF at the TOL of test_logmel_host.py on the one family where HF is that exact."""
    g = golden("logmel_like.npz")
    for b, c in enumerate(ll.cases(family, n_mels)):
        out = ops.logmel_host(c.wave, n_mels=n_mels).numpy()
        assert out.shape == (c.wave.shape[0], n_mels, 3000) and out.dtype == np.float32
        yard = float(np.abs(ll.ideal_host(c.wave, n_mels)[:, :, :c.frames] - c.out).max())
        err = float(np.abs(out[:, :, :c.frames] - c.out).max())
        print(f"{family} {n_mels} batch {b}: host max |err| {err:.2e}, ideal_host {yard:.2e}")
        assert 0 < yard < 5e-7 and err <= 4 * yard
        assert (out[:, :, c.live:] == out[:, :1, 2999:]).all()
        assert (np.abs(out[:, 0, 2999] - c.pad) <= 4 * yard).all()
        if family in HF_WITHIN_TOL:
            hf, cols = golden_on_case(g, family, n_mels, b, c)
            np.testing.assert_allclose(out[:, :, cols], hf, atol=TOL, rtol=0)


def test_the_two_window_tables_differ():
    """float32(exact Hann), the library's table, against torch.hann_window(400), HF's: up to 2.4e-7 apart.  In exact
    arithmetic that alone moves a leakage-skirt element by about 3e-5, so the oracle of these tests is given the
    library's table: the window table is part of the definition of the operation."""
    d = np.abs(torch.hann_window(400).numpy().astype(np.float64) - ll.lib_window().astype(np.float64)).max()
    print(f"max |torch.hann_window(400) - float32(exact Hann)| = {d:.3e}")
    assert 0 < d < 1e-6
