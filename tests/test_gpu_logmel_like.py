"""ops.logmel per element on band-limited strain (tests/logmel_like.py): every element the fp64 oracle leaves unclamped is
held to LIMIT x GAMMA x e_model of its own, the clamped ones to one bit-identical value per segment, the per-segment
maximum to its segment, power-of-two scalings to an exact shift.  The inputs, the oracle (exact arithmetic on the
library's window table), the bound and the constants are those test_logmel_like_host.py checks without a GPU.  Figures
measured on an MI355X are in DESIGN.md section 24."""

import numpy as np
import pytest

from oracle import logmel as olm

from . import logmel_like as ll

pytestmark = pytest.mark.gpu

CASES = [(f, m) for f in ll.FAMILIES for m in ll.N_MELS]
_OUT = {}


@pytest.fixture(scope="module")
def T():
    import torch
    assert torch.cuda.is_available()
    return torch


def run(T, wave, n_mels):
    from gw_whisper_amd import ops
    out = ops.logmel(T.from_numpy(np.array(wave)).cuda(), n_mels=n_mels).cpu().numpy()   # (a copy: the cases are read-only)
    assert out.shape == (wave.shape[0], n_mels, olm.N_FRAMES) and out.dtype == np.float32
    return out


def device_out(T, family, n_mels):
    """The kernel's output of every batch of the family, computed once."""
    if (family, n_mels) not in _OUT:
        outs = [run(T, c.wave, n_mels) for c in ll.cases(family, n_mels)]
        for o in outs:
            o.setflags(write=False)
        _OUT[(family, n_mels)] = outs
    return _OUT[(family, n_mels)]


def limit(family, n_mels):
    return ll.LIMIT * ll.GAMMA[(family, n_mels)]


@pytest.mark.parametrize("family,n_mels", CASES)
def test_every_unclamped_element_within_its_own_bound(T, gww, family, n_mels):
    """|ops.logmel - oracle| <= LIMIT x GAMMA x e_model[m, f] on the elements the oracle leaves unclamped (those on the 1e-10
    clamp of the quiet ladder and mixed items included: the model's denominator is the clamped mel)."""
    worst = 0.0
    for c, out in zip(ll.cases(family, n_mels), device_out(T, family, n_mels)):
        assert c.unclamped.any()
        r = c.ratio(out)
        worst = max(worst, float(r[c.unclamped].max()))
    print(f"{family} {n_mels}: worst |err| / e_model = {worst:.3f} = {worst / ll.GAMMA[(family, n_mels)]:.3f} x GAMMA "
          f"(limit {ll.LIMIT:g} x GAMMA)")
    assert worst <= limit(family, n_mels)


@pytest.mark.parametrize("family,n_mels", CASES)
def test_clamped_elements_hold_one_value_per_segment(T, gww, family, n_mels):
    """Every live element the oracle puts at least 0.01 (log10) under the floor holds one single value per segment; that
    value is the dead-frame constant whenever the floor is at or above -10 and the item has dead frames, and it is off the
    oracle's floor value by no more than the bound of the segment's maximum element (the floor is the maximum minus 8)."""
    seen = 0
    for c, out in zip(ll.cases(family, n_mels), device_out(T, family, n_mels)):
        for i in range(out.shape[0]):
            far = c.clamped[i]
            dead = out[i, :, c.live:]
            if dead.size:
                assert (dead == dead[0, 0]).all(), "dead frames must be one constant"
                assert abs(float(dead[0, 0]) - c.pad[i]) <= limit(family, n_mels) * c.e_max[i]
            if not far.any():
                continue
            seen += 1
            v = out[i, :, :c.frames][far]
            assert (v == v[0]).all()
            if dead.size and c.floor[i] >= -10.0:
                assert v[0] == dead[0, 0]
            floor_out = (c.floor[i] + 4.0) / 4.0
            assert abs(float(v[0]) - floor_out) <= limit(family, n_mels) * c.e_max[i]
    assert seen or family == "white"


@pytest.mark.parametrize("n_mels", ll.N_MELS)
def test_the_maximum_is_taken_per_segment(T, gww, n_mels):
    """Each item of [burst, resampled x 1e-3, zeros, line60] is bit-identical to the same item run alone (four floors 12
    decades apart in one batch); the all-zero item is -1.5 everywhere."""
    wave = ll.cases("mixed", n_mels)[0].wave
    out = device_out(T, "mixed", n_mels)[0]
    for i in range(wave.shape[0]):
        assert np.array_equal(run(T, wave[i:i + 1], n_mels)[0], out[i]), i
    assert (out[2] == np.float32(-1.5)).all()


@pytest.mark.parametrize("n_mels", ll.N_MELS)
def test_power_of_two_scalings_shift_the_output_exactly(T, gww, n_mels):
    """Scaling the input by 2^k scales every fp32 product and sum of the kernel exactly, so the mel energies are the same
    significands: on elements that neither item clamps (the max - 8 floor or the 1e-10 one, by the oracle, with a margin
    of 0.01 in log10), out(2^k x) - out(x) = k log10(2) / 2 up to the roundings of the log10 and of the sum with 4.0 in each
    item: at most one unit (ll.out_ulp) each, two per item, four in the difference.  The 2^-17 item (1e-10 clamp active)
    also meets the per-element bound against the oracle."""
    c = ll.cases("ladder", n_mels)[0]
    out = device_out(T, "ladder", n_mels)[0][:, :, :c.live].astype(np.float64)
    raw = c.raw[:, :, :c.live]
    free = (raw >= c.floor[:, None, None] + ll.NEAR) & (raw >= -10.0 + ll.NEAR)
    for i, k in enumerate(ll.LADDER_K):
        if k == 0:
            continue
        both = free[0] & free[i]
        assert both.sum() > 1000, k
        d = np.abs(out[i] - out[0] - k * np.log10(2.0) / 2.0)
        tol = 4.0 * np.maximum(ll.out_ulp(out[i]), ll.out_ulp(out[0]))
        print(f"2^{k}: {int(both.sum())} elements, worst {float((d / tol)[both].max()) * 4:.2f} units")
        assert (d[both] <= tol[both]).all(), k
    i17 = ll.LADDER_K.index(-17)
    assert c.at_1e10[i17].any()
    r = c.ratio(device_out(T, "ladder", n_mels)[0])[i17]
    assert r[c.unclamped[i17]].max() <= limit("ladder", n_mels)


@pytest.mark.parametrize("n_mels", ll.N_MELS)
def test_ragged_edges(T, gww, n_mels):
    """The last partial frame, the first dead frame and the right reflect edge of the full buffer (frames 2990..2999)
    against the oracle, per element; the dead frames one constant."""
    lim = limit("ragged", n_mels)
    for c, out in zip(ll.cases("ragged", n_mels), device_out(T, "ragged", n_mels)):
        r = c.ratio(out)
        if c.live < olm.N_FRAMES:
            last = c.live - 1
            assert c.unclamped[0, :, last].any()
            assert (r[0, :, last][c.unclamped[0, :, last]] <= lim).all()
            dead = out[0, :, c.live:]
            assert (dead == dead[0, 0]).all()
            assert abs(float(dead[0, 0]) - c.out[0, 0, c.live]) <= lim * c.e_max[0]
        else:
            edge = slice(2990, 3000)
            assert c.unclamped[0, :, edge].any()
            assert (r[0, :, edge][c.unclamped[0, :, edge]] <= lim).all()
            far = c.clamped[0, :, edge]
            assert (np.abs(out[0, :, edge].astype(np.float64) - c.out[0, :, edge])[far] <= lim * c.e_max[0]).all()
