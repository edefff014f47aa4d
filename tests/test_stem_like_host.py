"""The conv-stem backward check itself, on the CPU: the fp64 reference against a per-tap loop on the
kernels' padded layout, where the scale S is exactly zero, the host emulation of the bf16 and fp32 chains against the
bound c S (conv gradients: c S + E) that the GPU tests apply (tests/stem_like.py: c_bound is 4 x the worst ratio printed here), and that the
comparison flags every modelled indexing defect on its impulse case.  No GPU."""

import numpy as np
import pytest
import torch

from tests import stem_like as sl

ALL = sl.table() + [(sl.POOLED_CASE, "pooled")]
_CACHE = {}


def _d_x0(case, pattern):
    d, C, Tn, B = sl.CASES[case]
    g = sl.impulse(case, pattern)
    if pattern != "pooled":
        return g
    out = np.zeros((B, Tn, d), np.float32)
    out[:, Tn - 1] = g
    return out


def _setup(case, pattern, regime, precision="bf16"):
    """(sd, mel, d_x0, reference, S, S + E of the precision), computed once and left unchanged."""
    key = (case, pattern, regime)
    if key not in _CACHE:
        sd, mel, g = sl.weights(case, regime), sl.features(case), _d_x0(case, pattern)
        _CACHE[key] = (sd, mel, g, sl.reference(torch, sd, mel, g),
                       {p: sl.scales(torch, sd, mel, g, p) for p in ("bf16", "fp32")})
    sd, mel, g, ref, sc = _CACHE[key]
    return (sd, mel, g, ref) + sc[precision]


@pytest.mark.parametrize("regime", sl.REGIMES)
@pytest.mark.parametrize("case,pattern", ALL)
def test_reference_equals_the_per_tap_loop(case, pattern, regime):
    sd, mel, g, ref, S, _ = _setup(case, pattern, regime)
    loop = sl.chain(torch, sd, mel, g, mode="fp64")
    # gelu' has a zero at z = -0.7518, where two fp64 evaluations of it agree to 1e-16 absolutely, not relatively: an
    # element of a conv gradient under an impulse is one product with it, and gets the floor of the bound's E at fp64's
    # own size.  d_mel and embed_positions sum over all channels and are held to 1e-12 S alone.
    S64 = sl.scale(torch, sd, mel, g, floor=2.0 ** -48)
    for name in sl.NAMES:
        floor = 0.0 if name in sl.RAW_RATIO else S64[name] - S[name]
        assert (np.abs(loop[name] - ref[name]) <= 1e-12 * S[name] + floor).all(), name
        assert (loop[name][S[name] == 0] == 0).all() and (ref[name][S[name] == 0] == 0).all(), name


@pytest.mark.parametrize("case,pattern", [cp for cp in ALL if cp[1] != "dense"])
def test_scale_is_zero_exactly_outside_the_live_frames(case, pattern):
    """S(d_mel) = 0 outside frames 2 t - 2 .. 2 t + 2 of the live tokens and > 0 inside; S(embed_positions) = 0 on the
    dead tokens; a conv2 tap that only ever sees a pad row has S = 0."""
    d, C, Tn, B = sl.CASES[case]
    sd, mel, g, ref, S, Sf = _setup(case, pattern, "synth")
    reach = np.zeros((B, 2 * Tn), bool)
    for b, t in sl.live_tokens(case, pattern):
        reach[b, max(2 * t - 2, 0):min(2 * t + 3, 2 * Tn)] = True
    assert ((S["d_mel"] > 0) == reach[:, None, :]).all()
    assert ((Sf["d_mel"] > 0) == reach[:, None, :]).all()          # the floor does not widen the support
    live = sl.live_mask(case, pattern).any(0)
    assert ((S["embed_positions.weight"] > 0).all(1) == live).all()
    if pattern in ("first", "seg1"):
        assert (S["conv2.weight"][:, :, 0] == 0).all() and (S["conv2.weight"][:, :, 1:] > 0).all()


@pytest.mark.parametrize("mode", ["bf16", "fp32"])
@pytest.mark.parametrize("regime", sl.REGIMES)
@pytest.mark.parametrize("case,pattern", ALL)
def test_emulation_stays_within_the_bound(case, pattern, regime, mode):
    sd, mel, g, ref, S, Sf = _setup(case, pattern, regime, mode)
    emu = sl.chain(torch, sd, mel, g, mode=mode)
    for name in sl.WORST[mode]:
        c = sl.c_bound(mode, name, case)
        r = sl.ratios(name, emu[name], ref[name], S[name], Sf[name])
        print(f"emulation {mode} case {case} {pattern} {regime} {name}: worst ratio {r.max():.3e} (c = {c:.3e})")
        msg = sl.compare(name, emu[name], ref[name], S[name], Sf[name], c)
        assert msg is None, msg
        if mode == "bf16":   # c is 4 x the worst of these (the fp32 figure moves with the host's matmul order); 10 % for a
            # host whose fp64 summation order flips a bf16 tie
            assert r.max() <= 1.1 * sl.worst(mode, name, case), (name, r.max())


# defect -> the (case, pattern) impulses it must show on, and the tensors in which it shows
_FLAGGED = {
    "tap1_token0": ([(1, "first"), (2, "first"), (6, "first")], ("d_mel", "conv1.weight")),
    "tap2_last_token": ([(1, "last"), (2, "last"), (2, "pooled"), (3, "last")], ("d_mel", "conv1.weight")),
    "halo_frame64": ([(2, "seam"), (4, "seam"), (5, "seam")], ("d_mel",)),
    "neighbour_segment": ([(2, "seg1"), (3, "seg1"), (6, "seg1")], ("d_mel",)),
    "junk_row": ([(2, "seg1"), (4, "seg1")], ("conv2.weight", "conv2.bias")),
    "guard_dropped": ([(2, "seg1"), (5, "seg1")], ("d_mel", "conv1.weight")),
    "kc1_padding": ([(1, "first"), (2, "dense"), (4, "last")], ("conv1.weight",)),
    "pos_one_segment_short": ([(2, "last"), (3, "last"), (2, "dense")], ("embed_positions.weight",)),
}


@pytest.mark.parametrize("regime", sl.REGIMES)
@pytest.mark.parametrize("defect", sl.DEFECTS)
def test_the_comparison_flags_each_modelled_defect(defect, regime):
    """The bf16 emulation with one indexing defect fails the check the GPU test applies, in the tensors named; with the
    tolerance of the bound the defect-free emulation passes (test_emulation_stays_within_the_bound)."""
    cases, tensors = _FLAGGED[defect]
    for case, pattern in cases:
        sd, mel, g, ref, S, Sf = _setup(case, pattern, regime)
        bad = sl.chain(torch, sd, mel, g, mode="bf16", defect=defect)
        for name in tensors:
            msg = sl.compare(name, bad[name], ref[name], S[name], Sf[name], sl.c_bound("bf16", name, case))
            assert msg is not None, (defect, case, pattern, name)
            print(f"{defect} case {case} {pattern} {regime}: {msg}")
        if "d_mel" in tensors:                       # and the fp32 twin's check flags it too
            _, _, _, _, S, Sf = _setup(case, pattern, regime, "fp32")
            bad32 = sl.chain(torch, sd, mel, g, mode="fp32", defect=defect)
            assert sl.compare("d_mel", bad32["d_mel"], ref["d_mel"], S["d_mel"], Sf["d_mel"],
                              sl.c_bound("fp32", "d_mel", case)) is not None, (defect, case, pattern)


def test_the_case_table_and_its_inputs():
    assert sl.CASES == {1: (128, 80, 16, 1), 2: (128, 80, 33, 2), 3: (128, 80, 100, 3), 4: (384, 80, 33, 2),
                        5: (512, 80, 33, 2), 6: (1280, 128, 16, 2), 7: (128, 80, 1500, 2)}
    assert sl.patterns_of(1) == ("first", "last", "dense")                     # T = 16: no seam, one segment
    assert sl.patterns_of(2) == sl.PATTERNS and sl.patterns_of(6) == ("first", "last", "seg1", "dense")
    assert sl.patterns_of(7) == ("dense", "first", "last")
    m = sl.features(2)
    assert (sl.bf16_round(m) == m).all()
    for k in ("conv1.weight", "conv2.weight"):
        w = sl.weights(2, "sat")[k]
        assert (sl.bf16_round(w) == w).all()
    assert set(np.abs(sl.weights(2, "sat")["conv1.bias"])) == {6.0}
