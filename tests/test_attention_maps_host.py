"""The checker of the attention-map tests discriminates (no GPU): on every case of tests/test_gpu_attention_maps.py's
grid except T = 1500 it passes a plain float32 restatement of the map and rejects five subtly or grossly wrong maps
built from the float64 reference, and the conditions that keep a case meaningful hold."""
import numpy as np
import pytest

from . import attention_maps_helpers as mh

CASES = [pytest.param(c, id=mh.case_id(c)) for c in mh.HOST_GRID]
LN2 = 0.6931471805599453


def _swap_lane_halves(p):
    """keys 0-3 exchanged with keys 4-7 in every 32-key tile: the two halves of a lane pair writing each other's first
    store (a tile's tail is exchanged only where both groups exist)"""
    T = p.shape[-1]
    idx = np.arange(T)
    for t in range(0, T, 32):
        if t + 8 <= T:
            idx[t:t + 4], idx[t + 4:t + 8] = np.arange(t + 4, t + 8), np.arange(t, t + 4)
    return p[..., idx]


def _defects(qkv, H, q_log2):
    s, p = mh.reference(qkv, H, q_log2)
    T = p.shape[-1]
    return {
        "scale_1.01": mh.softmax64(s * 1.01),
        "bf16_p": mh._bf(p.astype(np.float32)).astype(np.float64),
        "lane_halves": _swap_lane_halves(p),
        "exp2_for_exp": mh.softmax64(s * LN2),
        "uniform": np.full_like(p, 1.0 / T),
    }


def _not_a_defect(kind, T):
    """equal_keys: every score of a row is the same number, so the map is 1/T whatever the score scale, the base of
    the exponential or the order of the keys: only rounding P changes it.  T = 4 has no keys 4-7 to exchange."""
    skip = set()
    if kind == "equal_keys":
        skip |= {"scale_1.01", "exp2_for_exp", "lane_halves", "uniform"}
    if T < 8:
        skip.add("lane_halves")
    return skip


@pytest.mark.parametrize("case", CASES)
def test_restatement_passes_and_conditions_hold(case):
    kind, B, T, H = case
    data = mh.case_data(case)
    for variant, q_log2 in (("bf16", False), ("log2q", True)):
        v = data[variant]
        worst = mh.check(mh.restatement32(v["qkv"], H, q_log2), v["ref"], v["tol"])
        print(f"{mh.case_id(case)} {variant}: restatement32 {worst:.2e} = e32 {v['e32']:.2e}, tol {v['tol']:.2e}, "
              f"{100 * float((v['ref'] < mh.FLOOR).mean()):.1f} % below the floor, max p {float(v['ref'].max()):.4f}")
        assert worst == v["e32"]
        mh.check_conditions(kind, v["ref"], v["tol"])


@pytest.mark.parametrize("case", CASES)
def test_defects_are_rejected(case):
    kind, B, T, H = case
    data = mh.case_data(case)
    skip = _not_a_defect(kind, T)
    for variant, q_log2 in (("bf16", False), ("log2q", True)):
        v = data[variant]
        for name, wrong in _defects(v["qkv"], H, q_log2).items():
            if name in skip:
                assert mh.check(wrong, v["ref"], v["tol"]) <= v["tol"], name      # indeed no defect there
                continue
            with pytest.raises(AssertionError):
                mh.check(wrong, v["ref"], v["tol"])
                pytest.fail(f"{mh.case_id(case)} {variant}: the checker accepted the defect {name}", pytrace=False)


def test_check_names_the_entry():
    case = ("bland", 1, 36, 1)
    v = mh.case_data(case)["bf16"]
    wrong = v["ref"].copy()
    wrong[0, 0, 5, 7] *= 1.0 + 1e-4
    with pytest.raises(AssertionError, match=r"\(0, 0, 5, 7\)"):
        mh.check(wrong, v["ref"], v["tol"])
    neg = v["ref"].copy()
    neg[0, 0, 1, 2] = -1e-30
    with pytest.raises(AssertionError, match="negative"):
        mh.check(neg, v["ref"], v["tol"])
    nan = v["ref"].copy()
    nan[0, 0, 3, 3] = np.nan
    with pytest.raises(AssertionError, match="not finite"):
        mh.check(nan, v["ref"], v["tol"])


def test_below_the_floor_zero_passes_and_a_large_value_does_not():
    case = ("peaked", 1, 132, 1)
    v = mh.case_data(case)["bf16"]
    lo = v["ref"] < mh.FLOOR
    assert lo.any()
    flushed = np.where(lo, 0.0, v["ref"])
    mh.check(flushed, v["ref"], v["tol"])
    at = tuple(np.argwhere(lo)[0])
    leak = v["ref"].copy()
    leak[at] = 1e-20                       # far below the row-sum rule, far above the floor
    with pytest.raises(AssertionError, match="below the floor"):
        mh.check(leak, v["ref"], v["tol"])


def test_old_absolute_rule_accepts_bf16_rounded_maps():
    """Why this file exists.  On the contract test's input (bland, B 2, T 200, H 2, the same seed) the earlier rule
    max |P - P_ref| < 2e-3 accepts a map whose every entry was rounded to bf16; the relative checker does not."""
    B, T, H = 2, 200, 2
    qkv = mh.make_case("bland", B, T, H, mh.case_seed("bland", B, T, H))
    rng = np.random.default_rng(B * 100 + T + H)
    assert np.array_equal(qkv, mh._bf(rng.standard_normal((B, T, 3 * H * 64)) * 0.3))
    ref = mh.reference(qkv, H)[1]
    tol, e32 = mh.tolerance(qkv, H, False, ref)
    rounded = mh._bf(ref.astype(np.float32)).astype(np.float64)
    assert np.abs(rounded - ref).max() < 2e-3
    with pytest.raises(AssertionError, match="relative error"):
        mh.check(rounded, ref, tol)
