"""tests/exact_int.py on the CPU, for every case of the table that tests/test_gpu_backward_exact.py runs on the device:
(a) the operands keep the rules of the module docstring and every intermediate stays in the fp32-exact range, with u and v
exact as bf16; sampled elements of the reference are re-derived with int64 sums and ``fractions.Fraction`` scales;
(b) an fp32 numpy evaluation that sums the rows in a scrambled split returns the reference bit for bit; (c) the bitwise
comparison flags every defect of ``exact_int.MUTATIONS`` that can occur in the case.  (c) is a condition on the table: a
case in which one of its defects leaves every output element unchanged may not be in it.  No GPU."""

from fractions import Fraction

import numpy as np
import pytest

from tests import exact_int as xi

IDS = [c.id for c in xi.CASES]


def _parts(case):
    kernel = "dora" if case.kernel == "dora_multi" else case.kernel
    return [(label, kernel, e, xi.reference(kernel, e)) for label, e in xi.effective(case)]


def test_table_covers_what_the_device_test_promises():
    by = {k: xi.cases(k) for k in ("wgrad", "dora", "dora_multi", "adapter", "ln")}
    assert sum(len(v) for v in by.values()) == len(xi.CASES) and all(by.values())
    w = by["wgrad"]
    assert {c.M for c in w if (c.N, c.K) == (128, 128) and c.get("view", "plain") == "plain"} >= set(xi.WGRAD_M)
    assert {(c.N, c.K, c.M) for c in w} >= {(n, k, m) for n, k in ((64, 16), (192, 144)) for m in (65, 257, 3001)}
    assert {(c.N, c.K, c.M) for c in w} >= {(384, 384, 3001), (1152, 384, 777)}
    assert {c.get("view", "plain") for c in w} == {"plain", "sections", "rows", "conv1", "conv2"}
    assert {c.alpha for c in w if c.get("acc")} == set(xi.ALPHAS) and any(not c.get("db", True) for c in w)
    d = by["dora"]
    for width in xi.DORA_D:
        mine = [c for c in d if c.d_in == width]
        assert {c.M for c in mine} == set(xi.DORA_M)
        assert {(c.layout, c.yscale) for c in mine} == {(l, y) for l in xi.DORA_LAYOUTS for y in xi.YSCALES}
        assert {c.layout for c in mine if c.M == 8193} & {"q", "k", "v"}
    m = by["dora_multi"]
    assert {(c.d, len(c.order)) for c in m} == {(384, 1), (384, 2), (384, 3), (512, 1), (512, 2), (512, 3), (768, 1)}
    for key in {(c.d, len(c.order)) for c in m}:
        mine = [c for c in m if (c.d, len(c.order)) == key]
        assert {c.M for c in mine} == {31, 33, 8193}
        assert key[1] == 1 or {tuple(c.order) == tuple(sorted(c.order)) for c in mine} == {True, False}
    a = by["adapter"]
    shapes = {(c.d_in, c.d_out) for c in a}
    assert shapes == {(128, 128), (128, 512), (512, 128), (384, 384), (384, 1536), (1536, 384), (1280, 1280)}
    for s in shapes:
        mine = [c for c in a if (c.d_in, c.d_out) == s]
        assert {c.r for c in mine} == set(xi.ADAPTER_R) and {c.M for c in mine} == set(xi.ADAPTER_M)
        assert {c.layout for c in mine} == {"plain", "strided"} and {c.lora for c in mine} == {True, False}
    assert {(c.d, c.M, c.dy) for c in by["ln"]} == {(d_, m_, t) for d_ in xi.LN_D for m_ in xi.LN_M for t in ("f32", "bf16")}


def test_every_defect_is_exercised_for_every_kernel():
    """Every defect is applicable in at least one case of each kernel in which it can occur at all."""
    expect = {"wgrad": set(xi.MUTATIONS) - {"g_from_neighbour"},
              "dora": set(xi.MUTATIONS) - {"dw0_not_added", "alpha_twice"},
              "dora_multi": set(xi.MUTATIONS) - {"dw0_not_added", "alpha_twice"},
              "adapter": set(xi.MUTATIONS) - {"dw0_not_added", "alpha_twice"},
              "ln": {"row_dropped", "row_doubled", "dy_chunk_zeroed"}}
    seen = {k: set() for k in expect}
    for c in xi.CASES:
        if c.M > 600:
            continue
        for _, kernel, e, _ in _parts(c):
            seen[c.kernel] |= set(xi.applicable(kernel, e))
    assert seen == expect


def _exact_element(kernel, e, name, idx):
    """One element of the reference from int64 column sums and Fraction scales."""
    F = Fraction
    dy = e["dy"]
    if kernel == "wgrad":
        if name == "dw":
            n, k = idx
            s, base = int(np.dot(dy[:, n], e["x"][:, k])), 0 if e["dw0"] is None else int(e["dw0"][n, k])
        else:
            (n,) = idx
            s, base = int(dy[:, n].sum()), 0 if e["db0"] is None else int(e["db0"][n])
        return base + F(e["alpha"]) * s
    if kernel == "ln":
        return F(int(e["dbeta0"][idx[0]]) + int(dy[:, idx[0]].sum()))
    g = [F(e["yscale"]) * F(float(m_)) / F(float(n_)) for m_, n_ in zip(e["mag"], e["nrm"])]
    A, B, x = e["A"].astype(np.int64), e["B"].astype(np.int64), e["x"]
    if name == "dA":
        j, k = idx
        return F(e["scaling"]) * sum(g[c] * int(B[c, j]) * int(np.dot(dy[:, c], x[:, k])) for c in np.flatnonzero(B[:, j]))
    if name == "dB":
        c, j = idx
        return F(e["scaling"]) * g[c] * sum(int(A[j, k]) * int(np.dot(dy[:, c], x[:, k])) for k in np.flatnonzero(A[j]))
    (c,) = idx
    return (int(np.dot(dy[:, c], e["y"][:, c])) - int(e["bias"][c]) * int(dy[:, c].sum())) / F(float(e["mag"][c]))


@pytest.mark.parametrize("case", xi.CASES, ids=IDS)
def test_case_is_exact_order_free_and_bites(case):
    for label, kernel, e, ref in _parts(case):
        # (a) the rules, the range, and sampled elements re-derived exactly
        xi.check_ranges(kernel, e)
        rng = np.random.default_rng(len(case.id))
        for name, r in ref.items():
            f = xi.as_f32(r)
            assert float(np.abs(f).max()) < xi.LIMIT * 8      # |scale| <= 8 times an integer below 2^24
            for _ in range(3):
                idx = tuple(int(rng.integers(0, n)) for n in r.shape)
                assert Fraction(float(f[idx])) == _exact_element(kernel, e, name, idx), (label, name, idx)
            corner = tuple(n - 1 for n in r.shape)
            assert Fraction(float(f[corner])) == _exact_element(kernel, e, name, corner), (label, name, corner)
        # (b) any order of summation, in fp32, with u and v stored as bf16
        for seed in (1, 2):
            got = xi.scrambled_f32(kernel, e, seed)
            assert set(got) == set(ref)
            for name in ref:
                assert xi.mismatch(got[name], ref[name]) is None, (label, name, seed)
        # (c) every defect changes at least one output element, and the comparison says so
        for which in xi.applicable(kernel, e):
            bad = xi.reference(kernel, xi.mutate(kernel, e, which))
            hit = [name for name in ref if xi.mismatch(xi.as_f32(bad[name]), ref[name]) is not None]
            assert hit, (label, which)
            assert xi.report(hit[0], xi.as_f32(bad[hit[0]]), ref[hit[0]], (1,) * ref[hit[0]].ndim).startswith(hit[0])


def test_bf16_round_is_round_to_nearest_even():
    x = np.array([1.0, 255.0, 256.0, 257.0, 258.0, 259.0, 384.0, -385.0, 0.125 * 255, 3.0 * 2.0 ** -7], np.float32)
    want = np.array([1.0, 255.0, 256.0, 256.0, 258.0, 260.0, 384.0, -384.0, 0.125 * 255, 3.0 * 2.0 ** -7], np.float32)
    assert np.array_equal(xi.bf16_round(x), want)
    assert xi.significant_bits([255, 510, -96, 0]) == 8 and xi.significant_bits([257]) == 9


def test_wgrad_plan_restated():
    # 16385 rows: 52 slices of 320 rows, the last one 65 rows long (a full chunk and a one-row chunk)
    assert xi.wgrad_plan(16385, 128, 128) == (1, 1, 52, 320) and 16385 - 51 * 320 == 65
    assert xi.wgrad_plan(96000, 384, 384)[2:] == (56, 1728) and xi.wgrad_plan(3001, 192, 144) == (2, 2, 12, 256)
    assert xi.wgrad_plan(20161, 128, 128) == (1, 1, 64, 320) and 20161 - 63 * 320 == 1
    assert xi.wgrad_plan(1, 128, 128)[2:] == (1, 64) and xi.wgrad_plan(257, 128, 128)[2:] == (2, 192)
