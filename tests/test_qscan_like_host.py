"""The inputs, the yardstick and the envelopes of tests/test_gpu_qscan_like.py, held to what those tests assume (no GPU).

Three conditions, all on the fp64 oracle and the numpy restatements alone: the segments are mostly noise floor (so that an
error relative to a tile's own size is measured where an SNR-8 signal lives), no batch's plane choice hangs on a rounding, and
the ideal-fp32 restatements reproduce the yardstick constants every GPU limit is a multiple of."""

import numpy as np
import pytest

from . import qscan_like as ql


def test_the_row_subset_has_every_ntiles_class_and_both_ends_of_every_plane():
    rows = ql.row_subset()
    t = ql.tables()
    assert len(t.rows) == 148 and t.e_total == 49664 and len(rows) < 50
    for r0, nr in t.plane_rows:
        assert r0 in rows and r0 + nr - 1 in rows
    assert int(t.rows[:, 2].max()) == 695


def test_generator_is_deterministic_and_the_families_are_what_they_say():
    a, b = ql.segments("glitch1e3", 3), ql.segments("glitch1e3", 3)
    assert a.dtype == np.float32 and np.array_equal(a, b) and not np.array_equal(a, ql.segments("glitch1e3", 3, seed=1))
    noise = ql.segments("noise", 3).astype(np.float64)
    assert 0.9 < noise.std() < 1.1
    for fam, peak in (("glitch1e2", 1e2), ("glitch1e3", 1e3), ("glitch_hf", 1e2)):
        d = ql.segments(fam, 3) - noise
        # (0.55 s falls between two samples: the largest sample is a little under the envelope's peak)
        assert 0.9 < np.abs(d).max() / peak <= 1.0 and abs(int(np.abs(d[0]).argmax()) - int(0.55 * ql.FS)) <= 7
    d = ql.segments("glitch_edge", 1)[0] - noise[0]
    assert np.abs(d[:4]).max() > 50 and np.abs(d[200:]).max() < 1e-3          # cut off at the segment's first sample
    assert np.abs(ql.segments("offset", 3) - noise - 50.0).max() < 1e-5
    g = ql.segments("gated", 2)
    assert (g[:, 614:1228] == 0).all() and (g[:, :614] != 0).all() and (g[:, 1228:] != 0).all()
    c = ql.segments("chirp", 5).astype(np.float64) - ql.segments("noise", 5)
    assert [round(float(np.abs(ci).max())) for ci in c] == [3, 5, 7, 9, 11]
    m = ql.mixed_batch()
    assert m.shape == (9, 2048) and np.array_equal(m[3], ql.segments("glitch1e3", 9)[3])


@pytest.mark.parametrize("family", ql.FAMILIES)
def test_most_tiles_of_every_row_are_noise_floor(family):
    """At least 60 % of the tiles of every (row, item) have 0.1 <= e_ref <= 10.  Seed 0: the lowest share is 0.656
    (glitch1e3), 0.70 .. 0.84 in the other families.

    `gated` cannot meet this per row at any seed: 30 % of its samples are exactly zero, so about 30 % of every row's tiles
    lie far below 0.1 by construction (those tiles are what the family is for: they sit on the envelope's floor) and the rest
    is quiet at the 93 % of plain noise -- 0.64 on average, 0.51 .. 0.57 in the worst of the 740 (row, item) pairs on each of
    seeds 0 .. 11.  For it the 60 % is asserted over each item's whole tiling, with no (row, item) under 50 %."""
    _, _, flat, _ = ql.family_case(family)
    q = np.stack([ql.quiet_fraction(e) for e in flat])                      # [148 rows, items]
    n = ql.tables().rows[:, 1].astype(np.float64)
    per_item = (q * n[:, None]).sum(axis=0) / n.sum()
    print(f"{family}: quiet share, worst (row, item) {q.min():.3f}, worst item over its tiling {per_item.min():.3f}")
    if family == "gated":
        assert per_item.min() >= 0.6 and q.min() >= 0.5
    else:
        assert q.min() >= 0.6


def _gap(maxima):
    s = np.sort(maxima)[::-1]
    return (s[0] - s[1]) / s[0]


def test_no_plane_choice_is_decided_by_rounding():
    """In every multi-item batch the GPU tests run, the oracle's two largest plane maxima differ by more than 1e-3."""
    batches = {f: ql.family_case(f)[3] for f in ql.FAMILIES}
    mixed = ql.mixed_batch()
    with_zero, without = ql.zero_row_batches()
    batches["mixed"] = ql.oracle(mixed)[3]
    batches["glitch1e2 of mixed alone"] = ql.oracle(mixed[2:3])[3]
    batches["without the zero row"] = ql.oracle(without)[3]
    for name, maxima in batches.items():
        print(f"{name}: plane {int(np.argmax(maxima))}, gap {_gap(maxima):.3f}")
        assert _gap(maxima) > 1e-3, name
    # the bit-identity tests compare maps across these: they must choose the same plane
    assert np.argmax(batches["mixed"]) == np.argmax(batches["glitch1e2 of mixed alone"])
    # numpy lets the zero row's NaN win the argmax; the kernels' policy is the plane of the other rows
    with np.errstate(invalid="ignore"):
        assert np.isnan(ql.oracle(with_zero)[3]).all()


@pytest.mark.parametrize("family", ql.FAMILIES)
def test_ideal_fp32_reproduces_the_tile_yardstick(family):
    x, _, flat, _ = ql.family_case(family)
    rows = ql.row_subset()
    ideal = ql.ideal_fp32(x, rows)
    rms, worst = ql.rel_errors([ideal[r] for r in rows], [flat[r] for r in rows], [ql.e_tile(flat[r]) for r in rows])
    y_rms, y_worst = ql.TILE_YARDSTICK[family]
    print(f'    "{family}": ({rms:.3e}, {worst:.3e}),')
    assert abs(rms / y_rms - 1) <= 0.1 and abs(worst / y_worst - 1) <= 0.1


def test_ideal_interp_fp32_reproduces_the_interpolation_yardstick():
    _, _, flat, _ = ql.oracle(ql.interp_batch())
    flat32 = [e.astype(np.float32) for e in flat]
    for shape in ql.INTERP_SHAPES:
        worst = 0.0
        for p in range(len(ql.tables().plane_rows)):
            F, T = ql.interp_shape(shape, p)
            r32 = ql.plane_energies(flat32, p)
            r64 = [e.astype(np.float64) for e in r32]
            got = ql.ideal_interp_fp32(r32, F, T)
            assert got.shape == (2, F, T) and got.dtype == np.float32
            worst = max(worst, ql.rel_errors(got, ql.oq.interpolate_plane(r64, (F, T)), ql.e_pix(r64, (F, T)))[1])
        print(f"    {shape!r}: {worst:.3e},")
        assert abs(worst / ql.INTERP_YARDSTICK[shape] - 1) <= 0.1, shape


def test_the_source_index_is_exact_at_the_production_shapes_and_not_at_300():
    """(128, 128) and (512, 512): every time ratio is a power of two and the fp32 source index is the fp64 one; at T = 300
    an index near 2048 carries an ulp of 1.2e-4."""
    f32 = np.float32
    for T in (128, 512, 300):
        worst = 0.0
        for n in (128, 256, 512, 1024, 2048):
            src32 = (np.arange(T, dtype=f32) + f32(0.5)) * (f32(n) / f32(T)) - f32(0.5)
            src = (np.arange(T) + 0.5) * (n / T) - 0.5
            worst = max(worst, float(np.abs(src32.astype(np.float64) - src).max()))
        assert (worst == 0.0) if T != 300 else (1e-5 < worst < 5e-4), (T, worst)


def test_the_envelope_is_the_interpolation_with_absolute_weights():
    """E_pix >= |ref| everywhere, with equality where a pixel's 16 weights share a sign and no tile is under the floor; the
    oracle's new keyword arguments leave its map unchanged."""
    x, best, flat, _ = ql.family_case("glitch1e2")
    rows = ql.plane_energies(flat, best)
    ref = ql.oq.interpolate_plane(rows, (80, 300))
    assert np.array_equal(ref, ql.oq.qscan(x.astype(np.float64), spectrogram_shape=(80, 300)))
    out, plane = ql.oq.qscan(x.astype(np.float64), spectrogram_shape=(80, 300), return_plane=True)
    assert plane == best and np.array_equal(out, ref)
    env = ql.e_pix(rows, (80, 300))
    assert (env >= np.abs(ref) * (1 - 1e-12)).all() and (env >= ql.FLOOR * (1 - 1e-12)).all()
    same = ql.oq.interpolate_plane(rows, (len(rows), 2048))              # nr == F and, on the widest rows, n == T
    assert same.shape == (x.shape[0], len(rows), 2048)
