"""The detector-like inputs of tests/test_gpu_whiten_detector_like.py, checked against the fp64 oracle alone (no GPU).

Four conditions on every (case, size) the GPU tests use: the strain is as steep as real detector strain, the oracle is
well conditioned on it (so the GPU tests compare against a meaningful number), an fp32 cast of the input cannot meet the
project's per-sample bound (so the GPU tests have teeth) and the whitened output has the usual standard deviation."""

import numpy as np
import pytest

from oracle import whiten as ow

from . import detector_like as dl

BOUND = 2e-3 * 32      # the per-sample bound of test_gpu_inference.py::test_whiten_matches_the_pycbc_restatement


def _pow2_scaled_fp32(x):
    """x brought to unit scale by an exact power of two, then rounded to fp32: what an fp32 front end would see."""
    scale = 2.0 ** (-np.floor(np.log2(np.abs(x).max())))
    return (x * scale).astype(np.float32).astype(np.float64)


@pytest.mark.parametrize("n", dl.SIZES)
@pytest.mark.parametrize("wall,lines,glitch", [(w, l, False) for w, l in dl.CASES] + [(4, True, True)])
def test_inputs_are_steep_well_conditioned_and_beyond_an_fp32_cast(wall, lines, glitch, n):
    for row, x in enumerate(dl.pair(n, dl.SEED, wall, lines, glitch)):
        assert x.dtype == np.float64
        # (a) ASD range >= 1e6, in-band rms 2e-6 .. 1e-4 of the peak
        rng_asd = dl.asd_range(n, wall, lines)
        ratio = dl.in_band(x).std() / np.abs(x).max()
        assert rng_asd >= 1e6, rng_asd
        assert 2e-6 <= ratio <= 1e-4, ratio
        ref = ow.whiten(x)
        # (b) conditioning: a 1e-13 relative perturbation of the input moves no whitened sample by more than 1e-4
        pert = x * (1 + 1e-13 * np.random.default_rng(5).standard_normal(n))
        cond = np.abs(ow.whiten(pert) - ref).max()
        assert cond <= 1e-4, cond
        # (c) teeth: the oracle itself on the fp32-rounded input misses the bound
        teeth = np.abs(ow.whiten(_pow2_scaled_fp32(x)) - ref).max()
        assert teeth > BOUND, teeth
        # (d) whitened noise has standard deviation about sqrt(fs / 2) = 32 (a glitch's own +- 0.5 s are left out: whitened,
        # its peak is about 490 of those and would dominate the figure)
        keep = np.abs(np.arange(n - 512) + 256 - dl.glitch_centre(n)) > 1024 if glitch else slice(None)
        std = ref[keep].std()
        assert 20 < std < 40, std
        print(f"wall={wall} lines={lines} glitch={glitch} n={n} row {row}: ASD range {rng_asd:.2e}, in-band rms / peak "
              f"{ratio:.2e}, conditioning {cond:.1e}, fp32-cast error {teeth:.3f}, std {std:.2f}")


def test_the_glitch_stands_200_times_above_the_floor_in_a_minority_of_segments():
    for n in dl.SIZES:
        clean, loud = dl.strain(n, dl.SEED), dl.strain(n, dl.SEED, glitch=True)
        g = loud - clean
        assert 150 < np.abs(g).max() / dl.in_band(clean).std() <= 200.0 * (1 + 1e-12)
        seg_len, stride = 1024, 512
        n_seg, start = ow.welch_segments(n, seg_len, stride)
        hit = [i for i in range(n_seg) if np.abs(g[start + i * stride: start + i * stride + seg_len]).max() > 1e-6 * np.abs(g).max()]
        assert 1 <= len(hit) <= 3 and n_seg >= 127
        # whitened, the burst is far above the noise
        w = ow.whiten(loud)
        assert np.abs(w).max() > 50 * 32


def test_generator_is_deterministic_per_seed():
    a, b, c = dl.strain(4096, 3), dl.strain(4096, 3), dl.strain(4096, 4)
    assert np.array_equal(a, b) and not np.array_equal(a, c)
    p = dl.pair(4096, 3)
    assert p.shape == (2, 4096) and 1e-4 < np.abs(p[1]).max() / np.abs(p[0]).max() < 1e-3


def test_the_search_harness_reads_raw_strain_at_its_stored_width(tmp_path):
    """harness/run_inference.py read float64 segments into float32, the very cast condition (c) shows to be too lossy: the
    strain must reach DeviceSegmentSlicer(white=False), and through it whiten, as the file holds it."""
    import importlib.util
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("run_inference", os.path.join(root, "harness", "run_inference.py"))
    ri = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ri)
    x = dl.pair(4096, dl.SEED)
    arrays = {f"{d}/7": x[i] for i, d in enumerate(ri.DETECTORS)}
    arrays["7/start_time"], arrays["7/delta_t"] = 7.0, 1.0 / dl.FS
    src = str(tmp_path / "raw.npz")
    np.savez(src, **arrays)
    got, st, dt = ri.read_segments(src)["7"]
    assert got.dtype == np.float64 and np.array_equal(got, x) and (st, dt) == (7.0, 1.0 / dl.FS)


@pytest.mark.parametrize("wall,lines,taps", [(0, False, 513), (4, True, 1025), (6, True, 1025)])
def test_design_filter_keeps_enough_taps_for_a_steep_spectrum(wall, lines, taps):
    """design_filter is plain torch and runs here: with its taps, an exact (fp64, numpy) circular correlation must stay
    within the per-sample bound of the oracle.  The l1 test alone (leak switched off) stops at 513 taps and, under the
    lined cases' wall, misses it whatever the arithmetic."""
    import torch
    from gw_whisper_amd.whiten import design_filter
    n = dl.SIZES[0]
    x = dl.strain(n, dl.SEED, wall, lines)
    x = x * 2.0 ** (-np.floor(np.log2(np.abs(x).max())))
    ref, psd_w = ow.whiten(x, return_psd=True)

    def filtered(**kw):
        g, K = design_filter(torch.from_numpy(psd_w)[None], 2.0, n, 1.0 / dl.FS, 512, **kw)
        idx = (np.arange(n - 512 + 2 * K) + 256 - K) % n
        return np.correlate(x[idx], g[0, :2 * K + 1].numpy(), "valid"), 2 * K + 1
    got, kept = filtered()
    err = np.abs(got - ref).max()
    short, kept_l1 = filtered(leak=np.inf)
    err_l1 = np.abs(short - ref).max()
    print(f"wall={wall} lines={lines}: {kept} taps, max |err| {err:.3e}; by the l1 test alone {kept_l1} taps, {err_l1:.3e}")
    assert kept == taps and err < BOUND
    assert kept_l1 == 513
    if lines:
        assert err_l1 > BOUND
