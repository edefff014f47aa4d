"""CPU-side checks of the signal-vs-noise evaluation (gw_whisper_amd/roc.py, csrc/roc.hip) against
tests/golden/roc_bootstrap.npz, which tools/make_roc_golden.py wrote by running the reference's own
``bootstrap_roc_curve`` and the metric statements of its ``evaluate`` on scikit-learn: the numpy restatement of the device
algorithm (tests/roc_helpers.py) reproduces the band bit for bit, the resample indices regenerate from the seed, the
``drop_intermediate`` post-processing equals sklearn's vertices, every new entry point refuses bad arguments before any HIP
call, and the evaluation program lists its flags."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from gw_whisper_amd import GwwError, lib, ops, roc

from . import roc_helpers as rh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def gold():
    return np.load(rh.GOLD)


def test_golden_cases_are_the_documented_ones(gold):
    assert [tuple(c) for c in gold["cases"].tolist()] == list(rh.CASES)
    for ci, (n, R) in enumerate(rh.CASES):
        assert gold[f"c{ci}_scores"].shape == (n,) and gold[f"c{ci}_scores"].dtype == np.float32
        assert int(gold[f"c{ci}_R"]) == R and gold[f"c{ci}_mean_tpr"].shape == (500,)
    # heavy ties at both ends in the larger cases
    assert (gold["c3_scores"] == 0).sum() > 1000 and (gold["c3_scores"] == 1).sum() > 1000


@pytest.mark.parametrize("ci", range(len(rh.CASES)))
def test_restatement_reproduces_the_reference_band_bit_for_bit(gold, ci):
    """max |delta| = 0.0 for mean_tpr and std_tpr: the algorithm of csrc/roc.hip, in numpy, IS the reference's
    resample + roc_curve + np.interp + np.mean / np.std.  The regenerated indices match the fixture's checksums."""
    n, R = rh.CASES[ci]
    scores, labels = gold[f"c{ci}_scores"], gold[f"c{ci}_labels"].astype(np.float32)
    idx = rh.draw_indices(int(gold[f"c{ci}_seed"]), R, n)
    assert rh.checksums(idx) == (int(gold[f"c{ci}_idx_xor"]), int(gold[f"c{ci}_idx_sum"]))
    _, rank, pos, gend = rh.sort_desc(scores, labels)
    rows, valid = rh.bootstrap_rows(rank, pos, gend, idx)
    assert valid.all()
    mean, std = rh.band(rows, valid)
    d_mean, d_std = np.abs(mean - gold[f"c{ci}_mean_tpr"]).max(), np.abs(std - gold[f"c{ci}_std_tpr"]).max()
    print(f"case {ci}: max |mean - golden| = {d_mean}, max |std - golden| = {d_std}")
    assert d_mean == 0.0 and d_std == 0.0
    assert std[-1] == 0.0 and mean[-1] == 1.0          # every replicate ends at (1, 1)


@pytest.mark.parametrize("ci", range(len(rh.CASES)))
def test_curve_and_drop_intermediate_equal_sklearn(gold, ci):
    scores, labels = gold[f"c{ci}_scores"], gold[f"c{ci}_labels"].astype(np.float32)
    _, _, pos, gend = rh.sort_desc(scores, labels)
    fps, tps, fpr, tpr, P, Nneg, auc = rh.curve(pos, gend)
    assert np.array_equal(fpr, gold[f"c{ci}_fpr_all"]) and np.array_equal(tpr, gold[f"c{ci}_tpr_all"])
    f, t = roc.drop_collinear(fps, tps)
    assert np.array_equal(f / np.float64(Nneg), gold[f"c{ci}_fpr_drop"])
    assert np.array_equal(t / np.float64(P), gold[f"c{ci}_tpr_drop"])
    # sklearn sums <= 2e4 fp64 trapezoids: its own rounding stays below 2e4 * 2^-53 ~ 2e-12
    assert abs(float(auc) - float(gold[f"c{ci}_auc"])) <= 1e-12


def test_drop_collinear_small_curves():
    for fps, tps in (([0, 1], [0, 1]), ([0, 0, 1], [0, 1, 1]), ([0, 1, 2, 3], [0, 1, 2, 3]), ([0, 0, 0, 2, 2], [0, 1, 2, 2, 3])):
        f, t = roc.drop_collinear(np.asarray(fps), np.asarray(tps))
        assert f[0] == 0 and t[0] == 0 and f[-1] == fps[-1] and t[-1] == tps[-1]
    f, t = roc.drop_collinear(np.asarray([0, 1, 2, 3]), np.asarray([0, 1, 2, 3]))
    assert f.tolist() == [0, 1, 3] and t.tolist() == [0, 1, 3]      # sklearn keeps the first vertex behind the origin


def test_tile_constant_and_workspace_sizes():
    L = lib()
    assert L.gww_roc_tile() == ops.ROC_TILE == 16384
    assert L.gww_roc_curve_workspace_bytes(1000) == 4000
    assert L.gww_roc_bootstrap_workspace_bytes(7, 1000) == 7 * 1000 * 8      # one row of 2 x uint32 x N per replicate
    assert L.gww_roc_sort_workspace_bytes(1000) >= 4 * 4 * 1000 + 256 * 4
    for bad in (1, (1 << 24) + 1):
        assert L.gww_roc_sort_workspace_bytes(bad) == 0 and L.gww_roc_curve_workspace_bytes(bad) == 0
        assert L.gww_roc_bootstrap_workspace_bytes(1, bad) == 0


def test_argument_errors_without_gpu():
    """Every check comes before any HIP call: N = 1, N > 2^24, Q = 0, Q > 1024, a workspace one byte short, NULL."""
    L = lib()
    p = 1 << 12                 # a non-NULL, aligned stand-in: nothing is dereferenced before the checks
    big = (1 << 24) + 1
    err = L.gww_last_error
    ws = L.gww_roc_sort_workspace_bytes(100)
    assert L.gww_roc_sort_f32(p, p, 1, p, p, p, p, p, p, p, 1 << 30, None) == -1 and b"N=1" in err()
    assert L.gww_roc_sort_f32(p, p, big, p, p, p, p, p, p, p, 1 << 40, None) == -1 and b"N=" in err()
    assert L.gww_roc_sort_f32(p, p, 100, p, p, p, p, p, p, p, ws - 1, None) == -1 and b"workspace" in err()
    assert L.gww_roc_sort_f32(p, None, 100, p, p, p, p, p, p, p, ws, None) == -1 and b"NULL" in err()
    assert L.gww_roc_sort_f32(p, p, 100, p, p, p, p, p, p, None, ws, None) == -1 and b"NULL" in err()
    ws = L.gww_roc_curve_workspace_bytes(100)
    assert L.gww_roc_curve_f64(p, p, p, 1, p, p, p, p, p, p, p, 1 << 30, None) == -1 and b"N=1" in err()
    assert L.gww_roc_curve_f64(p, p, p, big, p, p, p, p, p, p, p, 1 << 40, None) == -1 and b"N=" in err()
    assert L.gww_roc_curve_f64(p, p, p, 100, p, p, p, p, p, p, p, ws - 1, None) == -1 and b"workspace" in err()
    assert L.gww_roc_curve_f64(p, p, None, 100, p, p, p, p, p, p, p, ws, None) == -1 and b"NULL" in err()
    ws = L.gww_roc_bootstrap_workspace_bytes(3, 100)
    boot = L.gww_roc_bootstrap_tpr_f64
    assert boot(p, p, p, p, p, 3, 1, p, 500, p, p, p, 1 << 30, None) == -1 and b"N=1" in err()
    assert boot(p, p, p, p, p, 3, big, p, 500, p, p, p, 1 << 40, None) == -1 and b"N=" in err()
    assert boot(p, p, p, p, p, 0, 100, p, 500, p, p, p, ws, None) == -1 and b"Rc=0" in err()
    assert boot(p, p, p, p, p, 3, 100, p, 0, p, p, p, ws, None) == -1 and b"Q=0" in err()
    assert boot(p, p, p, p, p, 3, 100, p, 1025, p, p, p, ws, None) == -1 and b"Q=1025" in err()
    assert boot(p, p, p, p, p, 3, 100, p, 500, p, p, p, ws - 1, None) == -1 and b"workspace" in err()
    assert boot(p, p, p, p, None, 3, 100, p, 500, p, p, p, ws, None) == -1 and b"NULL" in err()
    assert L.gww_roc_band_f64(p, p, 0, 500, p, p, p, None) == -1 and b"R=0" in err()
    assert L.gww_roc_band_f64(p, p, 10, 0, p, p, p, None) == -1 and b"Q=0" in err()
    assert L.gww_roc_band_f64(p, p, 10, 1025, p, p, p, None) == -1 and b"Q=1025" in err()
    assert L.gww_roc_band_f64(p, None, 10, 500, p, p, p, None) == -1 and b"NULL" in err()
    acc = L.gww_binary_eval_accumulate
    assert acc(p, p, 0, p, 0, 10, p, p, p, None) == -1 and b"B=0" in err()
    assert acc(p, p, 8, p, 3, 10, p, p, p, None) == -1 and b"offset=3" in err()
    assert acc(p, p, 8, p, -1, 10, p, p, p, None) == -1 and b"offset" in err()
    assert acc(p, None, 8, p, 0, 10, p, p, p, None) == -1 and b"NULL" in err()


def test_cpu_tensors_and_bad_shapes_are_refused():
    s, y = torch.zeros(8), torch.zeros(8)
    with pytest.raises(GwwError, match="GPU"):
        ops.roc_sort(s, y)
    with pytest.raises(GwwError, match="GPU"):
        ops.roc_curve(torch.zeros(8, dtype=torch.uint8), torch.zeros(8, dtype=torch.int32), torch.zeros(1, dtype=torch.int32))
    with pytest.raises(GwwError, match="GPU"):
        ops.roc_band(torch.zeros(3, 5, dtype=torch.float64), torch.ones(3, dtype=torch.uint8))
    with pytest.raises(GwwError, match="GPU"):
        ops.binary_eval_accumulate(s, y, s, 0, torch.zeros(1, dtype=torch.float64), torch.zeros(1, dtype=torch.int64),
                                   torch.zeros(2, 2, dtype=torch.int64))
    with pytest.raises(GwwError, match="grid"):
        roc.RocEvaluator(grid=np.linspace(0.0, 1.0, 5))         # 0 is outside (0, 1]
    with pytest.raises(GwwError, match="grid"):
        roc.RocEvaluator(grid=np.linspace(0.1, 1.0, 1025))
    ev = roc.RocEvaluator(num_bootstrap=1000, chunk_bytes=1 << 20)
    assert ev.grid.shape == (500,) and np.array_equal(ev.grid, rh.GRID)
    assert ev.chunk_rows(20000) == 4 and ev.chunk_rows(10 ** 7) == 1 and roc.RocEvaluator(7).chunk_rows(2) == 7


def test_run_evaluation_lists_its_flags():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "harness", "run_evaluation.py"), "--help"], check=True,
                         capture_output=True, text=True).stdout
    for flag in ("--model_type", "--lora_weights_path", "--dense_layers_path", "--dataset_paths", "--synthetic", "--seed",
                 "--encoder", "--batch_size", "--num_bootstrap", "--out_dir"):
        assert flag in out, flag
