"""GPU checks of csrc/roc.hip and gw_whisper_amd/roc.py: the sort against numpy's stable sort, the curve against
sklearn's ``roc_curve(drop_intermediate=False)`` and an integer AUC, the bootstrap rows against the numpy restatement of
tests/roc_helpers.py bit for bit (tile carry included), the band against the reference's own ``bootstrap_roc_curve``
(tests/golden/roc_bootstrap.npz), degenerate resamples, chunking, the binary evaluation accumulate against torch on the
CPU, and ``harness/run_evaluation.py`` end to end on a model ``run_train.py`` saved."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from . import roc_helpers as rh

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def T():
    import torch
    assert torch.cuda.is_available()
    return torch


@pytest.fixture(scope="module")
def gold():
    return np.load(rh.GOLD)


def _sort(T, scores, labels):
    from gw_whisper_amd import ops
    return ops.roc_sort(T.from_numpy(np.ascontiguousarray(scores, np.float32)).cuda(),
                        T.from_numpy(np.ascontiguousarray(labels, np.float32)).cuda())


def _score_kinds(n, seed):
    rng = np.random.default_rng(seed)
    rand = rng.standard_normal(n).astype(np.float32)
    rand[rng.integers(0, n, n // 3)] = rand[0]                    # some ties
    zeros = np.where(rng.random(n) < 0.5, 0.0, -0.0).astype(np.float32)
    zeros[0], zeros[-1] = 0.0, -0.0
    inf = rand.copy()
    inf[0], inf[-1] = np.inf, -np.inf
    if n > 4:
        inf[n // 2], inf[n // 2 + 1] = -np.inf, np.inf
    asc = np.sort(rand)
    return {"random": rand, "all_equal": np.full(n, 0.25, np.float32), "signed_zeros": zeros, "inf": inf, "ascending": asc,
            "descending": asc[::-1].copy()}


@pytest.mark.parametrize("n", [2, 3, 63, 64, 65, 255, 257, 4096, 4097, 8193])
def test_sort(T, gww, n):
    labels = (np.random.default_rng(n).random(n) < 0.5).astype(np.float32)
    for kind, scores in _score_kinds(n, 100 + n).items():
        order, rank, pos, gend, G, n_nan = (t.cpu().numpy() for t in _sort(T, scores, labels))
        ro, rr, rp, rg = rh.sort_desc(scores, labels)
        s = scores[order]
        assert (s[:-1] >= s[1:]).all(), kind
        assert np.array_equal(np.sort(order), np.arange(n)) and np.array_equal(rank[order], np.arange(n)), kind
        assert np.array_equal(order, ro) and np.array_equal(rank, rr), kind        # stable: ties stay in index order
        assert np.array_equal(pos, rp), kind
        assert int(G[0]) == len(rg) and np.array_equal(gend[:len(rg)], rg), kind
        assert int(n_nan[0]) == 0
        if kind in ("all_equal", "signed_zeros"):
            assert int(G[0]) == 1 and gend[0] == n - 1, kind


def test_nan_is_counted_and_refused(T, gww):
    from gw_whisper_amd import roc
    scores, labels = rh.saturating_scores(65, 2.0, 5)
    scores[17] = np.nan
    assert int(_sort(T, scores, labels)[5].item()) == 1
    with pytest.raises(gww.GwwError, match="NaN"):
        roc.RocEvaluator(num_bootstrap=2, seed=0)(scores, labels)
    with pytest.raises(gww.GwwError, match="one class"):
        roc.RocEvaluator(num_bootstrap=2, seed=0)(np.linspace(0, 1, 9, dtype=np.float32), np.ones(9, np.float32))


def _curve(T, scores, labels):
    from gw_whisper_amd import ops
    _, _, pos, gend, G, _ = _sort(T, scores, labels)
    fps, tps, fpr, tpr, counts, auc = ops.roc_curve(pos, gend, G)
    g = int(G.item())
    return (fps[:g + 1].cpu().numpy(), tps[:g + 1].cpu().numpy(), fpr[:g + 1].cpu().numpy(), tpr[:g + 1].cpu().numpy(),
            counts.cpu().numpy(), float(auc.item()))


@pytest.mark.parametrize("ci", range(len(rh.CASES)))
def test_curve_on_the_golden_cases(T, gww, gold, ci):
    scores, labels = gold[f"c{ci}_scores"], gold[f"c{ci}_labels"].astype(np.float32)
    fps, tps, fpr, tpr, counts, auc = _curve(T, scores, labels)
    _, _, rp, rg = rh.sort_desc(scores, labels)
    rfps, rtps, _, _, P, Nneg, frac = rh.curve(rp, rg)
    assert np.array_equal(fps, rfps) and np.array_equal(tps, rtps) and counts.tolist() == [P, Nneg]
    assert np.array_equal(fpr, gold[f"c{ci}_fpr_all"]) and np.array_equal(tpr, gold[f"c{ci}_tpr_all"])
    assert auc == frac.numerator / frac.denominator            # int / int in Python is correctly rounded: one division
    d = abs(auc - float(gold[f"c{ci}_auc"]))
    print(f"case {ci}: |auc - roc_auc_score| = {d}")
    assert d <= 1e-12


def test_curve_n2(T, gww):
    from sklearn.metrics import roc_curve
    for scores, labels in (([0.9, 0.1], [1, 0]), ([0.1, 0.9], [1, 0]), ([0.5, 0.5], [0, 1])):
        scores, labels = np.asarray(scores, np.float32), np.asarray(labels, np.float32)
        fps, tps, fpr, tpr, counts, auc = _curve(T, scores, labels)
        rf, rt, _ = roc_curve(labels, scores, drop_intermediate=False)
        assert np.array_equal(fpr, rf) and np.array_equal(tpr, rt) and counts.tolist() == [1, 1]
        assert auc == (1.0 if scores[0] > scores[1] else 0.0 if scores[0] < scores[1] else 0.5)


def _indices(n, rank, pos, seed):
    """R = 8 rows: random draws, the identity, all draws one positive / one negative sample (degenerate), draws from the
    middle, the front and the back third of the sorted order only, and one positive + one negative sample alternating:
    zero-multiplicity runs at the front, in the middle and at the end."""
    rng = np.random.default_rng(seed)
    order = np.argsort(rank)
    one_pos, one_neg = order[np.flatnonzero(pos == 1)[0]], order[np.flatnonzero(pos == 0)[-1]]
    rows = [rng.integers(0, n, n), np.arange(n), np.full(n, one_pos), np.full(n, one_neg)]
    for lo, hi in ((n // 3, max(2 * n // 3, n // 3 + 1)), (0, max(n // 3, 1)), (2 * n // 3, n)):
        rows.append(order[rng.integers(lo, hi, n)])
    rows.append(np.where(np.arange(n) % 2 == 0, one_pos, one_neg))
    return np.stack(rows).astype(np.int64)


def _tile():
    from gw_whisper_amd import ops
    return ops.ROC_TILE


@pytest.mark.parametrize("n", [2, 3, 64, 257, "T-1", "T", "T+1", "2T+5"])
def test_bootstrap_rows_equal_the_restatement(T, gww, n):
    """max |delta| = 0.0 against tests/roc_helpers.py, NaN rows of degenerate replicates included; the last four sizes
    exercise the tile carry."""
    from gw_whisper_amd import ops
    if isinstance(n, str):
        n = {"T-1": _tile() - 1, "T": _tile(), "T+1": _tile() + 1, "2T+5": 2 * _tile() + 5}[n]
    if n == 2:
        scores, labels = np.asarray([0.2, 0.7], np.float32), np.asarray([0, 1], np.float32)
    elif n == 3:
        scores, labels = np.asarray([0.2, 0.7, 0.7], np.float32), np.asarray([0, 1, 0], np.float32)
    else:
        scores, labels = rh.saturating_scores(n, 2.0, n)
    order, rank, pos, gend, G, _ = _sort(T, scores, labels)
    _, rr, rp, rg = rh.sort_desc(scores, labels)
    idx = _indices(n, rr, rp, n + 1)
    ref, ref_valid = rh.bootstrap_rows(rr, rp, rg, idx)
    assert ref_valid[[1, 2, 3, 7]].tolist() == [1, 0, 0, 1]
    grid = T.from_numpy(rh.GRID).cuda()
    tpr, valid = ops.roc_bootstrap_tpr(rank, pos, gend, G, T.from_numpy(idx.astype(np.int32)).cuda(), grid)
    tpr, valid = tpr.cpu().numpy(), valid.cpu().numpy()
    assert np.array_equal(valid, ref_valid)
    ok = ref_valid != 0
    d = np.abs(tpr[ok] - ref[ok]).max()
    print(f"N={n}: max |tpr - restatement| = {d}")
    assert d == 0.0 and np.isnan(tpr[~ok]).all()
    assert np.array_equal(tpr, ref, equal_nan=True)
    # Q = 1 with grid = [1.0]: every valid replicate ends at TPR 1
    one, v1 = ops.roc_bootstrap_tpr(rank, pos, gend, G, T.from_numpy(idx.astype(np.int32)).cuda(),
                                    T.tensor([1.0], dtype=T.float64, device="cuda"))
    assert np.array_equal(v1.cpu().numpy(), ref_valid) and (one.cpu().numpy()[ok] == 1.0).all()


@pytest.mark.parametrize("ci", range(len(rh.CASES)))
def test_band_equals_the_reference(T, gww, gold, ci):
    """RocEvaluator with the fixture's seed draws the reference's resamples; the band equals the reference's
    ``bootstrap_roc_curve`` within 1e-13 = R * 2^-53 for R <= 1000 (expected: 0, the rows are exact and the band sums in
    numpy's order), the curve equals ``roc_curve``'s default vertices, the AUC ``roc_auc_score`` within 1e-12."""
    from gw_whisper_amd import roc
    n, R = rh.CASES[ci]
    scores, labels = gold[f"c{ci}_scores"], gold[f"c{ci}_labels"].astype(np.float32)
    out = roc.RocEvaluator(num_bootstrap=R, seed=int(gold[f"c{ci}_seed"]))(scores, labels)
    d_mean = np.abs(out["mean_tpr"] - gold[f"c{ci}_mean_tpr"]).max()
    d_std = np.abs(out["std_tpr"] - gold[f"c{ci}_std_tpr"]).max()
    print(f"case {ci} (N={n}, R={R}): max |mean - golden| = {d_mean}, max |std - golden| = {d_std}")
    assert d_mean <= 1e-13 and d_std <= 1e-13
    assert out["n_valid"] == R and out["n_nan"] == 0 and out["std_tpr"][-1] == 0.0 and out["mean_tpr"][-1] == 1.0
    assert np.array_equal(out["grid"], rh.GRID)
    assert np.array_equal(out["fpr"], gold[f"c{ci}_fpr_drop"]) and np.array_equal(out["tpr"], gold[f"c{ci}_tpr_drop"])
    assert abs(out["auc"] - float(gold[f"c{ci}_auc"])) <= 1e-12
    full = roc.RocEvaluator(num_bootstrap=1, seed=0)(scores, labels, drop_intermediate=False)
    assert np.array_equal(full["fpr"], gold[f"c{ci}_fpr_all"]) and np.array_equal(full["tpr"], gold[f"c{ci}_tpr_all"])


def test_degenerate_replicates(T, gww):
    from gw_whisper_amd import ops, roc
    scores, labels = np.asarray([0.8, 0.3], np.float32), np.asarray([1, 0], np.float32)
    idx = np.asarray([[0, 1], [1, 0], [0, 0], [1, 1]])
    order, rank, pos, gend, G, _ = _sort(T, scores, labels)
    tpr, valid = ops.roc_bootstrap_tpr(rank, pos, gend, G, T.from_numpy(idx.astype(np.int32)).cuda(), T.from_numpy(rh.GRID).cuda())
    assert valid.cpu().tolist() == [1, 1, 0, 0]
    rows = tpr.cpu().numpy()
    assert np.isnan(rows[2:]).all() and np.isfinite(rows[:2]).all()
    mean, std, n_valid = ops.roc_band(tpr, valid)
    assert int(n_valid.item()) == 2
    assert np.array_equal(mean.cpu().numpy(), np.mean(rows[:2], axis=0)) and np.array_equal(std.cpu().numpy(), np.std(rows[:2], axis=0))
    out = roc.RocEvaluator()(scores, labels, indices=idx)
    assert out["n_valid"] == 2 and np.array_equal(out["mean_tpr"], np.mean(rows[:2], axis=0))
    # no valid replicate at all: NaN band, n_valid = 0
    out = roc.RocEvaluator()(scores, labels, indices=idx[2:])
    assert out["n_valid"] == 0 and np.isnan(out["mean_tpr"]).all() and np.isnan(out["std_tpr"]).all()


def test_chunking_and_reproducibility(T, gww):
    from gw_whisper_amd import roc
    n, R = 300, 37
    scores, labels = rh.saturating_scores(n, 1.5, 77)
    outs = []
    for rows in (1, 5, 37, 37):
        ev = roc.RocEvaluator(num_bootstrap=R, seed=9, chunk_bytes=rows * 12 * n)
        assert ev.chunk_rows(n) == rows
        outs.append(ev(scores, labels))
    for o in outs[1:]:
        for k in ("mean_tpr", "std_tpr", "fpr", "tpr"):
            assert np.array_equal(o[k], outs[0][k]), k
        assert o["auc"] == outs[0]["auc"] and o["n_valid"] == outs[0]["n_valid"]
    idx = rh.draw_indices(9, R, n)
    assert np.array_equal(roc.RocEvaluator(chunk_bytes=7 * 12 * n)(scores, labels, indices=idx)["mean_tpr"], outs[0]["mean_tpr"])
    _, rr, rp, rg = rh.sort_desc(scores, labels)
    mean, std = rh.band(*rh.bootstrap_rows(rr, rp, rg, idx))
    assert np.array_equal(outs[0]["mean_tpr"], mean) and np.array_equal(outs[0]["std_tpr"], std)


@pytest.mark.parametrize("B", [1, 63, 64, 65, 257])
def test_binary_eval_accumulate(T, gww, B):
    """Two calls against torch on the CPU: scores within 1 ulp of fp32 of torch.sigmoid, the confusion matrix exact (every
    logit is either exactly 0.0 -- probability 0.5, class 0 -- or decisive beyond that ulp), the loss within 1e-6."""
    from gw_whisper_amd import roc
    rng = np.random.default_rng(B)
    special = np.asarray([0.0, 40.0, -40.0, 80.0, -80.0, -0.0, 1e-3, -1e-3], np.float32)
    state = roc.BinaryEvalState(2 * B, "cuda")
    zs, ys, losses = [], [], []
    for call in range(2):
        z = (rng.standard_normal(B) * 4.0).astype(np.float32)
        z[np.abs(z) < 1e-3] = 1.0
        k = min(B, len(special))
        z[:k] = np.roll(special, call)[:k]
        y = (rng.random(B) < 0.5).astype(np.float32)
        state.add(T.from_numpy(z).cuda().view(-1, 1), T.from_numpy(y).cuda().view(-1, 1), T.from_numpy(y * 9).cuda())
        zs.append(z)
        ys.append(y)
        losses.append(T.nn.BCEWithLogitsLoss()(T.from_numpy(z), T.from_numpy(y)).item())
    res = state.read()
    z, y = np.concatenate(zs), np.concatenate(ys)
    ref = T.sigmoid(T.from_numpy(z)).numpy()
    ulp = np.spacing(ref)
    d = np.abs(res["scores"].astype(np.float64) - ref.astype(np.float64))
    print(f"B={B}: max |score - torch.sigmoid| = {(d / ulp).max()} ulp")
    assert (d <= ulp).all()
    assert (res["scores"][z == 0] == 0.5).all()
    assert ((np.abs(ref.astype(np.float64) - 0.5) > ulp) | (z == 0)).all()
    pred = T.sigmoid(T.from_numpy(z)).round().numpy()
    cm = np.zeros((2, 2), np.int64)
    np.add.at(cm, ((y > 0.5).astype(int), pred.astype(int)), 1)
    assert np.array_equal(res["confusion"], cm) and (pred[z == 0] == 0).all()
    assert res["batches"] == 2 and abs(res["loss"] - np.mean(losses)) <= 1e-6 * abs(np.mean(losses))
    assert np.array_equal(res["labels"], y) and np.array_equal(res["snr"], y * 9)
    with pytest.raises(gww.GwwError, match="exceed"):
        state.add(T.zeros(1, device="cuda"), T.zeros(1, device="cuda"))


def test_run_evaluation_end_to_end(T, gww, tmp_path):
    """run_evaluation.py on the adapter and head a two-step run_train.py --synthetic run saved: the three artefacts, the
    saved band reproduced bit for bit from the saved predictions, the saved AUC against roc_auc_score."""
    from sklearn.metrics import roc_auc_score
    from gw_whisper_amd import roc
    out = str(tmp_path)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "harness", "run_train.py"), "--synthetic", "96", "--encoder", "tiny",
                        "--batch-size", "48", "--num-epochs", "1", "--models-path", out + "/m", "--log-dir", out + "/l"],
                       capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([sys.executable, os.path.join(ROOT, "harness", "run_evaluation.py"), "--synthetic", "96", "--model_type", "2D",
                        "--num_bootstrap", "20", "--encoder", "tiny", "--bootstrap_seed", "11", "--out_dir", out + "/e",
                        "--lora_weights_path", out + "/m/lora_weights_8_32", "--dense_layers_path", out + "/m/dense_layers_8_32.pth"],
                       capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout + r.stderr
    z = np.load(out + "/e/ROC_curve_SNR_0_2D.npz")
    assert sorted(z.files) == sorted(["fpr", "tpr", "auc", "grid", "mean_tpr", "std_tpr", "all_labels", "all_raw_preds", "all_snr"])
    assert z["all_raw_preds"].shape == (96,) and z["all_labels"].sum() == 48 and z["mean_tpr"].shape == (500,)
    assert ((z["all_snr"] > 0) == (z["all_labels"] > 0)).all()
    report = open(out + "/e/report_0.txt").read()
    assert "injection" in report and "noise" in report and "macro F1" in report
    rec = [json.loads(l) for l in open(out + "/e/eval_log.jsonl")][-1]
    assert np.isfinite(rec["loss"]) and 0.0 <= rec["f1"] <= 1.0 and rec["n_valid"] == 20
    again = roc.RocEvaluator(num_bootstrap=20, seed=11)(z["all_raw_preds"], z["all_labels"])
    assert np.array_equal(again["mean_tpr"], z["mean_tpr"]) and np.array_equal(again["std_tpr"], z["std_tpr"])
    assert np.array_equal(again["fpr"], z["fpr"]) and np.array_equal(again["tpr"], z["tpr"])
    assert rec["auc"] == float(z["auc"]) == again["auc"]
    assert abs(float(z["auc"]) - roc_auc_score(z["all_labels"], z["all_raw_preds"])) <= 1e-12
