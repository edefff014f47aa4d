"""CPU-side checks of the efficiency study (gw_whisper_amd/efficiency.py) against tests/golden/efficiency.npz,
efficiency_traces.json and efficiency_format.txt, which tools/make_golden_efficiency.py wrote by running the reference's own
classes: the fp64 rebuild of the head step the GPU tests measure against, the dataset's index plans, the three curriculum
schedulers, the false-alarm rank expression and the numpy statistics, the efficiency file format, the head's ``.pth`` key
layout, the ``.npz`` dataset reader, and the refusal of CPU tensors."""
import json
import os

import numpy as np
import pytest
import torch

from gw_whisper_amd import GwwError, efficiency as eff, models, ops

from . import efficiency_helpers as eh

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLD, "efficiency.npz"))


@pytest.mark.parametrize("ci", range(len(eh.CASES)))
def test_fp64_rebuild_reproduces_the_reference_head(gold, ci):
    """efficiency_helpers.head64 == the reference's head class + reg_BCELoss in fp64, to 1e-11: logits, probs, loss and
    every gradient digest; the stored cases keep their ReLU margin."""
    d_in, C, B = eh.CASES[ci]
    assert gold["head_cases"][ci].tolist() == [d_in, C, B]
    x, t = eh.case_inputs(d_in, C, B, int(gold["head_seeds"][ci]))
    params = [torch.from_numpy(p) for p in eh.case_params(ci, d_in, C)]
    loss, z, p, dx, grads, margin = eh.head64(torch.from_numpy(x), params, torch.from_numpy(t))
    assert margin >= 2e-6 and abs(margin - float(gold[f"head{ci}_margin"])) <= 1e-11
    assert np.abs(z.numpy() - gold[f"head{ci}_logits"]).max() <= 1e-11
    assert np.abs(p.numpy() - gold[f"head{ci}_probs"]).max() <= 1e-11
    assert abs(float(loss) - float(gold[f"head{ci}_loss"])) <= 1e-11
    for key, g, name in [(0, dx, "dx")] + [(1 + k, g, f"grad{k}") for k, g in enumerate(grads)]:
        ref = gold[f"head{ci}_{name}"]
        assert np.abs(eh.digest(g.numpy(), key) - ref).max() <= 1e-11 * max(1.0, np.abs(ref).max()), name


def _dataset(n_wave, n_noise, ia, snr_range=(1.0, 1.0), seed=0):
    # plan() needs only the tensors' lengths: host tensors do
    return eff.ResampledDataset(torch.zeros(n_wave, 4), torch.zeros(n_noise, 4), snr_range, ia[1], ia[2], ia[3],
                                noises_per_signal=ia[0], seed=seed)


def test_dataset_plans_equal_the_reference(gold):
    cases = json.loads(str(gold["plan_cases"]))
    assert len(cases) == 5
    for pi, (n_wave, n_noise, ia) in enumerate(cases):
        ds = _dataset(n_wave, n_noise, ia)
        ref = gold[f"plan{pi}"]
        assert len(ds) == int(gold[f"plan{pi}_len"]) == len(ref)
        noise_i, wave_i, snr, is_wave = ds.plan(np.arange(len(ds)))
        assert wave_i.tolist() == ref[:, 0].tolist() and noise_i.tolist() == ref[:, 1].tolist(), pi
        assert is_wave.astype(int).tolist() == ref[:, 2].tolist()
        assert (snr[is_wave] == 1.0).all() and (snr[~is_wave] == 0.0).all() and (wave_i[~is_wave] == -1).all()
        # any order, one at a time
        order = np.random.default_rng(pi).permutation(len(ds))
        got = np.asarray([[ds.plan([i])[1][0], ds.plan([i])[0][0]] for i in order])
        assert np.array_equal(got, ref[order][:, :2])


def test_dataset_snr_draws_and_snrs_accessor():
    ia = [2, [0, 4], [0, 8], [8, 12]]
    a, b = _dataset(4, 12, ia, (5.0, 15.0), seed=3), _dataset(4, 12, ia, (5.0, 15.0), seed=3)
    idx = [9, 0, 3, 11, 7]
    sa = a.plan(idx)[2]
    draws = np.random.default_rng(3).uniform(5.0, 15.0, 3).astype(np.float32)       # one draw per injected item, in order
    assert sa.tolist() == [0.0, draws[0], draws[1], 0.0, draws[2]] and np.array_equal(sa, b.plan(idx)[2])
    assert a.snrs() == (5.0, 15.0)
    a.snrs((7.0, 7.0))
    assert a.snrs() == (7.0, 7.0) and (a.plan([0, 1])[2] == 7.0).all()
    a.snrs(1.0, 2.0)
    assert a.snrs() == (1.0, 2.0)
    with pytest.raises(ValueError):
        a.snrs(1, 2, 3)
    with pytest.raises(AssertionError):
        _dataset(4, 12, [2, [0, 4], [0, 7], [8, 12]])


def test_scheduler_traces_equal_the_reference():
    traces = json.load(open(os.path.join(GOLD, "efficiency_traces.json")))
    assert sorted({t["class"] for t in traces}) == ["EpochCLScheduler", "PlateauCLScheduler", "ThresholdCLScheduler"]

    class DS:
        def __init__(self):
            self.r = (100.0, 200.0)

        def snrs(self, *a):
            if not a:
                return self.r
            self.r = a[0]
    for t in traces:
        dss = (DS(), DS())
        lin = torch.nn.Linear(2, 2)
        opt = torch.optim.Adam(lin.parameters(), lr=1e-3)
        # give the optimizer a state: every range change must put the initial (empty) one back
        lin(torch.ones(1, 2)).sum().backward()
        sched = getattr(eff, t["class"])([tuple(r) for r in t["ranges"]], dss, verbose=False, optim=opt, **t["kwargs"])
        opt.step()
        assert len(opt.state_dict()["state"]) == 2
        states = [[list(dss[0].snrs()), list(dss[1].snrs()), sched.done, sched.interrupt]]
        for m in t["metrics"]:
            before = dss[0].snrs()
            sched.step(*m)
            if dss[0].snrs() != before:
                assert opt.state_dict()["state"] == {}, "the optimizer state was not reloaded on a range change"
                opt.step()
            states.append([list(dss[0].snrs()), list(dss[1].snrs()), sched.done, sched.interrupt])
        assert states == t["states"], (t["class"], t["kwargs"])


def test_snr_ranges_of_the_scheduler_parameters():
    assert eff.snr_ranges((5., 15.), (5., 15.), 0) == [(5., 15.)]
    r = eff.snr_ranges((20., 30.), (5., 15.), 3)
    assert [tuple(map(float, x)) for x in r] == [(20., 30.), (15., 25.), (10., 20.), (5., 15.)]


def test_rank_expression_and_numpy_statistics_equal_the_reference_estimator(gold):
    """The reference's estimator ran on these scores: the rank expression (with its truncation to 0) and the numpy
    statistics the GPU tests hold the device kernels to reproduce its table exactly."""
    faps = gold["est_faps"].tolist()
    ranks = eff.false_alarm_ranks(faps, 57)
    assert ranks.tolist() == [28, 5, 2, 0] and ranks.dtype.kind == "i"
    assert eff.false_alarm_ranks([0.1, 0.01, 0.001, 0.0001, 0.00001], 400000).tolist() == [40000, 4000, 400, 40, 4]
    assert eff.false_alarm_ranks([0.29], 100).tolist() == [int(0.29 * 100)] == [28]      # the truncation is part of the result
    thr, table = eh.numpy_statistics(gold["est_noise_scores"], gold["est_wave_scores"], faps)
    assert thr[3] == gold["est_noise_scores"].min()
    assert np.array_equal(table, gold["est_table"])
    # and the scores themselves are noise + snr * wave through the stand-in network
    for s, snr in enumerate(gold["est_snrs"]):
        x = gold["est_noise"][57:] + np.float32(snr) * gold["est_wave"]
        assert np.allclose(x @ gold["est_proj"], gold["est_wave_scores"][s], rtol=0, atol=1e-4)


def test_efficiency_text_reproduces_the_shipped_file():
    text = open(os.path.join(GOLD, "efficiency_format.txt")).read()
    faps, snrs, table = eff.parse_efficiency_text(text)
    assert faps == [0.1, 0.01, 0.001, 0.0001, 0.00001] and snrs == [float(s) for s in np.arange(5, 25, 2)]
    assert table.shape == (10, 5)
    assert eff.efficiency_text(faps, snrs, table) == text
    assert eff.efficiency_text(faps, list(np.arange(5, 25, 2)), table) == text      # the program's numpy SNRs
    with pytest.raises(ValueError):
        eff.parse_efficiency_text("5.0 1.0\n")


def _enc(d):
    return type("Enc", (), {"config": type("Cfg", (), {"d_model": d})()})()


def test_head_key_layout_and_remove_softmax():
    m = models.efficiency_classifier(_enc(384))
    assert list(m.classifier.state_dict()) == list(eh.PARAM_KEYS)
    assert [type(l).__name__ for l in m.classifier] == ["Linear", "ReLU"] * 4 + ["Linear", "Softmax"]
    assert m.classifier[8].out_features == 2 and m.classifier[9].dim == 1
    sd = {k: torch.from_numpy(v) for k, v in zip(eh.PARAM_KEYS, eh.case_params(0, 384, 2))}
    m.classifier.load_state_dict(sd)                      # a dense_layers_*.pth of the reference has exactly these keys
    x = torch.randn(3, 384)
    z = torch.nn.Sequential(*list(m.classifier.children())[:-1])(x)
    eff.remove_softmax(m)
    assert isinstance(m.classifier[-1], eff.LogitDifference) and not m.classifier[-1].weight.requires_grad
    out = m.classifier(x)
    assert torch.equal(out[:, 0], z[:, 0] - z[:, 1]) and torch.equal(out[:, 1], -out[:, 0])
    with pytest.raises(ValueError, match="Softmax"):
        eff.remove_softmax(m)
    assert models.efficiency_classifier(_enc(128), num_classes=5).classifier[8].out_features == 5


def test_npz_reader(tmp_path):
    rng = np.random.default_rng(0)
    w = rng.standard_normal((5, 2048, 1)).astype(np.float32)       # the reference's waveform files: a trailing channel axis
    n = rng.standard_normal((9, 2048)).astype(np.float32)
    np.savez(tmp_path / "t_signals.hdf.npz", **{"data/0": w})
    np.savez(tmp_path / "t_noise.npz", **{"data/0": n})
    assert np.array_equal(eff._read_rows(str(tmp_path), "t_signals.hdf", 3), w[:3, :, 0])
    assert np.array_equal(eff._read_rows(str(tmp_path), "t_noise.npz", 100), n)
    with pytest.raises(FileNotFoundError):
        eff._read_rows(str(tmp_path), "absent.hdf", 3)
    np.savez(tmp_path / "bad.npz", **{"data/0": n[0]})
    with pytest.raises(ValueError, match="shape"):
        eff._read_rows(str(tmp_path), "bad.npz", 3)
    with pytest.raises(GwwError, match="GPU"):
        eff.load_resampled_dataset(str(tmp_path), "t_signals.hdf", "t_noise.npz", (5, 15), [1, [0, 5], [0, 5], [5, 9]],
                                   device="cpu")


def test_cpu_tensors_are_refused():
    d_in, C, B = 128, 2, 4
    params = [torch.from_numpy(p) for p in eh.case_params(3, d_in, C)]
    x, t = torch.zeros(B, d_in), torch.zeros(B, C)
    with pytest.raises(GwwError, match="GPU"):
        ops.det_head_forward(x, params, t)
    with pytest.raises(GwwError, match="GPU"):
        ops.det_head_scores(x, params, torch.zeros(B))
    with pytest.raises(GwwError, match="GPU"):
        ops.score_thresholds(torch.zeros(8), torch.ones(1, dtype=torch.int64))
    with pytest.raises(GwwError, match="GPU"):
        ops.detection_counts(torch.zeros(8), torch.zeros(2), torch.zeros(2, dtype=torch.int64))
    with pytest.raises(GwwError, match="GPU"):
        ops.det_eval_accumulate(torch.zeros(B, C), t, torch.zeros(B), *[torch.zeros(1, dtype=torch.int64)] * 4)
    m = models.efficiency_classifier(_enc(d_in))
    with pytest.raises(GwwError, match="GPU"):
        eff.reg_bce_head(m.classifier, x, t)
    with pytest.raises(GwwError, match="Sequential"):
        eff._det_parameters(torch.nn.Sequential(torch.nn.Linear(4, 2)))


def test_argument_errors_without_gpu():
    """Shape, mode and workspace checks come before any HIP call."""
    from gw_whisper_amd import lib
    L = lib()
    from gw_whisper_amd import _lib
    p = [1 << 12] * 12          # non-NULL, 16-byte aligned stand-ins: nothing is dereferenced before the checks
    five = (_lib.C.c_void_p * 5)(*p[:5])
    P, A, G = (_lib.C.byref(b) for b in (_lib.MlpParams(5, five, five), _lib.MlpActs((_lib.C.c_void_p * 4)(*p[:4]), p[0]),
                                         _lib.MlpGrads(five, five)))
    assert L.gww_det_head_forward_f32(p[0], P, p[0], 4, 100, 2, 1e-6, A, *p[:4], None) == -1 and b"d_in" in L.gww_last_error()
    assert L.gww_det_head_forward_f32(p[0], P, p[0], 4, 128, 1, 1e-6, A, *p[:4], None) == -1 and b"C=" in L.gww_last_error()
    assert L.gww_det_head_forward_f32(p[0], P, p[0], 4, 128, 2, 0.5, A, *p[:4], None) == -1 and b"epsilon" in L.gww_last_error()
    assert L.gww_det_head_forward_f32(p[0], P, p[0], 0, 128, 2, 1e-6, A, *p[:4], None) == -1 and b"B=" in L.gww_last_error()
    need = L.gww_det_head_workspace_bytes(4, 2)
    assert need == 4 * (512 + 256 + 128 + 64 + 2) * 4
    assert (L.gww_det_head_backward_f32(p[0], P, A, p[0], p[0], 4, 128, 2, p[0], need - 1, p[0], G, None) == -1
            and b"workspace" in L.gww_last_error())
    assert L.gww_det_head_scores_f32(p[0], P, 4, 128, 3, 1, p[0], 1, None) == -1 and b"C = 2" in L.gww_last_error()
    assert L.gww_det_head_scores_f32(p[0], P, 4, 128, 2, 2, p[0], 1, None) == -1 and b"mode" in L.gww_last_error()
    assert L.gww_det_head_scores_f32(p[0], P, 4, 128, 2, 0, p[0], 0, None) == -1 and b"stride" in L.gww_last_error()
    ws = L.gww_score_thresholds_workspace_bytes()
    assert L.gww_score_thresholds_f32(p[0], 10, p[0], 9, p[0], p[0], ws, None) == -1 and b"F=" in L.gww_last_error()
    assert L.gww_score_thresholds_f32(p[0], 10, p[0], 2, p[0], p[0], ws - 1, None) == -1 and b"workspace" in L.gww_last_error()
    assert L.gww_score_thresholds_f32(p[0], 0, p[0], 2, p[0], p[0], ws, None) == -1 and b"N=" in L.gww_last_error()
    assert L.gww_detection_counts_f32(p[0], 10, p[0], 0, p[0], None) == -1
    assert L.gww_det_eval_accumulate(p[0], p[0], p[0], 4, 1, p[0], p[0], p[0], p[0], None) == -1


def test_estimator_refuses_a_classifier_without_a_score_layer():
    class Net:
        classifier = torch.nn.Sequential(torch.nn.Linear(2, 2))
    with pytest.raises(GwwError, match="Softmax"):
        eff.EfficiencyEstimator(None, None, [5.0], faps=(0.1,))(Net())
