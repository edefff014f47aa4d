"""The efficiency study's test stage on the device (gw_whisper_amd/trigger_stats.py, csrc/trigger_stats.hip) against the
outputs of the reference's own functions (tests/golden/efficiency_test.npz): every array bit for bit, ``sens-dist`` to
2^-50 (tests/trigger_stats_helpers.py: DIST_REL).  Beyond the fixture the device is held to the numpy restatement, which
tests/test_trigger_stats_host.py holds to the same fixture.  ``score_windows`` and the two harness programs are plumbing
over kernels tested elsewhere: they are checked for identity, without a tolerance."""

import os
import sys

import numpy as np
import pytest

from . import trigger_stats_helpers as th

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "harness"))

GRID = [(ci, thr) for ci in range(th.n_cases()) for thr in th.THRESHOLDS]


@pytest.fixture(scope="module")
def T():
    import torch
    assert torch.cuda.is_available()
    return torch


@pytest.fixture(scope="module")
def gold(golden):
    return golden("efficiency_test.npz")


def _evaluate(T, c, thr, dtype=None, **kw):
    from gw_whisper_amd import trigger_stats as ts
    series = T.from_numpy(np.asarray(c["series"])).cuda()
    if dtype is not None:
        series = series.to(dtype)
    return ts.evaluate(series, c["delta_t"], c["epoch"], c["inj"], c["dist"], thr, th.CLUSTER_TOL, th.EVENT_TOL, **kw)


def _flat(res):
    out = {"trig_times": res["triggers"][0], "trig_values": res["triggers"][1], "ev_times": res["events"][0],
           "ev_values": res["events"][1]}
    out.update(res["statistics"])
    return out


@pytest.fixture(scope="module")
def device_results(T, gww):
    """``evaluate`` of every fixture case, computed once and shared."""
    from gw_whisper_amd import trigger_stats as ts
    out = {}
    for ci, thr in GRID:
        try:
            out[(ci, thr)] = _flat(_evaluate(T, th.case(ci), thr))
        except ts.NoTruePositive as e:
            out[(ci, thr)] = e
    return out


# ---- the fixture --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ci,thr", GRID)
def test_device_equals_the_reference(device_results, gold, ci, thr):
    got = device_results[(ci, thr)]
    if int(gold[th.key(ci, thr, "refused")]):
        assert isinstance(got, Exception) and "no true positive" in str(got)
        for k, (a, b) in (("triggers", ("trig_times", "trig_values")), ("events", ("ev_times", "ev_values"))):
            assert np.array_equal(got.partial[k][0], gold[th.key(ci, thr, a)])
            assert np.array_equal(got.partial[k][1], gold[th.key(ci, thr, b)])
        return
    assert not isinstance(got, Exception), got
    th.compare(got, {k: gold[th.key(ci, thr, k)] for k in th.ARRAYS}, f"device, case {ci} at {thr}")


def test_identical_calls_give_identical_bits(T, device_results):
    for ci, thr in ((3, 0.1), (4, 0.5)):
        again = _flat(_evaluate(T, th.case(ci), thr))
        for k in th.ARRAYS:
            assert np.array_equal(again[k].view(np.int64), device_results[(ci, thr)][k].view(np.int64)), k


def test_stages_entered_on_their_own(T, device_results):
    """``triggers``, ``events`` and ``statistics`` from numpy (what --load-triggers / --load-events read) and from device
    tensors equal the chained ``evaluate``."""
    from gw_whisper_amd import trigger_stats as ts
    for ci, thr in ((2, 0.1), (3, 0.1), (th.HAND, 0.1)):
        c, whole = th.case(ci), device_results[(ci, thr)]
        tt, tv = ts.triggers(T.from_numpy(c["series"]).cuda(), c["delta_t"], c["epoch"], thr)
        assert np.array_equal(tt, whole["trig_times"]) and np.array_equal(tv, whole["trig_values"])
        et, ev = ts.events(tt, tv, th.CLUSTER_TOL)
        assert np.array_equal(et, whole["ev_times"]) and np.array_equal(ev, whole["ev_values"])
        et2, ev2 = ts.events(T.from_numpy(tt).cuda(), T.from_numpy(tv).cuda(), th.CLUSTER_TOL)
        assert np.array_equal(et2, et) and np.array_equal(ev2, ev)
        duration = len(c["series"]) * c["delta_t"]
        for a, b in ((et, ev), (T.from_numpy(et).cuda(), T.from_numpy(ev).cuda())):
            st = ts.statistics(a, b, c["inj"], c["dist"], duration, th.EVENT_TOL)
            for k in ts.STAT_KEYS:
                assert np.array_equal(st[k], whole[k], equal_nan=True), k


# ---- beyond the fixture: the device against the restatement -----------------------------------------------------------------
def _against_restatement(T, c, thr, side, **kw):
    got = _flat(_evaluate(T, c, thr, **kw))
    th.compare(got, th.restate(c, thr), side)
    return got


def test_one_run_all_above_threshold(T, gww):
    """Every sample a trigger, one cluster over five workgroups of the event kernels; the maximum twice, first in the
    second workgroup: the carry must keep the first."""
    c = th.make_case(4500, 3, 0, 4201, 0.75)
    c["series"] = np.round(0.2 + 0.5 * np.random.default_rng(4202).random(4500), 2)
    c["series"][[1500, 3900]] = 0.95
    c["inj"] = np.array([0.75 + 150.0, 10.0, 400.0])
    got = _against_restatement(T, c, 0.1, "one run")
    assert len(got["trig_times"]) == 4500 and len(got["ev_times"]) == 1 and got["ev_times"][0] == 1500 * 0.1 + 0.75
    assert len(got["ranking"]) == 0                      # the one event is a true positive: no false positive, no step


def test_no_trigger_and_no_false_positive(T, gww):
    from gw_whisper_amd import trigger_stats as ts
    c = th.make_case(300, 4, 0, 4203, 0.75)
    tt, tv = ts.triggers(T.from_numpy(c["series"]).cuda(), c["delta_t"], c["epoch"], 2.0)
    assert tt.shape == tv.shape == (0,) and tt.dtype == np.float64
    with pytest.raises(ts.NoTruePositive) as e:
        _evaluate(T, c, 2.0)
    assert all(len(a) == 0 for k in ("triggers", "events") for a in e.value.partial[k])
    with pytest.raises(th.NoTruePositive):
        th.restate(c, 2.0)
    # true positives only: samples above the threshold next to injections, nothing else
    c["series"] = np.zeros(300)
    at = np.array([20, 90, 160, 230])
    c["series"][at] = (0.6, 0.7, 0.6, 0.9)
    c["inj"] = at * c["delta_t"] + c["epoch"] + 0.05
    got = _against_restatement(T, c, 0.1, "no false positive")
    assert len(got["ev_times"]) == 4 and all(got[k].shape == (0,) and got[k].dtype == np.float64 for k in ts.STAT_KEYS)


def test_one_injection_fp32_series_and_capacity(T, gww):
    from gw_whisper_amd import trigger_stats as ts
    c = th.make_case(4097, 1, 0, 4204, 0.75)
    _against_restatement(T, c, 0.1, "one injection")
    # an fp32 series is widened exactly: the same as the restatement of the widened values; 0.1f > 0.1 is a trigger
    c32 = dict(th.make_case(5000, 20, 0, 4205, 0.75))
    c32["series"] = c32["series"].astype(np.float32)
    assert np.any(c32["series"] == np.float32(0.1))
    got = _against_restatement(T, c32, 0.1, "fp32 series", dtype=None)
    assert got["trig_values"].dtype == np.float64 and np.any(got["trig_values"] == float(np.float32(0.1)))
    # a capacity that holds the triggers changes nothing; one that does not is refused
    n_trig = len(got["trig_times"])
    again = _flat(_evaluate(T, c32, 0.1, capacity=n_trig))
    assert all(np.array_equal(again[k], got[k], equal_nan=True) for k in th.ARRAYS)
    with pytest.raises(gww.GwwError, match="capacity"):
        _evaluate(T, c32, 0.1, capacity=n_trig - 1)


@pytest.mark.parametrize("n", [4095, 4096, 1023, 1024, 1025])
def test_tile_boundaries(T, gww, n):
    """One below, at and above the 4096-sample tile of the trigger kernels; and exactly 1023, 1024 and 1025 triggers, around
    the 1024-trigger workgroup of the event kernels, with a cluster across the boundary."""
    if n >= 4095:
        _against_restatement(T, th.make_case(n, 30, 0, 4300 + n, 0.75), 0.1, f"n = {n}")
        return
    c = th.make_case(3000, 10, 0, 4300 + n, 0.75)
    c["series"] = np.zeros(3000)
    c["series"][:n + 6] = np.round(0.2 + 0.7 * np.random.default_rng(n).random(n + 6), 2)
    c["series"][1000:1021:4] = 0.0                       # six lone samples out: cluster boundaries in front of trigger 1024
    c["series"][5] = 0.99                                # the first cluster's event, with an injection on it
    c["inj"] = np.r_[5 * c["delta_t"] + c["epoch"], 400.0 + np.arange(9)]
    got = _against_restatement(T, c, 0.1, f"{n} triggers")
    assert len(got["trig_times"]) == n


def test_refusals_on_the_device(T, gww):
    from gw_whisper_amd import trigger_stats as ts
    c = th.make_case(300, 4, 0, 4206, 0.75)
    bad = c["series"].copy()
    bad[17] = np.nan
    with pytest.raises(gww.GwwError, match="NaN"):
        ts.triggers(T.from_numpy(bad).cuda(), 0.1, 0.0, 0.1)
    with pytest.raises(gww.GwwError, match="NaN"):
        ts.evaluate(T.from_numpy(bad).cuda(), 0.1, 0.75, c["inj"], c["dist"])
    with pytest.raises(gww.GwwError, match="NaN"):
        ts.events(np.array([1.0, 2.0]), np.array([0.5, np.nan]), 0.2)
    with pytest.raises(gww.GwwError, match="NaN"):
        ts.statistics(np.array([1.0, 2.0]), np.array([0.5, np.nan]), c["inj"], c["dist"], 30.0, 0.3)
    with pytest.raises(ts.NoTruePositive):
        ts.statistics(np.array([1.0e6]), np.array([0.5]), c["inj"], c["dist"], 30.0, 0.3)
    with pytest.raises(gww.GwwError, match="duration"):
        ts.evaluate(T.from_numpy(c["series"]).cuda(), 0.1, 0.75, c["inj"], c["dist"], duration=0.0)


# ---- the network over windows ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def reduced_model(T, gww):
    """The reduced encoder (d = 128, 2 layers, fp32) under the study's head, seeded."""
    from gw_whisper_amd import synth
    from gw_whisper_amd.encoder import WhisperConfig, WhisperEncoder
    from gw_whisper_amd.models import efficiency_classifier
    sd = synth.encoder_state_dict(128, 2, 2, 512, seed=11)
    enc = WhisperEncoder.from_numpy_state_dict(sd, WhisperConfig(128, 2, 2, 512), precision="fp32")
    T.manual_seed(12)
    return efficiency_classifier(enc, num_classes=2).cuda().eval()


def _windows(n, seed):
    return (np.random.default_rng(seed).normal(size=(n, 2048)) * 3.0).astype(np.float32)


def test_score_windows_is_the_separate_calls(T, gww, reduced_model):
    from gw_whisper_amd import efficiency, inference, ops
    from gw_whisper_amd import trigger_stats as ts
    from gw_whisper_amd.models import _pooled
    model = reduced_model
    w = T.from_numpy(_windows(5, 21)).cuda()
    params = [p.detach() for p in efficiency._det_parameters(model.classifier)]
    with T.no_grad():
        pooled = T.cat([_pooled(model.encoder, ops.logmel(inference.resample(w[i:i + 2], 16000))).to(T.float32)
                        for i in range(0, 5, 2)])
        col0 = ops.det_head_scores(pooled, params, T.empty(5, device="cuda"), ops.SCORE_PROB0)
        _, _, probs, _, _ = ops.det_head_forward(pooled, params, T.zeros(5, 2, device="cuda"))
        diff0 = ops.det_head_scores(pooled, params, T.empty(5, device="cuda"), ops.SCORE_LOGIT_DIFF)
    soft = ts.score_windows(model, w, 0)
    assert soft.shape == (5, 2) and soft.dtype == T.float32 and soft.is_cuda
    assert T.equal(soft, ts.score_windows(model, w, 3)) and T.equal(soft, ts.score_windows(model, w, 1))
    assert T.equal(soft[:, 0], col0) and T.equal(soft, probs)
    assert T.equal(soft, ops.det_head_scores2(pooled, params))
    from gw_whisper_amd.models import efficiency_classifier
    bare = efficiency_classifier(model.encoder, num_classes=2).cuda().eval()
    bare.classifier.load_state_dict(model.classifier.state_dict())
    lin = ts.score_windows(efficiency.remove_softmax(bare), w, 2)
    assert T.equal(lin[:, 0], diff0) and T.equal(lin[:, 1], -lin[:, 0])
    assert T.equal(lin, ops.det_head_scores2(pooled, params, remove_softmax=True))
    assert isinstance(list(model.classifier.children())[-1], T.nn.Softmax)        # the fixture's model kept its softmax


def test_programs_end_to_end(T, gww, reduced_model, tmp_path):
    """run_efficiency_test over two small files, again (both skipped), then run_efficiency_evaluate: its statistics file
    holds what ``evaluate`` gives on the same outputs."""
    import run_efficiency_evaluate as ev
    import run_efficiency_test as rt
    from gw_whisper_amd import trigger_stats as ts
    din, dout, log = tmp_path / "in", tmp_path / "out", tmp_path / "log.txt"
    din.mkdir()
    h5 = ev.output_path("x.hdf") == "x.hdf"
    for k, (name, n) in enumerate((("H1-0-2.hdf", 24), ("H1-2-2.hdf", 20))):
        if h5:
            import h5py
            with h5py.File(din / name, "w") as fp:
                fp.create_dataset("H1/data", data=_windows(n, 30 + k))
        else:
            np.savez(din / (name + ".npz"), **{"H1/data": _windows(n, 30 + k)})
    args = rt.build_parser().parse_args(["--input-dir", str(din), "--output-dir", str(dout), "--log-file", str(log),
                                         "--batch-size", "16"])
    written = rt.run(reduced_model, args, T.device("cuda"))
    assert len(written) == 2 and all(os.path.isfile(p) for p in written)
    lines = log.read_text().splitlines()
    assert lines == [f"Successfully saved output to {dout / 'H1-0-2.hdf'}", f"Successfully saved output to {dout / 'H1-2-2.hdf'}"]
    outs = [ev.read_arrays(str(dout / n))["data"] for n in ("H1-0-2.hdf", "H1-2-2.hdf")]
    assert outs[0].shape == (24, 2) and outs[0].dtype == np.float32
    assert np.array_equal(outs[1], ts.score_windows(reduced_model, T.from_numpy(_windows(20, 31)).cuda(), 7).cpu().numpy())
    stamp = [os.path.getmtime(p) for p in written]
    assert rt.run(reduced_model, args, T.device("cuda")) == [] and log.read_text().splitlines() == lines
    assert [os.path.getmtime(p) for p in written] == stamp
    # the evaluation: injections where the network's statistic is largest in each file, so there is a true positive
    series = ts.assemble_time_series_host(ev.load_data(str(dout), 0.75, 0.1, "softmax", "softmax"))
    thr = float(np.median(series.data[series.data > 0]))
    peak = series.sample_times[np.argmax(series.data)]
    inj = tmp_path / "inj.npz"
    np.savez(inj, tc=np.array([peak + 0.02, 1.0e4]), distance=np.array([100.0, 250.0]), mass1=np.ones(2), mass2=np.ones(2))
    flags = ["--injection-file", str(inj), "--data-dir", str(dout), "--test-data-activation", "softmax",
             "--trigger-threshold", repr(thr)]
    assert ev.main(flags) == 0
    want = ts.evaluate(T.from_numpy(series.data).cuda(), 0.1, float(series.start_time), np.array([peak + 0.02, 1.0e4]),
                       np.array([100.0, 250.0]), thr, 0.2, 0.3)
    trig, evs, st = (ev.read_arrays(str(dout / n)) for n in ("triggers.hdf", "events.hdf", "statistics.hdf"))
    assert np.array_equal(trig["data"], want["triggers"][0]) and np.array_equal(trig["trigger_values"], want["triggers"][1])
    assert np.array_equal(evs["times"], want["events"][0]) and np.array_equal(evs["values"], want["events"][1])
    assert sorted(st) == sorted(ts.STAT_KEYS) and len(want["triggers"][0]) > 0
    assert all(np.array_equal(st[k], want["statistics"][k], equal_nan=True) for k in ts.STAT_KEYS)
    th.compare({**{"trig_times": trig["data"], "trig_values": trig["trigger_values"], "ev_times": evs["times"],
                   "ev_values": evs["values"]}, **st},
               th.restate({"series": series.data, "delta_t": 0.1, "epoch": float(series.start_time),
                           "inj": np.array([peak + 0.02, 1.0e4]), "dist": np.array([100.0, 250.0])}, thr), "programs")
    with pytest.raises(IOError, match="Cannot overwrite"):
        ev.main(flags)
    # from the event file on: the same statistics
    assert ev.main(flags[:4] + ["--load-events", str(dout / "events.hdf"), "--duration", repr(len(series) * 0.1),
                                "--stats-file-name", "again.hdf"]) == 0
    again = ev.read_arrays(str(dout / "again.hdf"))
    assert all(np.array_equal(again[k], st[k], equal_nan=True) for k in ts.STAT_KEYS)
