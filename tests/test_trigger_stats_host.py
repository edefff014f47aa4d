"""The efficiency study's test-stage evaluation without a GPU: the vectorised numpy restatement of the device algorithm
(tests/trigger_stats_helpers.py) against the outputs of the reference's own functions (tests/golden/efficiency_test.npz,
written by tools/make_golden_efficiency_test.py), bit for bit; the file bookkeeping and the flag errors of
harness/run_efficiency_evaluate.py; and every refusal that happens before a launch."""

import ctypes as C
import os
import sys

import numpy as np
import pytest

import gw_whisper_amd
from gw_whisper_amd import trigger_stats as ts

from . import trigger_stats_helpers as th

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "harness"))

GRID = [(ci, thr) for ci in range(th.n_cases()) for thr in th.THRESHOLDS]


@pytest.fixture(scope="module")
def gold(golden):
    return golden("efficiency_test.npz")


# ---- the restatement against the reference ---------------------------------------------------------------------------------
@pytest.mark.parametrize("ci,thr", GRID)
def test_restatement_equals_the_reference(gold, ci, thr):
    c = th.case(ci)
    if int(gold[th.key(ci, thr, "refused")]):
        assert (ci, thr) in th.REFUSED
        with pytest.raises(th.NoTruePositive):
            th.restate(c, thr)
        tt, tv = th.triggers(c["series"], c["delta_t"], c["epoch"], thr)
        assert np.array_equal(tt, gold[th.key(ci, thr, "trig_times")]) and np.array_equal(tv, gold[th.key(ci, thr, "trig_values")])
        return
    assert (ci, thr) not in th.REFUSED
    th.compare(th.restate(c, thr), {k: gold[th.key(ci, thr, k)] for k in th.ARRAYS}, f"case {ci} at {thr}")


def test_the_cases_hold_what_they_are_there_for(gold):
    """Both branches of the first-step quirk, a cluster longer than a chunk, both sides of the cluster tolerance at a
    two-sample gap, a distance equal to the event tolerance, a GPS-sized epoch an fp32 time could not hold."""
    first_run = {}
    for ci in (1, 2, th.HAND):
        r = th.restate(th.case(ci), 0.5 if ci < th.HAND else 0.1)
        fp = th.split(r["ev_times"], r["ev_values"], th.case(ci)["inj"], th.EVENT_TOL)[1]
        first_run[ci] = int(np.sum(fp == fp[0]))
    assert first_run[1] == 1 and first_run[2] > 1 and first_run[th.HAND] == 1, first_run
    big = th.restate(th.case(3), 0.1)
    opens = np.r_[True, np.diff(big["trig_times"]) >= th.CLUSTER_TOL]
    assert np.diff(np.r_[np.flatnonzero(opens), len(opens)]).max() >= 5000
    hand = th.restate(th.case(th.HAND), 0.1)
    gaps = np.diff(hand["trig_times"])
    two = gaps[np.round(gaps / th.DELTA_T) == 2]
    assert np.any(two < th.CLUSTER_TOL) and np.any(two >= th.CLUSTER_TOL)
    d = th.nearest(np.sort(th.case(th.HAND)["inj"]), hand["ev_times"])
    assert np.any(d == th.EVENT_TOL) and hand["ev_times"][0] < 0.2 and hand["ev_times"][-1] > 4.0
    gps = th.restate(th.case(th.GPS), 0.1)["trig_times"]
    assert not np.array_equal(gps.astype(np.float32).astype(np.float64), gps) and np.all(np.diff(gps.astype(np.float32)) >= 0)
    assert np.unique(gps.astype(np.float32)).size < gps.size


def test_first_maximum_and_cluster_rule():
    t = np.array([0.0, 0.1, 0.2, 0.5, 0.6, 1.0])
    v = np.array([0.3, 0.7, 0.7, 0.2, 0.2, 0.9])
    et, ev = th.events(t, v, 0.2)
    assert et.tolist() == [0.1, 0.5, 1.0] and ev.tolist() == [0.7, 0.2, 0.9]


def test_ranking_quirk_of_the_first_step():
    inj, dist = np.array([100.0]), np.array([50.0])
    t = np.array([100.0, 1.0, 2.0, 3.0, 4.0])
    one = th.statistics(t, np.array([0.9, 0.2, 0.3, 0.3, 0.5]), inj, dist, 10.0, 0.3)
    assert (one["far"] / th.SEC_PER_MONTH * 10.0).round().tolist() == [4, 1, 0]      # n, not n - 1, for the lone first value
    run = th.statistics(t, np.array([0.9, 0.2, 0.2, 0.3, 0.5]), inj, dist, 10.0, 0.3)
    assert (run["far"] / th.SEC_PER_MONTH * 10.0).round().tolist() == [2, 1, 0]


# ---- the container and the file bookkeeping ------------------------------------------------------------------------------
def test_time_series_stand_in():
    a = ts.TimeSeries(np.arange(5.0), 0.1, epoch=1238166018.75)
    assert a.start_time.ns == 1238166018750000000 and float(a.start_time) == 1238166018.75
    assert float(a.end_time - a.start_time) == 0.5 and a.duration == 0.5
    assert np.array_equal(a.sample_times, np.arange(5) * 0.1 + 1238166018.75)
    assert float(ts.GPSTime(0.3) - ts.GPSTime(0.1)) == 200000000 * 1e-9
    assert np.array_equal(a > 2.0, [False, False, False, True, True])


def test_start_time_and_ranking_statistic():
    import run_efficiency_evaluate as ev
    assert ev.get_start_time("H1-0-100.hdf") == 0 and ev.get_start_time("H1-1200-100.hdf") == 1200 + 0.1
    data = np.random.default_rng(3).normal(size=(7, 2)).astype(np.float32)
    soft = ev.ranking_statistic(data, "linear", "softmax")
    e0, e1 = np.exp(data.T[0]), np.exp(data.T[1])
    assert soft.dtype == np.float32 and np.array_equal(soft, e0 / (e0 + e1))
    assert np.array_equal(ev.ranking_statistic(data, "linear", "linear"), data.T[0] - data.T[1])
    assert np.array_equal(ev.ranking_statistic(data, "softmax", "softmax"), data.T[0])
    with pytest.raises(ValueError, match="softmax activation"):
        ev.ranking_statistic(data, "softmax", "linear")


def test_load_and_assemble(tmp_path):
    """Files in ascending start order, a later file over an earlier one where they overlap, zero fill in the gap, and the
    trigger file of an earlier run skipped."""
    import run_efficiency_evaluate as ev
    rng = np.random.default_rng(5)
    files = {"H1-0-10.hdf.npz": rng.normal(size=(30, 2)), "H1-2-10.hdf.npz": rng.normal(size=(20, 2)),
             "H1-6-10.hdf.npz": rng.normal(size=(10, 2))}
    for fn, d in files.items():
        np.savez(tmp_path / fn, data=d.astype(np.float32))
    np.savez(tmp_path / "triggers.hdf.npz", data=np.zeros(3), trigger_values=np.zeros(3))
    (tmp_path / "notes.txt").write_text("not a data file")
    lst = ev.load_data(str(tmp_path), epoch_offset=0.75, delta_t=0.1, data_activation="linear", target_activation="linear")
    assert [float(t.start_time) for t in lst] == [0.75, 2.1 + 0.75, 6.1 + 0.75]
    start, n, dt, place = ts.assemble_plan(lst)
    assert start == 0.75 and dt == 0.1 and n == int((float(lst[2].end_time) - 0.75) / 0.1) + 1
    whole = ts.assemble_time_series_host(lst)
    want = np.zeros(n)
    for (i, t) in place:
        want[i:i + len(t)] = t.data
    # int(float(start - start0) / dt) truncates as the reference does: 6.1 / 0.1 is 60.99999999999999
    assert [i for i, _ in place] == [0, int(2.1 / 0.1), int(6.1 / 0.1)] == [0, 21, 60]
    assert np.array_equal(whole.data, want) and whole.data.dtype == np.float64
    assert np.array_equal(whole.data[21:30], lst[1].data[:9].astype(np.float64))      # the later file won the overlap
    assert np.all(whole.data[41:60] == 0) and float(whole.start_time) == 0.75


def test_flag_errors(tmp_path):
    import run_efficiency_evaluate as ev
    inj = tmp_path / "inj.npz"
    np.savez(inj, tc=np.array([1.0]), distance=np.array([10.0]), mass1=np.ones(1), mass2=np.ones(1))
    base = ["--injection-file", str(inj)]
    with pytest.raises(ValueError, match="linear ranking statistic"):
        ev.main(base + ["--data-dir", str(tmp_path), "--ranking-statistic", "linear", "--test-data-activation", "softmax"])
    with pytest.raises(ValueError, match="Must provide a directory"):
        ev.main(base)
    with pytest.raises(ValueError, match="Duration required"):
        ev.main(base + ["--load-triggers", str(tmp_path / "t.npz")])
    with pytest.raises(ValueError, match="Duration required"):
        ev.main(base + ["--load-events", str(tmp_path / "e.npz")])
    open(ev.output_path(str(tmp_path / "statistics.hdf")), "wb").close()
    with pytest.raises(IOError, match="Cannot overwrite statistics file"):
        ev.main(base + ["--load-events", str(tmp_path / "e.npz"), "--duration", "10", "--data-dir", str(tmp_path)])
    p = ev.build_parser().parse_args(base)
    assert (p.trigger_threshold, p.cluster_tolerance, p.event_tolerance, p.delta_t, p.start_time_offset) == (0.1, 0.2, 0.3, 0.1, 0.75)
    assert (p.test_data_activation, p.ranking_statistic, p.trigger_file_name, p.event_file_name, p.stats_file_name) == \
        ("linear", "softmax", "triggers.hdf", "events.hdf", "statistics.hdf")


def test_processed_files_of_the_log(tmp_path):
    import run_efficiency_test as rt
    log = tmp_path / "log.txt"
    assert rt.get_already_processed_files(str(log)) == []
    log.write_text("INFO | x: Successfully saved output to /out/H1-0-10.hdf\nnoise\nSuccessfully saved output to /out/b.hdf\n")
    assert rt.get_already_processed_files(str(log)) == ["/out/H1-0-10.hdf", "/out/b.hdf"]
    p = rt.build_parser().parse_args(["--input-dir", "i", "--output-dir", "o", "--log-file", "l"])
    assert p.batch_size == 0 and p.device == "cuda" and not p.remove_softmax


# ---- refusals that need no GPU ------------------------------------------------------------------------------------------
def test_refusals_without_gpu():
    import torch
    E = gw_whisper_amd.GwwError
    inj, dist = np.array([1.0, 2.0]), np.array([10.0, 20.0])
    with pytest.raises(E, match="GPU"):
        ts.triggers(torch.zeros(4), 0.1, 0.0, 0.1)
    with pytest.raises(E, match="GPU"):
        ts.evaluate(torch.zeros(4, dtype=torch.float64), 0.1, 0.0, inj, dist)
    with pytest.raises(E, match="CPU tensor"):
        ts.events(torch.zeros(4, dtype=torch.float64), torch.zeros(4, dtype=torch.float64), 0.2)
    with pytest.raises(E, match="CPU tensor"):
        ts.statistics(torch.zeros(4, dtype=torch.float64), torch.zeros(4, dtype=torch.float64), inj, dist, 10.0, 0.3)
    with pytest.raises(E, match="GPU"):
        ts.score_windows(None, torch.zeros(2, 2048))
    with pytest.raises(E, match="no injection"):
        ts.statistics(np.zeros(3), np.zeros(3), np.zeros(0), np.zeros(0), 10.0, 0.3)
    with pytest.raises(E, match="NaN"):
        ts.statistics(np.zeros(3), np.zeros(3), np.array([1.0, np.nan]), dist, 10.0, 0.3)
    for bad in (0.0, -1.0, None):
        with pytest.raises(E, match="duration"):
            ts.statistics(np.zeros(3), np.zeros(3), inj, dist, bad, 0.3)
    with pytest.raises(E, match="not ascending"):
        ts.events(np.array([1.0, 0.5]), np.zeros(2), 0.2)
    assert issubclass(ts.NoTruePositive, E)
    assert all(len(a) == 0 for a in ts.events(np.zeros(0), np.zeros(0), 0.2))


def test_c_entry_points_refuse_before_any_launch():
    """Sizes above 2^27, NULL pointers and undersized workspaces come back as argument errors; no HIP call is made, so
    this runs without a GPU (the pointers are never dereferenced)."""
    lib = gw_whisper_amd.lib()
    p = C.c_void_p(4096)
    big = (1 << 27) + 1
    for f in ("triggers", "events", "split", "steps"):
        assert getattr(lib, f"gww_trig_{f}_workspace_bytes")(big) == 0 and getattr(lib, f"gww_trig_{f}_workspace_bytes")(0) == 0
        assert getattr(lib, f"gww_trig_{f}_workspace_bytes")(1 << 27) > 0
    assert lib.gww_trig_triggers_f64(p, 1, big, 1, 0.1, 0.0, 0.1, p, p, p, p, 1 << 40, None) == -1
    assert b"2^27" in lib.gww_last_error()
    assert lib.gww_trig_triggers_f64(None, 1, 8, 8, 0.1, 0.0, 0.1, p, p, p, p, 1 << 20, None) == -1
    assert b"NULL" in lib.gww_last_error()
    assert lib.gww_trig_triggers_f64(p, 2, 8, 8, 0.1, 0.0, 0.1, p, p, p, p, 1 << 20, None) == -1
    need = lib.gww_trig_triggers_workspace_bytes(70001)
    assert lib.gww_trig_triggers_f64(p, 1, 70001, 70001, 0.1, 0.0, 0.1, p, p, p, p, need - 1, None) == -1
    assert b"workspace" in lib.gww_last_error()
    assert lib.gww_trig_events_f64(p, p, None, big, 0.2, p, p, p, p, 1 << 40, None) == -1
    assert lib.gww_trig_events_f64(p, p, None, 5000, 0.2, p, p, p, p, lib.gww_trig_events_workspace_bytes(5000) - 1, None) == -1
    assert b"workspace" in lib.gww_last_error()
    assert lib.gww_trig_split_f64(p, p, None, 5000, 0.3, p, p, p, p, lib.gww_trig_split_workspace_bytes(5000) - 1, None) == -1
    assert b"workspace" in lib.gww_last_error()
    assert lib.gww_trig_steps_f64(p, p, 5000, p, p, 5000, 10.0, 1.0, 3.0, p, p, p, p, p, p, p,
                                  lib.gww_trig_steps_workspace_bytes(5000) - 1, None) == -1
    assert b"workspace" in lib.gww_last_error()
    assert lib.gww_trig_steps_f64(p, p, 5000, p, p, 5000, 0.0, 1.0, 3.0, p, p, p, p, p, p, p, 1 << 30, None) == -1
    assert b"duration" in lib.gww_last_error()
    from gw_whisper_amd import _lib
    five = (_lib.C.c_void_p * 5)(*([p] * 5))
    P = _lib.C.byref(_lib.MlpParams(5, five, five))
    assert lib.gww_det_head_scores2_f32(p, P, 4, 128, 2, 2, p, 2, None) == -1
    assert b"mode" in lib.gww_last_error()
    assert lib.gww_det_head_scores2_f32(p, P, 4, 128, 2, 0, p, 1, None) == -1
    assert b"out_stride" in lib.gww_last_error()
