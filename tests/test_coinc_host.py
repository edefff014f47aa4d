"""Host side of the single-detector coincident search (gw_whisper_amd/coinc.py, harness/run_coinc_search.py): the numpy
oracle ``coinc_host`` against a brute-force double loop, the boundary of the pair predicate, the three tie-breaks of the
partner rule, the one-to-one property, ``slide_shifts`` and the harness's refusals and file layout.  No GPU."""

import importlib.util
import os

import numpy as np
import pytest

from gw_whisper_amd import GwwError, coinc

from . import coinc_helpers as ch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _harness(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "harness", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _host(c, window):
    return coinc.coinc_host(c["t0"], c["v0"], c["t1"], c["v1"], c["shifts"], window)


@pytest.mark.parametrize("step", ch.STEPS)
@pytest.mark.parametrize("N,q", ch.CASES)
def test_generator_cases_are_not_empty(N, q, step):
    """The cap that keeps every test below (and on the GPU) from passing on empty lists: at least one zero-lag coincidence
    at window 0.15, and for N >= 600 a coincidence in at least half of the slides."""
    c = ch.make_case(N, q, step)
    assert len(c["shifts"]) == 1 + min(300, (N - 11) // 20)
    per_slide = np.diff(_host(c, ch.WINDOW)["offsets"])
    print(f"N={N} step={step!r}: events {len(c['t0'])} / {len(c['t1'])}, zero lag {per_slide[0]}, non-empty slides "
          f"{int((per_slide[1:] > 0).sum())} / {len(per_slide) - 1}")
    assert per_slide[0] >= 1
    if N >= 600:
        assert 2 * int((per_slide[1:] > 0).sum()) >= len(per_slide) - 1
    # neighbouring events of one detector lie more than the cluster threshold apart
    for t in (c["t0"], c["t1"]):
        assert len(t) >= 2 and (np.diff(t) > ch.CLUSTER_THRESHOLD).all()


@pytest.mark.parametrize("step", ch.STEPS)
@pytest.mark.parametrize("N,q", ch.CASES)
def test_oracle_equals_the_double_loop(N, q, step):
    c = ch.make_case(N, q, step)
    for window in (ch.WINDOW, step, 0.05):
        got = _host(c, window)
        ref = ch.brute_force(c["t0"], c["v0"], c["t1"], c["v1"], c["shifts"], window)
        assert got["offsets"][0] == 0 and np.array_equal(np.diff(got["offsets"]), [len(r[0]) for r in ref])
        for s, (i, j, d) in enumerate(ref):
            a, b = got["offsets"][s], got["offsets"][s + 1]
            assert np.array_equal(got["idx0"][a:b], i) and np.array_equal(got["idx1"][a:b], j)
            assert np.array_equal(got["dt"][a:b], d)
            assert np.array_equal(got["time"][a:b], c["t0"][i])
            assert np.array_equal(got["stat"][a:b], c["v0"][i].astype(np.float64) + c["v1"][j].astype(np.float64))
        assert got["idx0"].dtype == np.int32 and got["idx1"].dtype == np.int32 and got["offsets"].dtype == np.int64
        if window in (ch.WINDOW, 0.05):
            # one to one under 2 * window < cluster_threshold: no detector-1 event twice within a slide
            assert 2 * window < ch.CLUSTER_THRESHOLD
            for s in range(len(ref)):
                j = got["idx1"][got["offsets"][s]:got["offsets"][s + 1]]
                assert len(np.unique(j)) == len(j)


def test_rule_breaking_lists_equal_the_double_loop():
    t0, v0, t1, v1 = ch.rule_breaking()
    shifts = np.array([0.0, 0.125, 0.3, 1.0])
    for window in (0.0625, 0.15, 0.1875, 0.5):
        got = coinc.coinc_host(t0, v0, t1, v1, shifts, window)
        ref = ch.brute_force(t0, v0, t1, v1, shifts, window)
        for s, (i, j, d) in enumerate(ref):
            a, b = got["offsets"][s], got["offsets"][s + 1]
            assert np.array_equal(got["idx0"][a:b], i) and np.array_equal(got["idx1"][a:b], j) and np.array_equal(got["dt"][a:b], d)
    assert len(got["idx1"]) > len(np.unique(got["idx1"][:got["offsets"][1]]))      # a detector-1 event IS chosen twice here


def test_boundary_counts():
    """fabs(d) == window exactly is a coincidence; the next smaller window is none.  On both sides of detector 0, and
    with the shift's addition in the predicate."""
    t0 = np.array([1000.5])
    for t1, o in (([1000.625], 0.0), ([1000.375], 0.0), ([990.625], 10.0), ([1000.6], 0.0), ([1000.4], 0.0)):
        t1 = np.array(t1)
        window = float(np.fabs((t1[0] + o) - t0[0]))
        got = coinc.coinc_host(t0, [1.0], t1, [2.0], [o], window)
        assert got["offsets"].tolist() == [0, 1] and got["idx1"].tolist() == [0] and abs(got["dt"][0]) == window
        assert got["stat"][0] == 3.0 and got["time"][0] == t0[0]
        got = coinc.coinc_host(t0, [1.0], t1, [2.0], [o], float(np.nextafter(window, 0.0)))
        assert got["offsets"].tolist() == [0, 0] and len(got["time"]) == 0


def test_partner_rule_tie_breaks_in_order():
    t0, v0 = np.array([1000.0]), np.array([0.5], np.float32)
    t1 = np.array([999.75, 999.875, 1000.0625, 1000.125, 1000.25])

    def partner(v1, window=0.3):
        return coinc.coinc_host(t0, v0, t1, np.array(v1, np.float32), [0.0], window)["idx1"].tolist()

    assert partner([1, 1, 1, 1, 5]) == [4]            # the largest v1 wins, however far and however late
    assert partner([5, 1, 1, 1, 5]) == [0]            # equal v1, equal fabs(d) = 0.25: the smaller j
    assert partner([1, 3, 1, 3, 1]) == [1]            # equal v1, equal fabs(d) = 0.125: the smaller j again
    assert partner([1, 3, 3, 1, 1]) == [2]            # equal v1: the smaller fabs(d), 0.0625 against 0.125 ...
    assert partner([1, 1, 3, 3, 1]) == [2]
    assert partner([3, 1, 1, 3, 1]) == [3]            # ... although the other candidate comes first
    assert partner([3, 2, 9, 2, 3], window=0.05) == []
    assert partner([3, 2, 1, 2, 3], window=0.13) == [1]          # v1 is compared among the coincident events only


def test_empty_lists():
    e, f = np.zeros((0,)), np.zeros((0,), np.float32)
    for a, b in (((e, f), (np.array([1.0]), np.array([1.0], np.float32))), ((np.array([1.0]), np.array([1.0], np.float32)), (e, f)),
                 ((e, f), (e, f))):
        got = coinc.coinc_host(*a, *b, [0.0, 2.0], 0.15)
        assert got["offsets"].tolist() == [0, 0, 0] and all(len(got[k]) == 0 for k in ("time", "stat", "dt", "idx0", "idx1"))


# ---------------------------------------------------------------------------------------------- slide_shifts
@pytest.mark.parametrize("N,step,tstep", [(600, 0.1, 204.0 / 2048.0), (37, 0.1, 204.0 / 2048.0), (5000, 0.1, 0.1), (11, 0.1, 0.1)])
def test_slide_shifts_existence_and_livetime(N, step, tstep):
    S, shift, slice_seconds = 40, 2.0, 1.0
    plan = coinc.slide_shifts(N, step, shift, S, slice_seconds, tstep, window=0.15)
    assert plan.k == 20 and plan.n_slides == S and plan.livetime.shape == (S,)
    exists = [s for s in range(1, S + 1) if s * 20 * tstep < N * tstep - slice_seconds]
    assert list(plan.slides) == exists
    assert list(plan.shifts) == [s * 20 * tstep for s in exists]
    for s in range(1, S + 1):
        assert plan.livetime[s - 1] == (N * tstep - s * 20 * tstep if s in exists else 0.0)
    if N == 600:
        assert len(exists) == 29
    if N == 11:
        assert exists == []
    default = coinc.slide_shifts(N, step, shift, S, slice_seconds)
    assert list(default.shifts) == [s * 20 * step for s in default.slides]


def test_slide_shifts_refusals():
    with pytest.raises(GwwError, match="whole number of steps"):
        coinc.slide_shifts(600, 0.1, 2.05, 5, 1.0)
    with pytest.raises(GwwError, match="same second of sky"):
        coinc.slide_shifts(600, 0.1, 1.1, 5, 1.0, window=0.15)           # 1.1 <= 1.0 + 0.15
    with pytest.raises(GwwError, match="same second of sky"):
        coinc.slide_shifts(600, 0.1, 1.0, 5, 1.0)                        # equality is refused
    coinc.slide_shifts(600, 0.1, 1.2, 5, 1.0, window=0.15)
    for n in (0, -3):
        with pytest.raises(GwwError, match="n_slides"):
            coinc.slide_shifts(600, 0.1, 2.0, n, 1.0)
    with pytest.raises(GwwError, match="step_size"):
        coinc.slide_shifts(600, 0.0, 2.0, 5, 1.0)


# ---------------------------------------------------------------------------------------------- the harness, host only
@pytest.fixture(scope="module")
def rcs():
    return _harness("run_coinc_search")


def test_harness_argument_errors(rcs, tmp_path, monkeypatch, capsys):
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    out = str(tmp_path / "o.npz")
    base = ["none", out, "--synthetic", "30", "--white"]
    for extra, text in ((["--detectors", "H1", "--time-slides", "3", "--slides-output", str(tmp_path / "b.npz")], "two detectors"),
                        (["--detectors", "L1", "--time-slides", "3"], "two detectors"),
                        (["--time-slides", "3"], "--slides-output"),
                        (["--time-slides", "-1"], ">= 0"),
                        (["--detectors", "H1", "H1"], "twice"),
                        (["--coinc-window", "0.2"], "--cluster-threshold"),
                        (["--coinc-window", "0.175"], "--cluster-threshold"),          # 2 * 0.175 == 0.35: refused
                        (["--coinc-window", "-0.1"], "negative"),
                        (["--lora-weights", "a", "b", "c", "--dense-weights", "a", "b", "c"], "one per detector"),
                        (["--detectors", "H1", "--lora-weights", "a", "b", "--dense-weights", "a", "b"], "one per detector"),
                        (["--lora-weights", "a"], "--dense-weights")):
        with pytest.raises(SystemExit) as e:
            rcs.main(base + extra)
        assert text in str(e.value), (extra, str(e.value))
    with pytest.raises(SystemExit):
        rcs.parse_args(base + ["--detectors", "V1"])
    # one detector without slides and the default two-detector run get as far as the GPU check
    import torch
    if not torch.cuda.is_available():
        for extra in (["--detectors", "L1"], [], ["--time-slides", "3", "--slides-output", str(tmp_path / "b.npz")]):
            with pytest.raises(SystemExit, match="no GPU"):
                rcs.main(base + extra)
    open(out, "wb").close()
    with pytest.raises(RuntimeError, match="Output file exists"):
        rcs.main(base)
    assert rcs.parse_args(base).coinc_window == 0.15
    with pytest.raises(SystemExit):
        rcs.parse_args(["--help"])
    assert "one and a half steps" in " ".join(capsys.readouterr().out.split())


def test_harness_refuses_more_than_one_rank(rcs, tmp_path, monkeypatch):
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(SystemExit, match="one rank only"):
        rcs.main(["none", str(tmp_path / "o.npz"), "--synthetic", "30", "--white"])


def test_background_file_has_the_layout_of_run_inference_slides(rcs, tmp_path):
    """The six datasets, names and dtypes, of ``run_inference.py --slides-output`` -- built there from ``slide_background``'s
    columns, here from ``search_segment``'s -- written through the same ``write_result`` and read back."""
    ri = _harness("run_inference")
    S = 4
    live = np.array([58.0, 56.0, 54.0, 0.0])
    cols = [np.array([1000.6, 1003.1]), np.array([2.5, -0.25]), np.full((2,), 0.2), np.array([1, 3], np.int32)]
    # run_inference.get_triggers, `slides = {...}`, on columns of the types time_slides.slide_background returns
    theirs = {"time": cols[0], "stat": cols[1], "var": cols[2], "slide": cols[3].astype(np.int32),
              "slide_livetime": live, "livetime": np.float64(live.sum())}
    ours = rcs.background_dict(cols, live)
    assert list(ours) == list(theirs) and len(ours) == 6
    for k in theirs:
        assert np.asarray(ours[k]).dtype == np.asarray(theirs[k]).dtype and np.array_equal(ours[k], theirs[k]), k
    assert ours["slide"].dtype == np.int32 and ours["slide_livetime"].shape == (S,)
    path = str(tmp_path / "b.npz")
    assert rcs.ri.write_result.__code__.co_code == ri.write_result.__code__.co_code       # imported, not restated
    rcs.ri.write_result(path, ours)
    z = np.load(path)
    assert sorted(z.files) == sorted(theirs)
    for k in theirs:
        assert z[k].dtype == np.asarray(theirs[k]).dtype and np.array_equal(z[k], theirs[k])
    # ... and an empty background keeps the types
    empty = rcs.background_dict([np.zeros((0,)), np.zeros((0,)), np.zeros((0,)), np.zeros((0,), np.int32)], np.zeros((S,)))
    assert empty["slide"].dtype == np.int32 and empty["time"].dtype == np.float64 and float(empty["livetime"]) == 0.0
