"""The ordered compactions of csrc/device_compact.h at their seams, through the entry points that use them: the events
and injections of ``score_match`` around one workgroup of 1024 and with one list empty, ``trig_split`` and ``trig_steps``
with whole trailing workgroups behind the device's count, ``trig_triggers`` with more triggers than capacity.  The
references are numpy and the restatements of tests/search_score_helpers.py and tests/trigger_stats_helpers.py; every
comparison is ``==``."""

import numpy as np
import pytest

from tests.guard import run_contract

from . import search_score_helpers as sh
from . import trigger_stats_helpers as th

pytestmark = pytest.mark.gpu

WG = 1024
MODULES = ("gw_whisper_amd.ops",)


@pytest.fixture(scope="module")
def T():
    import torch
    assert torch.cuda.is_available()
    return torch


# ---- score_match --------------------------------------------------------------------------------------------------------
def _match(T, fg, bg, inj, duration):
    """The keys of EXACT_KEYS from ``score_sort`` / ``score_match`` / ``score_far`` called directly (``get_stats`` refuses
    a search without a true positive), plus the injections' lists and the counts."""
    from gw_whisper_amd import ops
    ev = T.from_numpy(np.ascontiguousarray(fg)).cuda()
    order, _, _ = ops.score_sort(ev[0])
    m = ops.score_match(ev, order, T.from_numpy(np.asarray(inj["tc"], np.float64)).cuda())
    E, B = fg.shape[1], bg.shape[1]
    fg_far = ops.score_far(E, duration, ev.device, n_dev=m["counts"][1:2])
    far = ops.score_far(B, duration, ev.device)
    n_tp, n_fp, n_f, n_m, n_nan = (int(v) for v in m["counts"].cpu().numpy())
    assert n_nan == 0 and n_tp + n_fp == E

    def host(t, dtype=None):
        a = t.cpu().numpy()
        return a if dtype is None else a.astype(dtype)
    return {"fg-events": host(m["fg_sorted"]), "found-indices": host(m["found_idx"], np.int64),
            "missed-indices": host(m["missed"][:n_m], np.int64),
            "true-positive-event-indices": host(m["tp_idx"][:n_tp], np.int64),
            "false-positive-event-indices": host(m["fp_idx"][:n_fp], np.int64), "sorting-indices": host(order, np.int64),
            "true-positive-diffs": host(m["tp_diff"][:n_tp]), "false-positive-diffs": host(m["fp_diff"][:n_fp]),
            "true-positives": host(m["tp_events"][:, :n_tp]), "false-positives": host(m["fp_events"][:, :n_fp]),
            "fg-far": host(fg_far[:n_fp]), "far": host(far),
            "_found_inj": host(m["found_inj"][:n_f], np.int64), "_found_stat": host(m["found_stat"][:n_f])}


def _check_match(T, fg, bg, inj, duration):
    got = _match(T, fg, bg, inj, duration)
    ref = sh.restate(fg, bg, inj, duration)
    for k in sh.EXACT_KEYS:
        a, b = got[k], np.asarray(ref[k])
        assert a.shape == b.shape, f"{k} has shape {a.shape}, expected {b.shape}"
        assert np.array_equal(a, b), f"{k} differs"
    # the found injections in index order with their best true-positive statistic
    tpi, idx, stat = ref["true-positive-event-indices"], ref["found-indices"], ref["fg-events"][1]
    found = np.unique(idx[tpi])
    best = np.full(len(inj["tc"]), -np.inf)
    np.maximum.at(best, idx[tpi], stat[tpi])
    assert np.array_equal(got["_found_inj"], found) and np.array_equal(got["_found_stat"], best[found])
    return got, ref


@pytest.mark.parametrize("N", (WG - 1, WG, WG + 1))
@pytest.mark.parametrize("E", (WG - 1, WG, WG + 1))
def test_score_match_at_the_workgroup_seam(T, gww, E, N):
    fg, bg, inj, duration = sh.make_case(E, 3, N, 8100 + 3 * E + N)
    got, _ = _check_match(T, fg, bg, inj, duration)
    assert len(got["true-positive-event-indices"]) and len(got["false-positive-event-indices"])
    assert len(got["missed-indices"]) and len(got["_found_inj"])


E_DEG = 2 * WG + 1


def _every_event_a_true_positive():
    fg, bg, inj, duration = sh.make_case(E_DEG, 3, 300, 8201)
    rng = np.random.default_rng(8202)
    fg[0] = inj["tc"][rng.integers(0, 300, E_DEG)] + rng.uniform(-0.05, 0.05, E_DEG)
    fg[2] = 0.2
    return fg, bg, inj, duration


def _every_event_a_false_positive():
    fg, bg, inj, duration = sh.make_case(E_DEG, 3, 300, 8203)
    fg[2] = 0.0                                     # var = 0: only an event on an injection would be a true positive
    assert not np.isin(fg[0], inj["tc"]).any()
    return fg, bg, inj, duration


def _every_injection_missed():
    """All events lie before the first injection and outside their var: injection 0 owns them all (a run of false
    positives: neither found nor missed), every other injection has an empty run."""
    fg, bg, inj, duration = sh.make_case(E_DEG, 3, E_DEG, 8204)
    rng = np.random.default_rng(8205)
    fg[0] = inj["tc"][0] - 1.0 - np.sort(rng.uniform(0.0, 40.0, E_DEG))
    return fg, bg, inj, duration


def _a_workgroup_of_true_positives_between_mixed_ones():
    fg, bg, inj, duration = sh.make_case(3 * WG + 1, 3, 300, 8206)
    fg[2, np.argsort(fg[0], kind="stable")[WG:2 * WG]] = 1e9
    return fg, bg, inj, duration


# name: (the case, the numbers of true positives, false positives and missed injections it was built for)
DEGENERATE = {"all true": (_every_event_a_true_positive, (E_DEG, 0, None)),
              "all false": (_every_event_a_false_positive, (0, E_DEG, None)),
              "all missed": (_every_injection_missed, (0, E_DEG, E_DEG - 1)),
              "one workgroup all true": (_a_workgroup_of_true_positives_between_mixed_ones, (None, None, None))}


@pytest.mark.parametrize("name", sorted(DEGENERATE))
def test_score_match_with_a_list_empty(T, gww, name):
    make, (n_tp, n_fp, n_missed) = DEGENERATE[name]
    fg, bg, inj, duration = make()
    assert np.unique(fg[0]).size == fg.shape[1]
    got, ref = _check_match(T, fg, bg, inj, duration)
    for want, k in ((n_tp, "true-positive-event-indices"), (n_fp, "false-positive-event-indices"), (n_missed, "missed-indices")):
        assert want is None or len(got[k]) == want, f"{name}: {len(got[k])} {k}, the case was built for {want}"
    if name == "one workgroup all true":
        fpi = ref["false-positive-event-indices"]
        assert (fpi < WG).any() and (fpi >= 2 * WG).any() and not ((fpi >= WG) & (fpi < 2 * WG)).any()


# ---- trig_split / trig_steps ----------------------------------------------------------------------------------------------
CAPS = (1, WG - 1, WG, WG + 1, 3 * WG + 1)


def _counts(cap):
    """the device's count: the whole capacity, and one that leaves whole trailing workgroups empty"""
    return (cap,) + ((cap - 700,) if cap > 700 else ())


@pytest.mark.parametrize("cap", CAPS)
def test_trig_split_behind_a_device_count(T, gww, cap):
    from gw_whisper_amd import ops
    rng = np.random.default_rng(8300 + cap)
    tol = 0.3
    values = np.round(rng.random(cap), 3)
    diff = rng.choice([0.0, np.nextafter(tol, 0.0), tol, np.nextafter(tol, 1.0), 2 * tol], cap)
    diff[0] = tol                                   # equality counts
    for n in _counts(cap):
        n_dev = T.tensor([n], dtype=T.int32, device="cuda") if n < cap else None
        tp, fp, c = ops.trig_split(T.from_numpy(values).cuda(), T.from_numpy(diff).cuda(), tol, n_dev=n_dev)
        keep = diff[:n] <= tol
        ref_tp, ref_fp = values[:n][keep], values[:n][~keep]
        assert c.tolist() == [len(ref_tp), len(ref_fp), 0]
        assert np.array_equal(tp[:len(ref_tp)].cpu().numpy(), ref_tp) and np.array_equal(fp[:len(ref_fp)].cpu().numpy(), ref_fp)


@pytest.mark.parametrize("cap", CAPS)
def test_trig_steps_behind_a_device_count(T, gww, cap):
    """ranking and far pin the compacted starts: ranking[s] = v[start[s]], far[s] counts the values behind the run's end,
    which is the next start"""
    from gw_whisper_amd import ops
    rng = np.random.default_rng(8400 + cap)
    v = np.sort(np.round(rng.random(cap) * (cap / 5.0 + 1)))      # runs of about five equal values
    for seam in range(WG, cap, WG):                 # a run of equal values across every workgroup seam
        v[seam - 7:seam + 7] = v[seam - 7]
    assert np.all(np.diff(v) >= 0)
    tp = np.sort(np.round(rng.random(17) * (cap / 5.0 + 1)))
    duration = 1000.0
    for n in _counts(cap):
        if n > WG:
            assert v[WG - 1] == v[WG]
        n_fp = T.tensor([n], dtype=T.int32, device="cuda")
        n_tp = T.tensor([len(tp)], dtype=T.int32, device="cuda")
        ranking, far, _, _, _, n_steps = ops.trig_steps(T.from_numpy(v).cuda(), n_fp, T.from_numpy(tp).cuda(), n_tp, duration,
                                                        1.0, 40.0)
        _, starts = np.unique(v[:n], return_index=True)
        ends = np.r_[starts[1:], n] - 1
        count = n - ends - 1
        if ends[0] == 0:
            count[0] = n
        S = len(starts)
        assert int(n_steps) == S
        assert np.array_equal(ranking[:S].cpu().numpy(), v[starts])
        assert np.array_equal(far[:S].cpu().numpy(), count / duration * th.SEC_PER_MONTH)


# ---- trig_triggers ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ("float32", "float64"))
def test_trig_triggers_one_short_of_capacity(T, gww, dtype):
    """More triggers than ``cap``: all are counted, the first ``cap`` are stored, nothing is stored behind the outputs."""
    from gw_whisper_amd import ops
    n, thr = 2 * 4096 + 805, 0.1                    # three workgroups of 4096 samples
    c = th.make_case(n, 40, 0, 8500, 0.75)
    series = c["series"].astype(dtype)
    ref_t, ref_v = th.triggers(series, c["delta_t"], c["epoch"], thr)
    K = len(ref_t)
    assert K > 2 and (np.flatnonzero(series.astype(np.float64) > thr) >= 2 * 4096).sum() > 1
    cap = K - 1
    series_d = T.from_numpy(series).cuda()

    def case(g):
        t, v, counts = ops.trig_triggers(g.place(series_d), c["delta_t"], c["epoch"], thr, cap=cap)
        return {"times": t, "values": v, "counts": counts}
    r = run_contract(case, modules=MODULES)
    assert r["counts"].tolist() == [K, 0]
    assert r["times"].shape == (cap,) and r["values"].shape == (cap,)
    assert np.array_equal(r["times"].cpu().numpy(), ref_t[:cap]) and np.array_equal(r["values"].cpu().numpy(), ref_v[:cap])
