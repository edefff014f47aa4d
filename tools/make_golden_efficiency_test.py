#!/usr/bin/env python3
"""Write tests/golden/efficiency_test.npz by running the REFERENCE's own code: ``get_triggers`` is taken out of
``Signal_vs_Noise/Efficiency_test/bnslib.py`` and ``get_cluster_boundaries``, ``custom_get_event_list_from_triggers``,
``split_true_and_false_positives`` and ``get_closest_injection_times`` out of ``src/evaluate_test_data.py`` with ``ast``
where the files lie, together with the statements of its ``main`` from the ``split_true_and_false_positives`` call to the
end of the ``for idx in tidxs`` loop, and executed; the modules themselves are never imported (they import ``pycbc`` and
``h5py``, which this project does without), and nothing of their text is stored: only the OUTPUTS the reference computes
plus numpy's version.  The reference's ``TimeSeries`` is ``gw_whisper_amd.trigger_stats.TimeSeries``, the project's
stand-in for the (data, delta_t, epoch) container.  The inputs are regenerated from seeds by tests/trigger_stats_helpers.py.

Per case and threshold the file holds ``c<case>_t<10 * threshold>_<array>`` for the arrays of ``helpers.ARRAYS`` and
``..._refused`` (1 where the reference dies on ``tptimes, tpvals = tp.T``: then only the trigger and event arrays).  The tool
asserts what the cases are there for: both branches of the first-ranking-step quirk, a true positive everywhere but in
the refused case, the 5000-trigger cluster, both sides of the cluster tolerance in the hand-made case.

``--time``: also print how long the reference's functions take on the largest case (profiles/trigger_stats.md).

usage: make_golden_efficiency_test.py [--reference DIR] [--out FILE] [--time]"""
import argparse
import ast
import logging
import os
import sys
import time
import types
from queue import Queue

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from gw_whisper_amd.trigger_stats import TimeSeries  # noqa: E402
from tests import trigger_stats_helpers as th  # noqa: E402

BNSLIB = ("get_triggers",)
EVALUATE = ("get_cluster_boundaries", "custom_get_event_list_from_triggers", "split_true_and_false_positives",
            "get_closest_injection_times")


def _functions(path, wanted):
    tree = ast.parse(open(path).read(), filename=path)
    funcs = {n.name: n for n in tree.body if isinstance(n, ast.FunctionDef)}
    missing = [n for n in wanted if n not in funcs]
    assert not missing, f"{path} no longer defines {missing}"
    return tree, funcs


def _calls(node, name):
    return any(isinstance(n, ast.Call) and isinstance(n.func, ast.Name) and n.func.id == name for n in ast.walk(node))


def reference_code(ref):
    """(the namespace holding the reference's functions, the compiled statistics statements of its main)."""
    base = os.path.join(ref, "Signal_vs_Noise", "Efficiency_test")
    ns = {"np": np, "logging": logging, "Queue": Queue, "SEC_PER_MONTH": th.SEC_PER_MONTH}
    for path, wanted in ((os.path.join(base, "bnslib.py"), BNSLIB), (os.path.join(base, "src", "evaluate_test_data.py"), EVALUATE)):
        _, funcs = _functions(path, wanted)
        exec(compile(ast.fix_missing_locations(ast.Module(body=[funcs[n] for n in wanted], type_ignores=[])), path, "exec"), ns)
    tree, funcs = _functions(path, ("main",))
    body = funcs["main"].body
    first = [i for i, s in enumerate(body) if isinstance(s, ast.Assign) and _calls(s, "split_true_and_false_positives")]
    last = [i for i, s in enumerate(body) if isinstance(s, ast.For) and isinstance(s.iter, ast.Name) and s.iter.id == "tidxs"]
    assert len(first) == 1 and len(last) == 1 and first[0] < last[0], f"{path}: main no longer has the statistics statements"
    stats = compile(ast.fix_missing_locations(ast.Module(body=body[first[0]:last[0] + 1], type_ignores=[])), path, "exec")
    return ns, stats


def run_reference(ns, stats, c, threshold, clock=None):
    """The arrays of th.ARRAYS (None for the statistics where the reference dies without a true positive)."""
    t0 = time.perf_counter()
    ts = TimeSeries(c["series"], delta_t=c["delta_t"], epoch=c["epoch"])
    triggers = ns["get_triggers"](ts, threshold)
    cb = ns["get_cluster_boundaries"](triggers, boundarie_time=th.CLUSTER_TOL)
    events = ns["custom_get_event_list_from_triggers"](triggers, cb)
    out = {"trig_times": np.asarray(triggers[0], np.float64), "trig_values": np.asarray(triggers[1], np.float64),
           "ev_times": np.array([e[0] for e in events], np.float64), "ev_values": np.array([e[1] for e in events], np.float64)}
    env = dict(ns)
    env.update(events=events, inj_times=c["inj"], dist=c["dist"],
               args=types.SimpleNamespace(event_tolerance=th.EVENT_TOL, duration=ts.duration, verbose=False))
    try:
        exec(stats, env)
    except ValueError as e:
        assert "not enough values to unpack" in str(e), e
        return out, None, cb
    for k, name in (("ranking", "rank"), ("far", "far"), ("sens-frac", "sens_frac"), ("sens-dist", "sens_dist"),
                    ("sens-vol", "sens_vol"), ("sens-vol-err", "sens_vol_err")):
        out[k] = np.array(env[name], np.float64)
    if clock is not None:
        clock.append(time.perf_counter() - t0)
    return out, env, cb


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reference", default=os.path.join(os.path.dirname(ROOT), "reference"),
                    help="the reference checkout (default: the directory `reference` beside this repository)")
    ap.add_argument("--out", default=th.GOLD)
    ap.add_argument("--time", action="store_true")
    args = ap.parse_args()
    ns, stats = reference_code(args.reference)
    out = {"numpy_version": np.asarray(np.__version__)}
    first_run = {}
    for ci in range(th.n_cases()):
        c = th.case(ci)
        for thr in th.THRESHOLDS:
            clock = []
            with np.errstate(invalid="ignore"):
                res, env, cb = run_reference(ns, stats, c, thr, clock)
            refused = env is None
            assert refused == ((ci, thr) in th.REFUSED), f"case {ci} at {thr}: refused = {refused}"
            out[th.key(ci, thr, "refused")] = np.asarray(int(refused))
            for k, v in res.items():
                out[th.key(ci, thr, k)] = v
            if refused:
                print(f"case {ci} at {thr}: {len(res['trig_times'])} triggers, no true positive: the reference dies")
                continue
            fp = np.array([e[1] for e in env["fp"]])
            first_run[(ci, thr)] = int(np.sum(fp == fp[0])) if len(fp) else 0
            assert len(env["tp"]) >= 1
            if ci < th.HAND and th.CASES[ci][2] and thr == 0.1:
                longest = max(int(np.searchsorted(res["trig_times"], b, "right") - np.searchsorted(res["trig_times"], a, "left"))
                              for a, b in cb)
                assert longest >= th.CASES[ci][2] > 4096, f"case {ci}: the longest cluster has {longest} triggers"
            print(f"case {ci} at {thr}: n={len(c['series'])} triggers {len(res['trig_times'])} events {len(res['ev_times'])} "
                  f"true positives {len(env['tp'])} false positives {len(env['fp'])} steps {len(res['ranking'])} "
                  f"first run {first_run[(ci, thr)]}" + (f" reference {clock[0]:.2f} s" if args.time else ""))
    assert first_run[(1, 0.5)] == 1 and first_run[(2, 0.5)] > 1 and first_run[(th.HAND, 0.1)] == 1, \
        f"the first ranking runs {first_run} miss a branch of the quirk"
    hand = th.case(th.HAND)
    tt = out[th.key(th.HAND, 0.1, "trig_times")]
    two = np.flatnonzero(np.round((tt[1:] - tt[:-1]) / hand["delta_t"]) == 2)
    gaps = (tt[1:] - tt[:-1])[two]
    assert np.any(gaps < th.CLUSTER_TOL) and np.any(gaps >= th.CLUSTER_TOL), "the hand-made case misses a side of the tolerance"
    np.savez_compressed(args.out, **out)
    size = os.path.getsize(args.out)
    print(f"wrote {args.out}: {size} bytes")
    assert size <= 1 << 20, "the golden file exceeds 1 MiB"


if __name__ == "__main__":
    main()
