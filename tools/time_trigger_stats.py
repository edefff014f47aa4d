#!/usr/bin/env python3
"""Time the efficiency study's test-stage evaluation (gw_whisper_amd/trigger_stats.py) at a month of test data and at a
tenth of it, beside the vectorised numpy restatement (tests/trigger_stats_helpers.py) on the same host: the numbers of
profiles/trigger_stats.md.

Per size: the device time of the launches of one ``evaluate`` (HIP events around the chain of ``ops`` calls, no read) and
the wall time of ``evaluate`` from the call to the last array on the host, seven repeats each after one warm-up, median
and range; the restatement's wall time, three repeats.  The series has a trigger fraction of about 1e-3 at threshold 0.1;
one injection per 100 s, each with a loud sample on it.  The reference's own functions are timed on the fixture's cases by
``tools/make_golden_efficiency_test.py --time``.

``--stages`` prints instead, per size, the device time of every stage of that chain (HIP events between the ``ops`` calls,
nothing read back in between; medians of the repeats): the figures of profiles/device_compact.md.

``--capacity C`` makes room for C triggers instead of one per sample (``evaluate(capacity=C)``): every later stage -- the
events, the nearest-injection search, the two sorts, the ranking steps -- then runs over C elements.

usage: time_trigger_stats.py [--sizes N ...] [--repeats R] [--capacity C] [--stages]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import trigger_stats_helpers as th  # noqa: E402

MONTH = 25920000          # samples of 30 days at delta_t = 0.1


def make(n, seed=7):
    rng = np.random.default_rng(seed)
    series = np.round(0.1 * rng.random(n), 3)
    loud = rng.random(n) < 1e-3
    series[loud] = np.round(0.1 + 0.9 * rng.random(int(loud.sum())), 2) + 0.01
    at = np.arange(500, n, 1000)
    series[at] = np.round(0.5 + 0.5 * rng.random(len(at)), 2)
    inj = at * th.DELTA_T + 0.75 + rng.uniform(-0.04, 0.04, len(at))
    return {"series": series, "delta_t": th.DELTA_T, "epoch": 0.75, "inj": inj, "dist": rng.uniform(10.0, 500.0, len(at))}


def spread(ts):
    return f"{statistics.median(ts) * 1e3:.2f} ms ({min(ts) * 1e3:.2f} .. {max(ts) * 1e3:.2f})"


def staged(torch, ops, series, c, inj_sorted, prefactor, Ninj, capacity):
    """The chain stage by stage; returns {stage: ms} from device events, 'enqueue' = the whole.  Mirrors ``chain`` in
    ``main`` with ``trigger_stats._statistics_device`` written out call by call: keep the three in step."""
    marks = []

    def mark(name):
        ev = torch.cuda.Event(enable_timing=True)
        ev.record()
        marks.append((name, ev))
    mark("start")
    t, v, ct = ops.trig_triggers(series, c["delta_t"], c["epoch"], 0.1, cap=capacity)
    mark("triggers")
    et, ev, ce = ops.trig_events(t, v, th.CLUSTER_TOL, n_dev=ct[0:1])
    mark("events")
    _, diff = ops.score_closest(inj_sorted, et)
    mark("closest")
    tp, fp, cs = ops.trig_split(ev, diff, th.EVENT_TOL, n_dev=ce[0:1])
    mark("split")
    _, tp_sorted, _ = ops.score_sort(tp, n_dev=cs[0:1])
    _, fp_sorted, _ = ops.score_sort(fp, n_dev=cs[1:2])
    mark("sorts")
    ops.trig_steps(fp_sorted, cs[1:2], tp_sorted, cs[0:1], series.numel() * c["delta_t"], prefactor, Ninj)
    mark("steps")
    torch.cuda.synchronize()
    out = {name: marks[i][1].elapsed_time(e) for i, (name, e) in enumerate(marks[1:])}
    out["enqueue"] = marks[0][1].elapsed_time(marks[-1][1])
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--sizes", type=int, nargs="+", default=[MONTH // 10, MONTH])
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--capacity", type=int, default=None)
    ap.add_argument("--stages", action="store_true")
    args = ap.parse_args()
    import torch
    from gw_whisper_amd import ops
    from gw_whisper_amd import trigger_stats as ts
    assert torch.cuda.is_available(), "time_trigger_stats.py needs an MI355X"
    if args.stages:
        for n in args.sizes:
            c = make(n)
            series = torch.from_numpy(c["series"]).cuda()
            inj, prefactor, Ninj = ts._injections(c["inj"], c["dist"], "time")
            inj_sorted = ts._sorted_on(inj, series.device)
            runs = [staged(torch, ops, series, c, inj_sorted, prefactor, Ninj, args.capacity) for _ in range(args.repeats + 1)][1:]
            print(json.dumps({"samples": n, "repeats": args.repeats,
                              "device_events_ms": {k: statistics.median(r[k] for r in runs) for k in runs[0]}}), flush=True)
        return
    print("| samples | triggers | events | steps | launches (device) | evaluate, call to read | numpy restatement |")
    print("|---|---|---|---|---|---|---|")
    for n in args.sizes:
        c = make(n)
        series = torch.from_numpy(c["series"]).cuda()
        inj, prefactor, Ninj = ts._injections(c["inj"], c["dist"], "time")
        inj_sorted = ts._sorted_on(inj, series.device)

        def chain():
            t, v, ct = ops.trig_triggers(series, c["delta_t"], c["epoch"], 0.1, cap=args.capacity)
            et, ev, ce = ops.trig_events(t, v, th.CLUSTER_TOL, n_dev=ct[0:1])
            return ts._statistics_device(et, ev, ce[0:1], inj_sorted, prefactor, Ninj, n * c["delta_t"], th.EVENT_TOL)

        def whole():
            return ts.evaluate(series, c["delta_t"], c["epoch"], c["inj"], c["dist"], 0.1, th.CLUSTER_TOL, th.EVENT_TOL,
                               capacity=args.capacity)
        dev, wall = [], []
        for r in range(args.repeats + 1):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            chain()
            b.record()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = whole()
            t1 = time.perf_counter()
            if r:
                dev.append(a.elapsed_time(b) * 1e-3)
                wall.append(t1 - t0)
        host = []
        for _ in range(3):
            t0 = time.perf_counter()
            ref = th.restate(c, 0.1)
            host.append(time.perf_counter() - t0)
        flat = {"trig_times": res["triggers"][0], "trig_values": res["triggers"][1], "ev_times": res["events"][0],
                "ev_values": res["events"][1], **res["statistics"]}
        th.compare(flat, ref, f"n = {n}")
        print(f"| {n} | {len(flat['trig_times'])} | {len(flat['ev_times'])} | {len(flat['ranking'])} | {spread(dev)} | {spread(wall)} | "
              f"{spread(host)} |", flush=True)


if __name__ == "__main__":
    main()
