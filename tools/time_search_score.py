#!/usr/bin/env python3
"""Time the search score (gw_whisper_amd/search_score.py: get_stats) on the device against its numpy restatement on the
same host, at E = 2e5 foreground events, B = 1e5 background events, N = 2e4 injections and at ten times that.

Per size and mode: the host clock around ``get_stats`` to the final read, with numpy inputs (upload included) and with
device-tensor inputs; device events around the enqueue of every stage (the same ops calls ``get_stats`` makes, nothing read
back in between); and the host clock of ``tests/search_score_helpers.restate``.  One warm-up call is excluded everywhere;
the host figures are [median, lowest, highest] of ``--repeat`` runs, the device-event figures medians.  Prints one JSON
line per size and mode; ``--out FILE`` also writes them.

usage: time_search_score.py [--repeat 5] [--scale 1 10] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import search_score_helpers as sh  # noqa: E402

BASE = (200000, 100000, 20000)


def staged(torch, ops, fg, bg, tc, w, duration, n_inj, prefactor):
    """The enqueue of get_stats stage by stage; returns {stage: ms} from device events, 'enqueue' = the whole."""
    marks = [("start", torch.cuda.Event(enable_timing=True))]

    def mark(name):
        ev = torch.cuda.Event(enable_timing=True)
        ev.record()
        marks.append((name, ev))
    marks[0][1].record()
    E, B = fg.shape[1], bg.shape[1]
    order, _, _ = ops.score_sort(fg[0])
    mark("sort event times")
    m = ops.score_match(fg, order, tc)
    mark("match + compact + best")
    c = m["counts"]
    ops.score_far(E, duration, fg.device, n_dev=c[1:2])
    ops.score_far(B, duration, fg.device)
    mark("far")
    f_order, f_sorted, _ = ops.score_sort(m["found_stat"], n_dev=c[2:3])
    mark("sort found statistics")
    _, noise, _ = ops.score_sort(bg[1])
    mark("sort background statistics")
    cs1 = cs2 = None
    if w is not None:
        cs1, cs2 = ops.score_suffix(w[0], w[1], m["found_inj"], f_order, c[2:3])
        mark("chirp suffix sums")
    ops.score_volume(f_sorted, c[2:3], noise, n_inj, prefactor, cs1, cs2)
    mark("volume")
    torch.cuda.synchronize()
    out = {name: marks[i][1].elapsed_time(ev) for i, (name, ev) in enumerate(marks[1:])}
    out["enqueue"] = marks[0][1].elapsed_time(marks[-1][1])
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--scale", type=int, nargs="+", default=[1, 10])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from gw_whisper_amd import ops, search_score as ss
    assert torch.cuda.is_available(), "time_search_score needs a GPU"
    lines = []
    for scale in args.scale:
        E, B, N = (scale * v for v in BASE)
        fg, bg, inj, duration = sh.make_case(E, B, N, 9000 + scale)
        fg_d, bg_d, tc_d = (torch.from_numpy(a).cuda() for a in (fg, bg, inj["tc"]))
        for chirp in (False, True):
            def host(fn):
                fn()                                     # warm-up
                ts = []
                for _ in range(args.repeat):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    fn()
                    ts.append((time.perf_counter() - t0) * 1e3)
                return [statistics.median(ts), min(ts), max(ts)]
            ref = sh.restate(fg, bg, inj, duration, chirp)
            w = None
            if chirp:
                mc = ss.mchirp(inj["mass1"], inj["mass2"])
                w = (torch.from_numpy(mc ** 2.5).cuda(), torch.from_numpy(mc ** 5).cuda())
            staged(torch, ops, fg_d, bg_d, tc_d, w, duration, ref["_Ninj"], ref["_prefactor"])          # warm-up
            runs = [staged(torch, ops, fg_d, bg_d, tc_d, w, duration, ref["_Ninj"], ref["_prefactor"]) for _ in range(args.repeat)]
            line = {"E": E, "B": B, "N": N, "chirp": chirp, "repeat": args.repeat,
                    "get_stats_numpy_inputs_ms": host(lambda: ss.get_stats(fg, bg, inj, duration, chirp)),
                    "get_stats_device_inputs_ms": host(lambda: ss.get_stats(fg_d, bg_d, inj, duration, chirp)),
                    "restatement_numpy_ms": host(lambda: sh.restate(fg, bg, inj, duration, chirp)),
                    "device_events_ms": {k: statistics.median(r[k] for r in runs) for k in runs[0]}}
            print(json.dumps(line), flush=True)
            lines.append(line)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(lines, f, indent=1)


if __name__ == "__main__":
    main()
