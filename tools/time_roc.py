#!/usr/bin/env python3
"""Timing of the signal-vs-noise ROC evaluation on an MI355X (profiles/roc_bootstrap.md).

    time_roc.py sort       the device sort + curve + AUC (``ops.roc_sort`` + ``ops.roc_curve``) against
                           ``sklearn.metrics.roc_curve(drop_intermediate=False)`` + ``roc_auc_score`` on one host thread
    time_roc.py bootstrap  the whole band, ``roc.RocEvaluator`` (host index stream, upload, sort, ``--resamples`` replicates,
                           band, download), and the bootstrap kernel alone on resident indices, against the host loop the
                           reference runs: per replicate ``resample`` + ``roc_curve`` + ``np.interp``, then mean / std
    time_roc.py band       ``ops.roc_band`` on resident [R, 500] rows against ``np.mean`` / ``np.std``

at every ``--n`` (default 20000 and 2^17).  Every figure is the median of ``--repeats`` timed runs after a warm-up, with the
lowest and highest beside it; every timed device region ends in a synchronisation.  The host loop is timed once on
``--host-resamples`` replicates and scaled to ``--resamples``: it is linear in them.  One JSON line per measurement on
stdout; ``--md FILE`` appends the same figures as table rows."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

GRID = np.logspace(-4, 0, num=500)


def spread(xs):
    xs = sorted(xs)
    return {"median": xs[len(xs) // 2], "min": xs[0], "max": xs[-1]}


def timed(fn, repeats, warmup=1, sync=True):
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(repeats):
        if sync:
            torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        if sync:
            torch.cuda.synchronize()
        out.append(time.perf_counter() - t0)
    return out


def inputs(n, seed=0):
    """Bernoulli(1/2) labels, fp32 sigmoids of N(+-2, 3^2) logits: saturated ties at both ends."""
    rng = np.random.default_rng(seed)
    labels = (rng.random(n) < 0.5).astype(np.float32)
    z = (rng.standard_normal(n) * 3.0 + np.where(labels > 0.5, 2.0, -2.0)).astype(np.float32)
    return torch.sigmoid(torch.from_numpy(z)).numpy(), labels


def host_band(scores, labels, resamples, seed):
    from sklearn.metrics import roc_curve
    rs = np.random.RandomState(seed)
    rows = []
    for _ in range(resamples):
        pick = rs.randint(0, len(scores), size=len(scores))
        fpr, tpr, _ = roc_curve(labels[pick], scores[pick])
        rows.append(np.interp(GRID, fpr, tpr))
    return np.mean(rows, axis=0), np.std(rows, axis=0)


def emit(args, rec):
    print(json.dumps(rec), flush=True)
    if args.md:
        with open(args.md, "a") as f:
            f.write("| " + " | ".join(f"{v:.4g}" if isinstance(v, float) else str(v) for v in rec.values()) + " |\n")


def cmd_sort(args):
    from sklearn.metrics import roc_auc_score, roc_curve
    from gw_whisper_amd import ops
    for n in args.n:
        scores, labels = inputs(n)
        s, l = torch.from_numpy(scores).cuda(), torch.from_numpy(labels).cuda()

        def dev():
            _, _, pos, gend, G, _ = ops.roc_sort(s, l)
            ops.roc_curve(pos, gend, G)[5].item()
        ts = [t * 1e3 for t in timed(dev, args.repeats)]
        emit(args, {"what": "sort_curve_auc_device_ms", "N": n, **spread(ts)})

        def host():
            roc_curve(labels, scores, drop_intermediate=False)
            roc_auc_score(labels, scores)
        ts = [t * 1e3 for t in timed(host, args.repeats, sync=False)]
        emit(args, {"what": "roc_curve_auc_sklearn_ms", "N": n, **spread(ts)})


def cmd_bootstrap(args):
    from gw_whisper_amd import ops, roc
    R = args.resamples
    for n in args.n:
        scores, labels = inputs(n)
        s, l = torch.from_numpy(scores).cuda(), torch.from_numpy(labels).cuda()
        ev = roc.RocEvaluator(num_bootstrap=R, seed=1)
        out = {}

        def whole():
            out.update(ev(s, l))
        ts = timed(whole, args.repeats)
        emit(args, {"what": "band_device_whole_s", "N": n, "R": R, "chunk": ev.chunk_rows(n), **spread(ts)})
        _, rank, pos, gend, G, _ = ops.roc_sort(s, l)
        rc = min(ev.chunk_rows(n), R)
        idx = torch.from_numpy(np.random.RandomState(1).randint(0, n, size=(rc, n)).astype(np.int32)).cuda()
        grid = torch.from_numpy(GRID).cuda()
        ws = torch.empty((rc * n * 8,), dtype=torch.uint8, device="cuda")
        ts = [t * 1e3 for t in timed(lambda: ops.roc_bootstrap_tpr(rank, pos, gend, G, idx, grid, ws=ws), args.repeats)]
        emit(args, {"what": "bootstrap_kernel_ms", "N": n, "R": rc, **spread(ts), "replicates_per_s": rc / spread(ts)["median"] * 1e3})
        hr = min(args.host_resamples, R)
        host_band(scores, labels, 2, 0)          # warm-up: the first call pays sklearn's import
        t0 = time.perf_counter()
        mean, std = host_band(scores, labels, hr, 1)
        t_host = (time.perf_counter() - t0) * R / hr
        emit(args, {"what": "band_host_loop_s", "N": n, "R": R, "timed_resamples": hr, "median": t_host})
        if hr == R:
            emit(args, {"what": "band_device_vs_host_max_abs_diff", "N": n, "mean": float(np.abs(out["mean_tpr"] - mean).max()),
                        "std": float(np.abs(out["std_tpr"] - std).max())})


def cmd_band(args):
    from gw_whisper_amd import ops
    R = args.resamples
    rows = np.random.default_rng(0).random((R, 500))
    t, v = torch.from_numpy(rows).cuda(), torch.ones(R, dtype=torch.uint8, device="cuda")
    ts = [x * 1e3 for x in timed(lambda: ops.roc_band(t, v), args.repeats)]
    emit(args, {"what": "band_kernel_ms", "R": R, **spread(ts)})
    ts = [x * 1e3 for x in timed(lambda: (np.mean(rows, axis=0), np.std(rows, axis=0)), args.repeats, sync=False)]
    emit(args, {"what": "band_numpy_ms", "R": R, **spread(ts)})


if __name__ == "__main__":
    p = argparse.ArgumentParser()
    p.add_argument("what", choices=("sort", "bootstrap", "band"))
    p.add_argument("--n", type=int, nargs="+", default=[20000, 1 << 17])
    p.add_argument("--resamples", type=int, default=1000)
    p.add_argument("--host-resamples", type=int, default=50)
    p.add_argument("--repeats", type=int, default=5)
    p.add_argument("--md", type=str, default=None)
    a = p.parse_args()
    assert torch.cuda.is_available(), "time_roc.py needs an MI355X"
    {"sort": cmd_sort, "bootstrap": cmd_bootstrap, "band": cmd_band}[a.what](a)
