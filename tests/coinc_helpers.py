"""What the coincidence tests share (tests/test_coinc_host.py, tests/test_gpu_coinc.py, tests/test_gpu_coinc_contract.py):
the seeded case generator -- window stamps, two detectors' score rows with common bumps, their clustered events, the
shifts of the slides --, a brute-force double loop over all pairs, and hand-built lists that break the search's
``2 * window < cluster_threshold`` condition."""

import functools

import numpy as np

STEPS = (204.0 / 2048.0, 0.1)          # exactly representable / not: the second exercises the boundary
CASES = ((40, 70.0), (600, 85.0), (5000, 90.0))      # (windows N, percentile q of the trigger threshold)
CLUSTER_THRESHOLD = 0.35
WINDOW = 0.15


def stamps(N, step, start=1000.0, peak_offset=0.6):
    """float64 window stamps as ``DeviceSegmentSlicer.times_host`` makes them: a running sum from ``start``, then the
    peak offset."""
    steps = np.full((max(N, 1),), step, np.float64)
    steps[0] = start
    return np.add.accumulate(steps)[:N] + peak_offset


def clusters(times, row, thr, cluster_threshold=CLUSTER_THRESHOLD):
    """``inference.get_clusters`` restated for one score row: the windows above ``thr`` in time order, a gap of more than
    ``cluster_threshold`` closes a cluster, a cluster reports the time and value of its FIRST maximum.  Returns (t fp64,
    v fp32)."""
    t, v, cur = [], [], []

    def flush():
        if cur:
            k = int(np.argmax([row[i] for i in cur]))
            t.append(times[cur[k]])
            v.append(row[cur[k]])

    for i in range(len(row)):
        if not row[i] > np.float32(thr):
            continue
        if cur and (times[i] - times[cur[-1]]) > cluster_threshold:
            flush()
            cur = []
        cur.append(i)
    flush()
    return np.asarray(t, np.float64), np.asarray(v, np.float32)


def shifts_for(N, step):
    """[0] + [s * 20 * step], S = min(300, (N - 11) // 20) slides of 20 steps (2 s): the first entry is zero lag."""
    S = min(300, (N - 11) // 20)
    return np.array([0.0] + [(s * 20) * step for s in range(1, S + 1)], np.float64)


@functools.lru_cache(maxsize=None)
def make_case(N, q, step, seed=0):
    """One generator case, computed once and shared (the arrays are read-only): standard-normal fp32 scores [2, N],
    ``max(2, N // 60)`` common bumps of +4 planted at the same window +-1 in both rows, the threshold at the q-th percentile,
    each row's clusters, and the shifts."""
    rng = np.random.default_rng(seed)
    times = stamps(N, step)
    scores = rng.standard_normal((2, N)).astype(np.float32)
    for _ in range(max(2, N // 60)):
        w = int(rng.integers(1, N - 1))
        scores[0, w] += np.float32(4.0)
        scores[1, w + int(rng.integers(-1, 2))] += np.float32(4.0)
    thr = float(np.float32(np.percentile(scores, q)))
    (t0, v0), (t1, v1) = (clusters(times, scores[g], thr) for g in range(2))
    case = dict(N=N, step=step, times=times, scores=scores, thr=thr, t0=t0, v0=v0, t1=t1, v1=v1, shifts=shifts_for(N, step))
    for a in case.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return case


def brute_force(t0, v0, t1, v1, shifts, window):
    """Every (i, j) of every shift under the pair predicate ``fabs((t1[j] + o) - t0[i]) <= window`` and the partner rule
    (largest v1, then smallest fabs(d), then smallest j): a list over the shifts of (idx0, idx1, dt) arrays in ascending i.
    No bisection, no early exit."""
    t0, t1 = np.asarray(t0, np.float64), np.asarray(t1, np.float64)
    v1 = np.asarray(v1, np.float32)
    window = np.float64(window)
    out = []
    for o in np.asarray(shifts, np.float64):
        d = (t1[None, :] + o) - t0[:, None]
        ok = np.fabs(d) <= window
        ii, jj, dd = [], [], []
        for i in np.nonzero(ok.any(axis=1))[0]:
            best = min(np.nonzero(ok[i])[0], key=lambda j: (-float(v1[j]), abs(float(d[i, j])), int(j)))
            ii.append(i); jj.append(best); dd.append(d[i, best])
        out.append((np.asarray(ii, np.int32), np.asarray(jj, np.int32), np.asarray(dd, np.float64)))
    return out


def rule_breaking(n=24, seed=3):
    """Event lists 0.1 s apart -- no clustering could have made them, ``2 * window < cluster_threshold`` fails at every
    window of the tests -- whose detector-1 values hold ties: several candidates per detector-0 event, equal ``v1`` among
    them (values drawn from four levels), equal ``fabs(d)`` too (detector 1 sits half a step off detector 0, so the two
    neighbours of an event are equally far on the exactly representable grid)."""
    rng = np.random.default_rng(seed)
    step = 0.125                                             # exactly representable: equal distances are equal bits
    t0 = 1000.0 + step * np.arange(n, dtype=np.float64)
    t1 = 1000.0 + step * np.arange(n, dtype=np.float64) + step / 2
    v0 = rng.standard_normal(n).astype(np.float32)
    v1 = rng.integers(0, 4, n).astype(np.float32)
    return t0, v0, t1, v1


def check_equal(got, ref):
    """``ops.coinc_slides`` (as numpy) or ``coinc_host`` against a reference dict: every field with ``==``."""
    assert np.array_equal(got["offsets"], ref["offsets"]), (got["offsets"], ref["offsets"])
    for k in ("idx0", "idx1", "time", "stat", "dt"):
        assert got[k].dtype == ref[k].dtype and np.array_equal(got[k], ref[k]), k
