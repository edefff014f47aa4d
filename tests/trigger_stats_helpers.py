"""Seeded cases and a vectorised numpy restatement of the efficiency study's test-stage evaluation
(gw_whisper_amd/trigger_stats.py, csrc/trigger_stats.hip): triggers by one comparison, clusters by one difference, the
event of a cluster by a segmented maximum, true / false positives by one search, ranking steps by runs of equal values.
The CPU pin of the algorithm, held to the reference's own functions through tests/golden/efficiency_test.npz by
tests/test_trigger_stats_host.py, and the second opinion for inputs the golden file does not hold."""
import os

import numpy as np

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "efficiency_test.npz")
SEC_PER_MONTH = 30 * 24 * 60 * 60
# (samples, injections, forced run above threshold, seed, epoch): around the sort's 256-element sub-tile and 4096-element
# chunk (the trigger kernels' tile is 4096 samples as well); then one with a GPS-sized epoch; the hand-made case comes last
CASES = ((1, 1, 0, 4101, 0.75), (257, 6, 0, 4102, 0.75), (4097, 40, 0, 4103, 0.75), (12305, 100, 5000, 4104, 0.75),
         (70001, 300, 5000, 4105, 0.75), (1031, 12, 0, 4106, 1238166018.75))
GPS = 5
HAND = len(CASES)
THRESHOLDS = (0.1, 0.5)
REFUSED = ((0, 0.5),)                 # (case, threshold) without a true positive
DELTA_T, CLUSTER_TOL, EVENT_TOL = 0.1, 0.2, 0.3
ARRAYS = ("trig_times", "trig_values", "ev_times", "ev_values", "ranking", "far", "sens-frac", "sens-dist", "sens-vol",
          "sens-vol-err")
EXACT = tuple(k for k in ARRAYS if k != "sens-dist")
# sens-dist: the reference takes (3 vol / (4 pi)) ** (1 / 3) of numpy scalars, the restatement and the package of an array.
# Each pow is good to under 1 ulp, so two of them differ by at most 2 ulp = 2^-51 relatively; the margin doubles that.
DIST_REL = 2.0 ** -50


def make_case(n, n_inj, run, seed, epoch):
    """{"series" fp64 [n], "delta_t", "epoch", "inj" [n_inj] (unsorted), "dist" [n_inj]}: values round(u ** 8, 2), so ties
    of a cluster's maximum and samples exactly on a threshold are frequent; every second injection gets five samples of one
    rounded value in [0.3, 1] around it; ``run`` consecutive samples above 0.1 form one cluster longer than a chunk."""
    rng = np.random.default_rng(seed)
    series = np.round(rng.random(n) ** 8, 2)
    if run:
        a = n // 3
        series[a:a + run] = np.round(0.11 + 0.85 * rng.random(run), 2)
    times = np.arange(n) * DELTA_T + epoch
    at = np.sort(rng.choice(n, n_inj, replace=False))
    inj = times[at] + np.round(rng.uniform(-0.04, 0.04, n_inj), 3)
    for k in range(0, n_inj, 2):
        series[max(at[k] - 2, 0):at[k] + 3] = np.round(rng.uniform(0.3, 1.0), 2)
    perm = rng.permutation(n_inj)
    return {"series": series, "delta_t": DELTA_T, "epoch": epoch, "inj": inj[perm], "dist": rng.uniform(10.0, 500.0, n_inj)[perm]}


def hand_case():
    """48 samples at delta_t = 0.1, epoch 0.  Pairs of triggers two samples apart at offsets where (i + 2) * 0.1 - i * 0.1
    falls below 0.2 (one cluster) and where it reaches it (two clusters); an event at 0.5 with an injection at 0.2, whose
    distance is 0.3 exactly (a true positive); the first event before the first injection and the last one after the last
    injection, and ties among the false positives' values."""
    series = np.zeros(48)
    gaps = np.arange(50) * DELTA_T
    gaps = gaps[2:] - gaps[:-2]
    below, reach = np.flatnonzero(gaps < CLUSTER_TOL), np.flatnonzero(gaps >= CLUSTER_TOL)
    assert len(below) and len(reach), "two-sample gaps lie on one side of the cluster tolerance only"
    b, r = int(below[below >= 10][0]), int(reach[reach >= 20][0])
    series[0] = 0.4                       # an event before the first injection (0.2 away: a true positive)
    series[5] = 0.9                       # t = 0.5: |0.5 - 0.2| == 0.3
    series[[b, b + 2]] = (0.6, 0.7)       # one cluster: the later, larger sample is its event
    series[[r, r + 2]] = (0.6, 0.6)       # two clusters of equal value
    series[[36, 37, 38]] = (0.8, 0.8, 0.3)   # the first of two equal maxima
    series[40] = 0.8                      # a true positive of the injection at 4.0
    series[47] = 0.4                      # an event after the last injection
    assert abs(5 * DELTA_T - 0.2) == EVENT_TOL
    return {"series": series, "delta_t": DELTA_T, "epoch": 0.0, "inj": np.array([4.0, 0.2]), "dist": np.array([120.0, 40.0])}


def case(ci):
    return hand_case() if ci == HAND else make_case(*CASES[ci])


def n_cases():
    return HAND + 1


# ---- the restatement ----------------------------------------------------------------------------------------------------
def triggers(series, delta_t, epoch, threshold):
    series = np.asarray(series).astype(np.float64)      # the reference's assembled series is fp64: compared as such
    idx = np.where(series > threshold)[0]
    return idx * delta_t + float(epoch), series[idx]


def events(times, values, cluster_tolerance):
    times, values = np.asarray(times, np.float64), np.asarray(values, np.float64)
    if len(times) == 0:
        return np.zeros(0), np.zeros(0)
    opens = np.r_[True, times[1:] - times[:-1] >= cluster_tolerance]
    starts = np.flatnonzero(opens)
    cid = np.cumsum(opens) - 1
    peak = np.maximum.reduceat(values, starts)
    at = np.flatnonzero(values == peak[cid])
    first = at[np.unique(cid[at], return_index=True)[1]]      # np.argmax: the first maximum of every cluster
    return times[first], values[first]


def nearest(inj_sorted, t):
    N = len(inj_sorted)
    r = np.searchsorted(inj_sorted, t, side="right")
    return np.minimum(np.abs(t - inj_sorted[np.maximum(r - 1, 0)]), np.abs(t - inj_sorted[np.minimum(r, N - 1)]))


class NoTruePositive(Exception):
    pass


def split(ev_times, ev_values, inj, event_tolerance):
    """(the true positives' values ascending, the false positives' values ascending)"""
    ev_times, ev_values = np.asarray(ev_times, np.float64), np.asarray(ev_values, np.float64)
    d = nearest(np.sort(np.asarray(inj, np.float64)), ev_times) if len(ev_times) else np.zeros(0)
    return np.sort(ev_values[d <= event_tolerance]), np.sort(ev_values[d > event_tolerance])


def statistics(ev_times, ev_values, inj, dist, duration, event_tolerance):
    tp, fp = split(ev_times, ev_values, inj, event_tolerance)
    if len(tp) == 0:
        raise NoTruePositive
    n, Ninj = len(fp), len(dist)
    prefactor = (4. / 3.) * np.pi * np.asarray(dist, np.float64).max() ** 3. / float(Ninj)
    if n == 0:
        return {k: np.zeros(0) for k in ARRAYS[4:]}
    starts = np.flatnonzero(np.r_[True, fp[1:] != fp[:-1]])
    ends = np.r_[starts[1:], n] - 1
    count = n - ends - 1
    if ends[0] == 0:
        count[0] = n                      # the reference's first entry, never overwritten by an equal value
    ranking = fp[starts]
    tidx = np.searchsorted(tp, ranking, side="right")
    s = len(tp) - tidx
    q = s / Ninj
    with np.errstate(invalid="ignore"):
        err = prefactor * (Ninj * (q - q ** 2)) ** 0.5
    vol = prefactor * s
    return {"ranking": ranking, "far": count / duration * SEC_PER_MONTH, "sens-frac": 1 - tidx.astype(np.float64) / len(tp),
            "sens-dist": (3 * vol / (4 * np.pi)) ** (1. / 3.), "sens-vol": vol, "sens-vol-err": err}


def restate(c, threshold, duration=None):
    """Every array of ARRAYS for a case dict; raises NoTruePositive where the reference dies."""
    series = np.asarray(c["series"])
    duration = len(series) * c["delta_t"] if duration is None else duration
    tt, tv = triggers(series, c["delta_t"], c["epoch"], threshold)
    et, ev = events(tt, tv, CLUSTER_TOL)
    ret = {"trig_times": tt, "trig_values": tv, "ev_times": et, "ev_values": ev}
    ret.update(statistics(et, ev, c["inj"], c["dist"], duration, EVENT_TOL))
    return ret


def key(ci, threshold, name):
    return f"c{ci}_t{int(round(threshold * 10)):02d}_{name}"


def compare(got, ref, side):
    """Bit identity on every array; ``sens-dist`` within DIST_REL."""
    for k in EXACT:
        a, b = np.asarray(got[k]), np.asarray(ref[k])
        assert a.dtype == np.float64 and a.shape == b.shape, f"{side}: {k} is {a.dtype} {a.shape}, expected float64 {b.shape}"
        # the same bits; where the reference's own variance came out negative (more true positives than injections) both
        # hold a NaN, whose sign and payload are the square root's business
        same = a.view(np.int64) == b.view(np.int64) if a.size else np.ones(0, bool)
        assert np.all(same | (np.isnan(a) & np.isnan(b))), f"{side}: {k} differs"
    a, b = np.asarray(got["sens-dist"]), np.asarray(ref["sens-dist"])
    assert a.shape == b.shape, f"{side}: sens-dist has shape {a.shape}, expected {b.shape}"
    assert np.all(np.abs(a - b) <= DIST_REL * np.abs(b)), f"{side}: sens-dist off by more than 2^-50"
