"""Seeded cases and a vectorised numpy restatement of the search score of csrc/score.hip (one stable sort of the event
times, the closest injection by one search, compaction by masks, the best statistic per injection over contiguous runs,
counting by searches): the CPU pin of the algorithm, held to the reference's own ``get_stats`` by
tests/test_search_score_host.py, and the second opinion for shapes tests/golden/search_score.npz does not hold."""
import os

import numpy as np

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "search_score.npz")
# (E foreground events, B background events, N injections, seed) around the sort's 256-element sub-tile and 4096-element
# chunk; the hand-made case comes last
CASES = ((1, 1, 1, 3101), (257, 255, 40, 3102), (4097, 4095, 300, 3103), (12305, 8193, 1000, 3104))
HAND = len(CASES)
MODES = ("plain", "chirp")
# the gathers of the inputs by stored indices the golden file leaves out for the largest case (the 1 MB limit)
BIG_KEYS = ("fg-events", "true-positives", "false-positives")
GPS0 = 1238166018
INT_KEYS = ("found-indices", "missed-indices", "true-positive-event-indices", "false-positive-event-indices", "sorting-indices")
EXACT_KEYS = INT_KEYS + ("fg-events", "true-positive-diffs", "false-positive-diffs", "true-positives", "false-positives",
                         "fg-far", "far")
VOLUME_KEYS = ("sensitive-volume", "sensitive-distance", "sensitive-volume-error", "sensitive-fraction")
U = 2.0 ** -53


def _stats(rng, n, loc):
    """float32 values rounded to one decimal: ties among statistics are frequent"""
    return np.round(rng.normal(loc, 2.5, n), 1).astype(np.float32).astype(np.float64)


def make_case(E, B, N, seed):
    """(fgevents [3, E], bgevents [3, B], injparams, duration): GPS-sized times, about half the foreground events within
    +-0.2 s of an injection (var is 0.2 or 0.1: not all of those are true positives), the first one always a true
    positive, event times pairwise distinct."""
    rng = np.random.default_rng(seed)
    tc = GPS0 + np.cumsum(rng.uniform(24, 30, N))
    lo, hi = tc[0] - 50.0, tc[-1] + 50.0
    near = rng.random(E) < 0.5
    near[0] = True
    t = np.where(near, tc[rng.integers(0, N, E)] + rng.uniform(-0.2, 0.2, E), rng.uniform(lo, hi, E))
    t[0] = tc[N // 2] + 0.05
    while True:                                 # distinct times: the reference's unstable argsort has one answer
        first = np.unique(t, return_index=True)[1]
        if first.size == E:
            break
        dup = np.ones(E, bool)
        dup[first] = False                      # GPS-sized doubles are 2.4e-7 s apart: move the later ones of equal times
        t[dup] += rng.uniform(1e-6, 1e-3, int(dup.sum()))
    var = np.where(rng.random(E) < 0.8, 0.2, 0.1)
    var[0] = 0.2
    fg = np.stack([t, _stats(rng, E, 6.0), var])
    bg = np.stack([rng.uniform(lo, hi, B), _stats(rng, B, 4.0), np.full(B, 0.2)])
    inj = {"tc": tc, "distance": rng.uniform(500, 7000, N), "mass1": rng.uniform(10, 50, N), "mass2": rng.uniform(10, 50, N)}
    return fg, bg, inj, float(hi - lo)


def hand_case():
    """Five events against tc = [100, 130, 160], given out of order.  In time order: one before the first injection; one
    whose |dt| = 0.25 equals its var exactly (a true positive); one on the exact midpoint 115 (goes right: a false
    positive on injection 1's run); a true positive of injection 1; one after the last injection.  The reference gives
    found-indices [0 0 1 1 2] and true positives [1 3].  The background holds ties with the found statistics."""
    tc = np.array([100.0, 130.0, 160.0])
    ev = np.array([[90.0, 3.0, 0.2], [100.25, 5.0, 0.25], [115.0, 9.0, 0.2], [130.125, 7.5, 0.2], [170.0, 8.0, 0.2]]).T
    fg = np.ascontiguousarray(ev[:, [3, 0, 4, 1, 2]])
    bg = np.array([[10.0, 20.0, 30.0, 40.0, 50.0], [7.5, 4.0, 5.0, 9.0, 5.0], [0.2] * 5])
    inj = {"tc": tc, "distance": np.array([1000.0, 2500.0, 4000.0]), "mass1": np.array([10.0, 30.0, 50.0]),
           "mass2": np.array([12.0, 25.0, 40.0])}
    return fg, bg, inj, 60.0


def case(ci):
    return hand_case() if ci == HAND else make_case(*CASES[ci])


def closest(tc, t):
    """(index, |dt|) of the closest injection; an exact midpoint goes to the right neighbour"""
    N = len(tc)
    r = np.searchsorted(tc, t, side="right")
    l, rc = np.maximum(r - 1, 0), np.minimum(r, N - 1)
    dl, dr = np.abs(tc[l] - t), np.abs(tc[rc] - t)
    left = (r == N) | (dl < dr)
    return np.where(left, l, r).astype(np.int64), np.where(left, dl, dr)


def restate(fgevents, bgevents, injparams, duration=None, chirp_distance=False):
    """The sixteen keys of ``get_stats`` plus ``_F`` (the number of found injections), ``_S1`` / ``_S2`` (chirp mode: the
    weighted sums at every background statistic) and ``_Ninj`` / ``_prefactor``."""
    fg, bg = np.asarray(fgevents, np.float64), np.asarray(bgevents, np.float64)
    tc, dist = np.asarray(injparams["tc"], np.float64), np.asarray(injparams["distance"], np.float64)
    N, E, B = len(tc), fg.shape[1], bg.shape[1]
    if duration is None:
        duration = tc.max() - tc.min()
    order = np.argsort(fg[0], kind="stable")
    ev = fg[:, order]
    idx, diff = closest(tc, ev[0])
    tp = diff <= ev[2]
    tpi, fpi = np.flatnonzero(tp), np.flatnonzero(~tp)
    # idx is non-decreasing: injection i owns the run [L[i], R[i]) of the sorted events
    assert np.all(np.diff(idx) >= 0)
    inj_ids = np.arange(N)
    L, R = np.searchsorted(idx, inj_ids, side="left"), np.searchsorted(idx, inj_ids, side="right")
    best = np.full(N, -np.inf)
    np.maximum.at(best, idx[tpi], ev[1][tpi])
    has = np.zeros(N, bool)
    has[idx[tpi]] = True
    found = np.flatnonzero(has)
    so = np.argsort(best[found], kind="stable")
    fstat, finj = best[found][so], found[so]
    F = len(found)
    noise = np.sort(bg[1], kind="stable")
    ret = {"fg-events": ev, "found-indices": idx, "missed-indices": np.flatnonzero(L == R), "true-positive-event-indices": tpi,
           "false-positive-event-indices": fpi, "sorting-indices": order, "true-positive-diffs": diff[tpi],
           "false-positive-diffs": diff[fpi], "true-positives": ev[:, tpi], "false-positives": ev[:, fpi],
           "fg-far": (len(fpi) - np.arange(len(fpi)) - 1) / duration, "far": (B - np.arange(B) - 1) / duration}
    fidx = np.searchsorted(fstat, noise, side="right")
    nfound = F - fidx
    vtot = (4. / 3.) * np.pi * dist.max()**3.
    if chirp_distance:
        m1, m2 = np.asarray(injparams["mass1"], np.float64), np.asarray(injparams["mass2"], np.float64)
        mc = (m1 * m2) ** (3. / 5.) / (m1 + m2) ** (1. / 5.)
        Ninj = np.sum((mc.max() / mc) ** (5. / 2.))
        prefactor = vtot / (mc.max() ** (5. / 2.) * N)
        cs1 = np.concatenate([np.cumsum((mc[finj] ** (5. / 2.))[::-1])[::-1], np.zeros(1)])
        cs2 = np.concatenate([np.cumsum((mc[finj] ** 5)[::-1])[::-1], np.zeros(1)])
        S1, S2 = cs1[fidx], cs2[fidx]
        sv = S2 / Ninj - (S1 / Ninj) ** 2
        ret["_S1"], ret["_S2"] = S1, S2
    else:
        Ninj, prefactor = N, vtot / N
        S1 = nfound
        sv = nfound / Ninj - (nfound / Ninj) ** 2
    vol = prefactor * S1
    ret.update({"sensitive-volume": vol, "sensitive-distance": (3 * vol / (4 * np.pi))**(1. / 3.),
                "sensitive-volume-error": prefactor * (Ninj * sv) ** 0.5, "sensitive-fraction": nfound / Ninj,
                "_F": F, "_Ninj": float(Ninj), "_prefactor": float(prefactor)})
    return ret


def compare(got, ref, chirp, side, keys=None):
    """``got`` (sixteen keys) against ``ref`` (a restatement's dict, which also carries _F, _S1, _S2, _Ninj, _prefactor).
    Integers and everything made of +, -, x, /, sqrt in the reference's order: bit-identical.  Chirp mode: S1 and S2 are
    sums of F positive terms taken in another order, each sum within (F - 1) u of the exact one, so two of them differ by at
    most 2 F u relatively, u = 2^-53.  The volume adds one rounding, the distance is its cube root (a third of the
    relative error); the volume error is compared through the implied sample variance, whose subtraction cancels:
    absolute 4 F u (S2 / Ninj + (S1 / Ninj)^2).  (F <= 2: a sum of two terms commutes, the bits are equal.)"""
    for k in (keys or EXACT_KEYS):
        if k not in EXACT_KEYS:
            continue
        a, b = np.asarray(got[k]), np.asarray(ref[k])
        assert a.shape == b.shape, f"{side}: {k} has shape {a.shape}, expected {b.shape}"
        assert np.array_equal(a, b), f"{side}: {k} differs"
    for k in INT_KEYS:
        assert np.asarray(got[k]).dtype == np.int64, f"{side}: {k} is {np.asarray(got[k]).dtype}"
    assert np.array_equal(got["sensitive-fraction"], ref["sensitive-fraction"]), f"{side}: sensitive-fraction differs"
    if not chirp:
        for k in VOLUME_KEYS:
            assert np.array_equal(got[k], ref[k]), f"{side}: {k} differs"
        return
    F, Ninj, pre = ref["_F"], ref["_Ninj"], ref["_prefactor"]
    rel = 2 * F * U
    vol, rvol = np.asarray(got["sensitive-volume"]), np.asarray(ref["sensitive-volume"])
    assert vol.shape == rvol.shape
    assert np.all(np.abs(vol - rvol) <= (rel + U) * np.abs(rvol)), f"{side}: sensitive-volume off by more than {rel + U:.3g}"
    d, rd = np.asarray(got["sensitive-distance"]), np.asarray(ref["sensitive-distance"])
    assert np.all(np.abs(d - rd) <= (rel + U) / 3 * np.abs(rd)), f"{side}: sensitive-distance off"
    sv = (np.asarray(got["sensitive-volume-error"]) / pre) ** 2 / Ninj
    rsv = (np.asarray(ref["sensitive-volume-error"]) / pre) ** 2 / Ninj
    tol = 4 * F * U * (ref["_S2"] / Ninj + (ref["_S1"] / Ninj) ** 2)
    # where the reference's own subtraction came out negative its error is NaN (one found injection of N = 1: S2 / Ninj
    # against (S1 / Ninj)^2 of the same term): there the variance is zero to within the bound, or NaN as well
    nan = np.isnan(rsv)
    assert np.all(np.abs(sv - rsv)[~nan] <= tol[~nan]), \
        f"{side}: the implied sample variance is off by {np.max((np.abs(sv - rsv) - tol)[~nan]):.3g} more than the bound"
    assert np.all(np.isnan(sv[nan]) | (np.abs(sv[nan]) <= tol[nan])), f"{side}: a variance where the reference has NaN"
