"""Cases of the glitch-scan event builder shared by tests/test_glitch_scan_host.py (``build_events_host`` against the
hand-written expectation) and tests/test_gpu_glitch_scan.py (``ops.glitch_events`` against ``build_events_host``).

Stamps are the slicer's: a running float64 sum ``t_0 = start + peak_offset, t_i = t_(i-1) + step`` with the step of a 0.1 s
scan at 2048 Hz, 204 samples = 0.099609375 s (exact in binary).  An expected event is written by hand as
``(class, first window, windows, last window, peak window)``; its stamps and its peak probability are read at those windows.
"""

import numpy as np

STEP = 204 / 2048.0


def stamps(n, start=0.8):
    s = np.full((max(n, 1),), STEP, np.float64)
    s[0] = start
    return np.add.accumulate(s)[:n]


def _case(name, cls, prob, expect, **kw):
    cls = np.asarray(cls, np.int32)
    return dict(name=name, times=stamps(len(cls)), cls=cls, prob=np.asarray(prob, np.float32), kw=kw, expect=expect)


_T = stamps(8)
_LOW = 0.1            # below every threshold used here
_NEXT = float(np.nextafter(np.float32(0.5), np.float32(1.0)))      # the fp32 value just above 0.5

HAND_CASES = [
    # one class throughout; the two equal peaks keep the first
    _case("one_class", [3] * 6, [0.6, 0.7, 0.9, 0.9, 0.8, 0.6], [(3, 0, 6, 5, 2)]),
    # A B A B ...: same-class triggers lie 2 steps = 0.199 s apart, so each class is ONE event and the two overlap
    _case("alternating", [0, 1] * 5, [0.9] * 10, [(0, 0, 5, 8, 0), (1, 1, 5, 9, 1)]),
    # triggers at windows 0, 3, 7: 3 steps (0.2988 s) join, 4 steps (0.3984 s) split at gap 0.35
    _case("gap_3_joins_4_splits", [2] * 8, [0.9, _LOW, _LOW, 0.8, _LOW, _LOW, _LOW, 0.95], [(2, 0, 2, 3, 0), (2, 7, 1, 7, 7)]),
    # gap == the stamp difference exactly: strict >, so the trigger joins ...
    _case("gap_equal_joins", [2, 2, 2, 2], [0.9, _LOW, _LOW, 0.8], [(2, 0, 2, 3, 0)], gap=float(_T[3] - _T[0])),
    # ... and one ulp less splits
    _case("gap_just_below_splits", [2, 2, 2, 2], [0.9, _LOW, _LOW, 0.8], [(2, 0, 1, 0, 0), (2, 3, 1, 3, 3)],
          gap=float(np.nextafter(_T[3] - _T[0], 0.0))),
    # prob == threshold is no trigger; the next fp32 value is
    _case("prob_equal_threshold", [1, 1, 1], [0.5, _NEXT, 0.5], [(1, 1, 1, 1, 1)], prob_threshold=0.5),
    # a NaN probability is no trigger (and does not end the event around it: only time does)
    _case("nan_prob", [4, 4, 4], [0.9, np.nan, 0.7], [(4, 0, 2, 2, 0)]),
    # ignored classes never trigger; the others do not see them
    _case("ignored", [5, 6, 5, 6, 7], [0.9, 0.9, 0.8, 0.95, 0.9], [(5, 0, 2, 2, 0), (7, 4, 1, 4, 4)], ignore=[6]),
    # classes outside 0..63 are skipped
    _case("class_range", [-1, 64, 63, -5, 0, 1000], [0.9] * 6, [(63, 2, 1, 2, 2), (0, 4, 1, 4, 4)]),
    # a later, strictly larger peak moves the peak; an equal one does not
    _case("peaks", [9] * 5, [0.7, 0.8, 0.8, 0.85, 0.85], [(9, 0, 5, 4, 3)]),
    # nothing triggers
    _case("empty", [1, 2, 3], [_LOW, 0.2, np.nan], []),
]


def expected_events(case):
    """The hand-written expectation of a case as the arrays ``build_events_host`` returns."""
    e, t, p = case["expect"], case["times"], case["prob"]
    col = lambda j: [x[j] for x in e]                                            # noqa: E731
    return {"cls": np.array(col(0), np.int32), "first": np.array(col(1), np.int32), "n": np.array(col(2), np.int32),
            "t_start": t[col(1)].astype(np.float64), "t_end": t[col(3)].astype(np.float64),
            "t_peak": t[col(4)].astype(np.float64), "p_peak": p[col(4)].astype(np.float32)}


def same_bits(a, b):
    """Two event dicts agree in every field: dtype, length, order and bits (NaN-free by construction)."""
    assert set(a) == set(b)
    for k in a:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        assert x.dtype == y.dtype and x.shape == y.shape, f"{k}: {x.dtype}{x.shape} against {y.dtype}{y.shape}"
        assert x.tobytes() == y.tobytes(), f"{k}: {x} against {y}"


def random_case(n, n_classes, seed, p_class0=0.0):
    """Seeded per-window results: classes 0 .. n_classes - 1 (class 0 with probability ``p_class0`` on top of its share),
    probabilities uniform in (0, 1) in fp32, a few NaN and a few classes outside the range."""
    rng = np.random.default_rng(seed)
    cls = rng.integers(0, n_classes, n).astype(np.int32)
    if p_class0 > 0:
        cls[rng.random(n) < p_class0] = 0
    prob = rng.random(n).astype(np.float32)
    if n >= 100:
        prob[rng.integers(0, n, n // 100)] = np.nan
        cls[rng.integers(0, n, n // 200)] = rng.choice(np.array([-1, 64, 99], np.int32), n // 200)
    return stamps(n, start=1.0e9 + 0.8), cls, prob


def spanning_case(n, n_classes, seed):
    """One event of class 0 over the whole series -- every third window triggers, 0.2988 s apart -- and many short events
    of the other classes in between."""
    times, cls, prob = random_case(n, n_classes, seed)
    cls[cls == 0] = 1
    cls[::3] = 0
    prob[::3] = np.float32(0.75)
    prob[(n // 2) // 3 * 3] = np.float32(0.97)               # the peak, far from both ends
    return times, cls, prob
