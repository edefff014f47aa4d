"""numpy restatement of the device ROC / bootstrap algorithm of csrc/roc.hip (one sort, a resample = multiplicities over
the sorted order, cumulative counts, np.interp's search and expression): the CPU pin of the algorithm, held to the
reference's own ``bootstrap_roc_curve`` by tests/test_roc_host.py, and the second opinion for shapes
tests/golden/roc_bootstrap.npz does not hold."""
import os
from fractions import Fraction

import numpy as np

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "roc_bootstrap.npz")
CASES = ((64, 50), (257, 50), (4096, 40), (20000, 12))      # (N, R) of the golden cases
GRID = np.logspace(-4, 0, num=500)


def saturating_scores(n, sep, seed):
    """labels Bernoulli(1/2); scores = the fp32 sigmoid of N(+-sep, 3^2) logits, exactly 0 / 1 where |logit| > 6: heavy
    ties at both ends, as fp32 sigmoids have."""
    rng = np.random.default_rng(seed)
    labels = (rng.random(n) < 0.5).astype(np.float32)
    z = (rng.standard_normal(n) * 3.0 + np.where(labels > 0.5, sep, -sep)).astype(np.float32)
    s = (1.0 / (1.0 + np.exp(-z.astype(np.float64)))).astype(np.float32)
    s[z > 6] = 1.0
    s[z < -6] = 0.0
    return s, labels


def draw_indices(seed, R, n):
    """The reference's resamples: ``np.random.seed(seed)`` and one ``randint(0, n, size=n)`` per replicate."""
    rs = np.random.RandomState(seed)
    return np.stack([rs.randint(0, n, size=n) for _ in range(R)]).astype(np.int64)


def checksums(idx):
    flat = np.asarray(idx, np.int64).ravel()
    return int(np.bitwise_xor.reduce(flat)), int(flat.sum())


def sort_desc(scores, labels):
    """order (stable, descending; -0.0 == +0.0), rank, pos, gend."""
    s = np.asarray(scores, np.float32) + np.float32(0.0)          # -0.0 + 0.0 = +0.0
    order = np.argsort(-s.astype(np.float64), kind="stable")
    rank = np.empty(len(s), np.int64)
    rank[order] = np.arange(len(s))
    ss = s[order]
    gend = np.flatnonzero(np.r_[ss[1:] != ss[:-1], True])
    pos = (np.asarray(labels)[order] > 0.5).astype(np.int64)
    return order, rank, pos, gend


def curve(pos, gend):
    """fps, tps (int64, leading (0, 0)), fpr, tpr (one division each), P, Nneg, the AUC as an exact fraction."""
    cum = np.cumsum(pos)
    tps = np.r_[0, cum[gend]].astype(np.int64)
    fps = np.r_[0, gend + 1 - cum[gend]].astype(np.int64)
    P, Nneg = int(tps[-1]), int(fps[-1])
    with np.errstate(divide="ignore", invalid="ignore"):
        fpr, tpr = fps / np.float64(Nneg), tps / np.float64(P)
    acc = sum(int(a) * int(b) for a, b in zip(np.diff(fps), tps[1:] + tps[:-1]))
    auc = Fraction(acc, 2 * P * Nneg) if P and Nneg else None
    return fps, tps, fpr, tpr, P, Nneg, auc


def bootstrap_rows(rank, pos, gend, idx, grid=GRID):
    """tpr [R, Q] and valid [R]: per replicate the multiplicities of the sorted positions, the cumulative (tps, fps) at
    the run ends behind a leading (0, 0), the rightmost vertex j with fpr_j <= x, and np.interp's expression."""
    n, G = len(rank), len(gend)
    grid = np.asarray(grid, np.float64)
    rows = np.full((len(idx), len(grid)), np.nan)
    valid = np.zeros(len(idx), np.uint8)
    for r, draws in enumerate(np.asarray(idx)):
        mult = np.bincount(rank[draws], minlength=n)
        ctp, cfp = np.cumsum(mult * pos), np.cumsum(mult * (1 - pos))
        Pr, Nr = int(ctp[-1]), int(cfp[-1])
        if Pr == 0 or Nr == 0:
            continue
        valid[r] = 1
        tv = np.r_[0, ctp[gend]].astype(np.float64) / np.float64(Pr)
        fv = np.r_[0, cfp[gend]].astype(np.float64) / np.float64(Nr)
        j = np.searchsorted(fv, grid, side="right") - 1
        jn = np.minimum(j + 1, G)
        with np.errstate(divide="ignore", invalid="ignore"):
            slope = (tv[jn] - tv[j]) / (fv[jn] - fv[j])
            rows[r] = np.where(j == G, tv[G], slope * (grid - fv[j]) + tv[j])
    return rows, valid


def band(rows, valid):
    v = rows[np.asarray(valid) != 0]
    return np.mean(v, axis=0), np.std(v, axis=0)
