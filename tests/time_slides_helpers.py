"""What the time-slide tests share (tests/test_time_slides_host.py, tests/test_gpu_time_slides.py,
tests/test_gpu_time_slides_contract.py): seeded cases, the gathered rows of a slide, the fp64 oracle of the search head on
them, the offsets that exercise the circular wrap, and score rows for the clustering."""

import numpy as np
import torch

SHAPES = ((37, 2, 384, 2), (5, 2, 128, 1), (64, 3, 128, 2), (33, 2, 768, 2))     # (N, D, d, C)
TILE = 16                                                                       # rows of one workgroup (head_chain.h)


def make_head(D, d, C, seed, softmax=True):
    """The search head of ``GWWhisperClassifier`` with torch's default initialisation, seeded."""
    import torch.nn as nn
    torch.manual_seed(seed)
    mods = [nn.Linear(D * d, 512), nn.ReLU(), nn.Linear(512, 256), nn.ReLU(), nn.Linear(256, 128), nn.ReLU(),
            nn.Linear(128, 64), nn.ReLU(), nn.Linear(64, C)]
    if softmax:
        mods.append(nn.Softmax(dim=1))
    return nn.Sequential(*mods).eval()


def make_case(N, D, d, C, seed):
    """(tokens fp32 [N, D, d] ~ N(0, 1) as numpy, the head on the CPU)."""
    rng = np.random.default_rng(seed)
    return rng.standard_normal((N, D, d)).astype(np.float32), make_head(D, d, C, seed)


def gathered(tokens, o):
    """[N, D * d]: row i = cat_g tokens[(i + g o) mod N, g] -- what slide offset o feeds the head."""
    N, D, _ = tokens.shape
    i = np.arange(N)
    return np.concatenate([tokens[(i + g * o) % N, g] for g in range(D)], axis=1)


def head_weights(head):
    """[(W fp64 [out, in], b fp64 [out])] of the five Linear layers."""
    return [(m.weight.detach().cpu().numpy().astype(np.float64), m.bias.detach().cpu().numpy().astype(np.float64))
            for m in head if isinstance(m, torch.nn.Linear)]


def oracle(rows, weights, softmax):
    """The head in fp64 on fp32 rows [n, D * d]: z[0], or softmax(z)[0]."""
    h = np.asarray(rows, np.float64)
    for li, (w, b) in enumerate(weights):
        h = h @ w.T + b
        if li < len(weights) - 1:
            h = np.maximum(h, 0.0)
    if not softmax:
        return h[:, 0]
    e = np.exp(h - h.max(axis=1, keepdims=True))
    return e[:, 0] / e.sum(axis=1)


def oracle_pair_loop(tokens, weights, o, softmax):
    """The same, pair by pair and layer by layer in python: the restatement the vectorised oracle is checked against."""
    N, D, _ = tokens.shape
    out = np.zeros((N,))
    for i in range(N):
        x = np.concatenate([tokens[(i + g * o) % N, g].astype(np.float64) for g in range(D)])
        for li, (w, b) in enumerate(weights):
            x = np.array([np.dot(w[n], x) + b[n] for n in range(w.shape[0])])
            if li < len(weights) - 1:
                x = np.where(x > 0, x, 0.0)
        if softmax:
            e = np.exp(x - x.max())
            out[i] = e[0] / e.sum()
        else:
            out[i] = x[0]
    return out


def offsets_for(N):
    """{0, 1, N - 1}, one offset whose wrap (detector 1 passes window N - 1 at i = N - o) falls inside a 16-row tile and,
    where N allows, one that puts it on a tile edge."""
    offs = {0, 1 % N, N - 1}
    inside = [o for o in range(1, N) if (N - o) % TILE not in (0,) and N - o > 1]
    if inside:
        offs.add(max(inside, key=lambda o: ((N - o) % TILE == 5, o)))      # i = N - o = 5 (mod 16) when it exists
    edge = [o for o in range(1, N) if (N - o) % TILE == 0]
    if edge:
        offs.add(edge[-1])
    return sorted(offs)


def stamps(N, start=1.0e9, step=204.0 / 2048.0, peak_offset=0.6):
    """float64 window stamps as ``DeviceSegmentSlicer.times_host`` makes them: a running sum."""
    steps = np.full((max(N, 1),), step, np.float64)
    steps[0] = start
    return np.add.accumulate(steps)[:N] + peak_offset


def score_rows(S, N, seed):
    """(scores fp32 [S, N], threshold): seeded N(0, 1), the threshold at the 80th percentile; with S = 5 rows 1..4 are
    crafted: no trigger, every window a trigger, equal maxima inside one cluster, a lone trigger in the last window."""
    rng = np.random.default_rng(seed)
    sc = rng.standard_normal((S, N)).astype(np.float32)
    thr = float(np.float32(np.percentile(sc, 80.0)))        # an fp32 value: host and device compare against the same number
    if S >= 5:
        sc[1] = thr - 1.0 - np.abs(sc[1])
        sc[2] = thr + 0.5 + np.abs(sc[2])
        sc[3] = thr - 1.0
        sc[3, : min(N, 3)] = thr + 2.0                     # neighbouring windows, equal values: the FIRST is reported
        sc[4] = thr - 1.0
        sc[4, N - 1] = thr + 3.0
    return sc, thr


def host_clusters(times, row, thr, cluster_threshold):
    """``inference.get_clusters`` on the triggers of one row, as ``evaluate_slices`` lists them."""
    from gw_whisper_amd import inference as inf
    trig = [[float(times[i]), float(row[i])] for i in range(len(row)) if row[i] > np.float32(thr)]
    t, v, var = inf.get_clusters({"k": trig}, cluster_threshold)
    return np.asarray(t, np.float64), np.asarray(v, np.float64), var
