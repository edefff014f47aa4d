"""Pieces shared by tests/test_efficiency_host.py, tests/test_gpu_efficiency.py and tools/make_golden_efficiency.py (which
runs the reference's head class and loss on the same inputs): the seeded inputs of the fixture cases, the digest the
fixture stores for each gradient tensor, and the detection head step restated in float64 torch."""
import numpy as np
import torch

from gw_whisper_amd import synth

EPSILON = 1e-6
N_SIGNS = 8
WIDTHS = (512, 256, 128, 64)
PARAM_KEYS = ("0.weight", "0.bias", "2.weight", "2.bias", "4.weight", "4.bias", "6.weight", "6.bias", "8.weight", "8.bias")
# (d_in, C, B) of the stored head cases
CASES = ((384, 2, 32), (512, 2, 32), (1280, 2, 7), (128, 2, 1), (384, 2, 1000), (384, 3, 33), (256, 64, 17))


def case_inputs(d_in, C, B, seed):
    """(x fp32 [B, d_in], hard targets fp32 [B, C]: one-hot rows)."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((B, d_in)).astype(np.float32)
    y = rng.integers(0, C, B)
    t = np.zeros((B, C), np.float32)
    t[np.arange(B), y] = 1.0
    return x, t


def case_params(ci, d_in, C):
    """The ten head tensors of fixture case ``ci`` (fp32 numpy, nn.Sequential order)."""
    sd = synth.head_state_dict([d_in, 512, 256, 128, 64, C], seed=700 + ci)
    return [sd[k] for k in PARAM_KEYS]


def digest(g, key):
    """[|G|_F, <G, S_0>, ..., <G, S_7>] in fp64, S_j seeded +-1 tensors of G's shape."""
    g = np.asarray(g, np.float64)
    rng = np.random.default_rng(2000 + key)
    out = [np.sqrt((g * g).sum())]
    for _ in range(N_SIGNS):
        s = rng.integers(0, 2, g.shape).astype(np.float64) * 2.0 - 1.0
        out.append((g * s).sum())
    return np.asarray(out, np.float64)


def head64(x, params, targets, epsilon=EPSILON, upstream=1.0):
    """The detection head + Softmax + regularised BCELoss in float64 with autograd: (Linear -> ReLU) x 4 -> Linear ->
    softmax -> q = eps + (1 - C eps) p -> ``binary_cross_entropy`` (mean; logs clamped at -100), times ``upstream``.
    x, params, targets: tensors of any float dtype on one device.  Returns (loss, logits, probs, dx, [10 parameter
    gradients], smallest |hidden pre-activation|)."""
    x = x.detach().double().requires_grad_(True)
    ps = [t.detach().double().requires_grad_(True) for t in params]
    h, margin = x, float("inf")
    for l in range(4):
        pre = h @ ps[2 * l].T + ps[2 * l + 1]
        margin = min(margin, float(pre.detach().abs().min()))
        h = torch.relu(pre)
    z = h @ ps[8].T + ps[9]
    p = torch.softmax(z, dim=1)
    C = z.shape[1]
    q = epsilon + (1.0 - epsilon * C) * p
    loss = torch.nn.functional.binary_cross_entropy(q, targets.detach().double())
    (loss * upstream).backward()
    return loss.detach(), z.detach(), p.detach(), x.grad, [t.grad for t in ps], margin


def with_gap(x, params, row, gap):
    """The ten tensors with w5 changed so that row ``row`` of x gets logits z0 - z1 = ``gap`` (C = 2) and every other row
    keeps its logits: the change is along the part of that row's last hidden activation that is orthogonal to all other
    rows' (fp64 numpy).  Needs B - 1 < 64."""
    xs = np.asarray(x, np.float64)
    ps = [np.asarray(p, np.float64) for p in params]
    h = xs
    for l in range(4):
        h = np.maximum(h @ ps[2 * l].T + ps[2 * l + 1], 0.0)
    z = h @ ps[8].T + ps[9]
    others = np.delete(h, row, axis=0)
    v = h[row].copy()
    if len(others):
        coef, *_ = np.linalg.lstsq(others.T, v, rcond=None)
        v = v - others.T @ coef
    assert np.linalg.norm(v) > 1e-3 * np.linalg.norm(h[row]), "the row's activation lies in the span of the others"
    shift = 0.5 * (gap - (z[row, 0] - z[row, 1])) / float(v @ h[row])
    w5 = ps[8].copy()
    w5[0] += shift * v
    w5[1] -= shift * v
    out = [np.asarray(p, np.float32) for p in params]
    out[8] = w5.astype(np.float32)
    return out


def numpy_statistics(noise_scores, wave_scores, faps):
    """(thresholds [F], table [S, F]) of tools.py:351-368 in numpy on fp32 scores: ascending sort, ``sorted[-rank]`` with
    rank ``int(fap * N)`` (rank 0: ``sorted[0]``), the fraction of each row of ``wave_scores`` [S, n] strictly above."""
    noise_scores = np.asarray(noise_scores, np.float32)
    srt = np.sort(noise_scores)
    ranks = (np.array(faps) * len(noise_scores)).astype(int)
    thr = np.asarray([srt[-r] for r in ranks], np.float32)
    wave_scores = np.asarray(wave_scores, np.float32)
    table = np.stack([(w[:, None] > thr[None, :]).sum(0) / len(w) for w in wave_scores], axis=0)
    return thr, table
