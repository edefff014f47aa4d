"""Pieces shared by tests/test_glitch_host.py and tests/test_gpu_glitch.py: the seeded inputs of the fixture cases (the
same functions as tools/make_golden_glitch.py, which runs the reference's head class on them), the digest the fixture
stores for each gradient tensor, and the head step restated in float64 torch."""
import numpy as np
import torch

from gw_whisper_amd import synth

P_DROP = 0.3
N_SIGNS = 8
WIDTHS = (512, 256, 128)
PARAM_KEYS = ("0.weight", "0.bias", "3.weight", "3.bias", "6.weight", "6.bias", "9.weight", "9.bias")


def case_inputs(d_in, C, B, seed):
    """(x fp32 [B, d_in], labels int64 [B], masks [3] of fp32 [B, width])."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((B, d_in)).astype(np.float32)
    y = rng.integers(0, C, B).astype(np.int64)
    masks = [(rng.random((B, w)) >= P_DROP).astype(np.float32) for w in WIDTHS]
    return x, y, masks


def case_params(ci, d_in, C):
    """The eight head tensors of fixture case ``ci`` (fp32 numpy, nn.Sequential order)."""
    sd = synth.head_state_dict([d_in, 512, 256, 128, C], seed=300 + ci, sequential_stride=3)
    return [sd[k] for k in PARAM_KEYS]


def digest(g, key):
    """[|G|_F, <G, S_0>, ..., <G, S_7>] in fp64, S_j seeded +-1 tensors of G's shape."""
    g = np.asarray(g, np.float64)
    rng = np.random.default_rng(1000 + key)
    out = [np.sqrt((g * g).sum())]
    for _ in range(N_SIGNS):
        s = rng.integers(0, 2, g.shape).astype(np.float64) * 2.0 - 1.0
        out.append((g * s).sum())
    return np.asarray(out, np.float64)


def head64(x, params, y, masks=None, p=P_DROP, upstream=1.0):
    """The glitch head + CrossEntropyLoss in float64 with autograd: Linear -> ReLU -> (mask / (1 - p)) x 3 -> Linear ->
    mean cross entropy, times ``upstream``.  x, params, masks: tensors of any float dtype on one device; y int64.
    Returns (loss, logits, dx, [8 parameter gradients], smallest |hidden pre-activation|)."""
    x = x.detach().double().requires_grad_(True)
    ps = [t.detach().double().requires_grad_(True) for t in params]
    h, margin = x, float("inf")
    for l in range(3):
        pre = h @ ps[2 * l].T + ps[2 * l + 1]
        margin = min(margin, float(pre.detach().abs().min()))
        h = torch.relu(pre)
        if masks is not None:
            h = h * masks[l].double() / (1.0 - p)
    z = h @ ps[6].T + ps[7]
    loss = torch.nn.functional.cross_entropy(z, y)
    (loss * upstream).backward()
    return loss.detach(), z.detach(), x.grad, [t.grad for t in ps], margin
