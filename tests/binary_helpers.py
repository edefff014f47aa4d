"""Pieces shared by tests/test_binary_host.py, tests/test_gpu_binary_head.py, tests/test_gpu_binary_contract.py,
tests/test_gpu_sd_train.py and tools/make_golden_binary.py (which runs the reference's classifier classes on the same
inputs): the seeded inputs of the fixture cases and the binary head step restated in float64 torch."""
import numpy as np
import torch

from gw_whisper_amd import synth

ONE, TWO = 1, 2                     # ops.BIN_HEAD_ONE / BIN_HEAD_TWO
WIDTHS = {ONE: (512, 256, 128, 64), TWO: (1024, 512, 256)}
# (layout, d_in, C, B) of the stored cases: B below, at and across the 16-row tile, C = 1 in a 16-column tile, and for the
# two-detector layout both sides of the d_in at which x no longer fits LDS next to the 1024-wide row (1280 | 1536)
CASES = ((ONE, 128, 1, 1), (ONE, 384, 1, 17), (ONE, 1280, 1, 33), (ONE, 384, 3, 16),
         (TWO, 256, 1, 1), (TWO, 768, 1, 17), (TWO, 1024, 1, 32), (TWO, 1536, 1, 7), (TWO, 2560, 1, 33), (TWO, 768, 2, 5))
MARGIN = 2e-6                       # every hidden pre-activation of a stored case is at least this far from zero


def param_keys(layout):
    return tuple(f"{2 * i}.{n}" for i in range(len(WIDTHS[layout]) + 1) for n in ("weight", "bias"))


def case_inputs(d_in, C, B, seed):
    """(x fp32 [B, d_in], hard targets fp32 [B, C] of zeros and ones)."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((B, d_in)).astype(np.float32)
    t = rng.integers(0, 2, (B, C)).astype(np.float32)
    return x, t


def case_params(ci, layout, d_in, C):
    """The head tensors of fixture case ``ci`` (fp32 numpy, nn.Sequential order)."""
    sd = synth.head_state_dict([d_in, *WIDTHS[layout], C], seed=900 + ci)
    return [sd[k] for k in param_keys(layout)]


def head64(x, params, targets, upstream=1.0):
    """(Linear -> ReLU) x (L - 1) -> Linear -> ``binary_cross_entropy_with_logits`` (mean) in float64 with autograd, times
    ``upstream``.  x, params, targets: tensors of any float dtype on one device.  Returns (loss, logits, probs, row_loss,
    dx, [parameter gradients], smallest |hidden pre-activation|)."""
    x = x.detach().double().requires_grad_(True)
    ps = [t.detach().double().requires_grad_(True) for t in params]
    L = len(ps) // 2
    h, margin = x, float("inf")
    for l in range(L - 1):
        pre = h @ ps[2 * l].T + ps[2 * l + 1]
        margin = min(margin, float(pre.detach().abs().min()))
        h = torch.relu(pre)
    z = h @ ps[-2].T + ps[-1]
    t = targets.detach().double()
    loss = torch.nn.functional.binary_cross_entropy_with_logits(z, t)
    (loss * upstream).backward()
    rows = torch.nn.functional.binary_cross_entropy_with_logits(z.detach(), t, reduction="none").sum(1)
    return loss.detach(), z.detach(), torch.sigmoid(z.detach()), rows, x.grad, [p.grad for p in ps], margin


def _logits_np(x, params, bias=True):
    ps = [np.asarray(p, np.float64) for p in params]
    h = np.asarray(x, np.float64)
    for l in range(len(ps) // 2 - 1):
        h = np.maximum(h @ ps[2 * l].T + (ps[2 * l + 1] if bias else 0.0), 0.0)
    return h @ ps[-2].T + (ps[-1] if bias else 0.0)


def with_extreme_rows(x, params, value):
    """(x', row_hi, row_lo): x with two of its rows scaled by positive factors so that the head (C = 1) gives row_hi the
    logit +``value`` and row_lo the logit -``value`` (fp64 numpy, to the fp32 rounding of x'); every other row and every
    weight is untouched.  The chain without its biases is positively homogeneous, so a row's logit grows linearly with its
    scale in the direction of its bias-free logit: the rows are those with the largest and the smallest bias-free logit,
    the factors come from a bisection.  Scaling an input row keeps every dot product of the chain as well conditioned as it
    was: efficiency_helpers.with_gap reaches its gap through the last weight along a direction orthogonal to all other
    rows, which at these heads' correlated post-ReLU activations makes every row's logit a difference of large terms."""
    x = np.array(x, np.float32)
    zh = _logits_np(x, params, bias=False)[:, 0]
    hi, lo = int(zh.argmax()), int(zh.argmin())
    assert zh[hi] > 0 > zh[lo], "the rows' bias-free logits have one sign"
    for row, target in ((hi, value), (lo, -value)):
        f = lambda a: float(_logits_np(a * x[row:row + 1].astype(np.float64), params)[0, 0]) - target   # noqa: E731
        a0, a1 = 1.0, 4.0 * value / abs(zh[row])
        assert np.sign(f(a0)) != np.sign(f(a1))
        for _ in range(200):
            am = 0.5 * (a0 + a1)
            a0, a1 = (am, a1) if np.sign(f(am)) == np.sign(f(a0)) else (a0, am)
        x[row] = (0.5 * (a0 + a1) * x[row].astype(np.float64)).astype(np.float32)
    return x, hi, lo
