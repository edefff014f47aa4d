"""GPU checks of the binary head step (csrc/binary_head.hip, ops.bin_head_*, gw_whisper_amd/binary.py).

The rule of tests/test_gpu_efficiency.py: the HIP step and the torch fp32 head it can replace (the classifier's
``nn.Sequential`` + ``BCEWithLogitsLoss`` + autograd) are both fp32 chains that differ in summation order, so neither is
privileged.  Both are measured against fp64 on the same inputs in the same test and
    err_hip <= 2 * err_torch + floor
with floor = 20 * 2^-24 * max|logit| for the logits (maximum error) and 20 * 2^-24 for the probabilities (maximum error), the
loss, the row losses, every parameter gradient and the pooled-token gradient (relative Frobenius error).  The fp64 side is
binary_helpers.head64, which tests/test_binary_host.py pins to the reference's own classifier classes through
tests/golden/binary_head.npz; logits, probs and loss of the fixture cases are compared with the stored values directly.
Every case asserts that no hidden pre-activation of its inputs is within 2e-6 of zero before anything is compared.

The measured errors of both sides are in the docstring of test_head_step_against_the_fixture and in
profiles/binary_head.md."""

import numpy as np
import pytest

from . import binary_helpers as bh

pytestmark = pytest.mark.gpu

EPS20 = 20.0 * 2.0 ** -24


@pytest.fixture(scope="module")
def T():
    import torch
    assert torch.cuda.is_available()
    return torch


class _Enc:
    def __init__(self, d):
        self.config = type("Cfg", (), {"d_model": d})()


def _rel(a, ref):
    """Relative Frobenius error in fp64; 0 when both are exactly zero."""
    d = float((a.double() - ref.double()).norm())
    n = float(ref.double().norm())
    return 0.0 if d == 0.0 else d / n if n > 0 else float("inf")


def _classifier(T, layout, params):
    """The torch fp32 head of the layout with ``params`` loaded, on the GPU."""
    from gw_whisper_amd import models
    d_in, C = params[0].shape[1], params[-2].shape[0]
    if layout == bh.ONE:
        cls = models.one_channel_ligo_binary_classifier(_Enc(d_in), num_classes=C).classifier
    else:
        cls = models.two_channel_ligo_binary_classifier(_Enc(d_in // 2), num_classes=C).classifier
    cls = cls.cuda()
    cls.load_state_dict({k: p for k, p in zip(bh.param_keys(layout), params)})
    return cls


def _torch_head(T, layout, params, x, t, upstream):
    """The torch fp32 head the HIP step can replace, with autograd."""
    cls = _classifier(T, layout, params)
    xr = x.detach().clone().requires_grad_(True)
    z = cls(xr)
    loss = T.nn.BCEWithLogitsLoss()(z, t)
    (loss * upstream).backward()
    sd = cls.state_dict(keep_vars=True)
    rows = T.nn.functional.binary_cross_entropy_with_logits(z.detach(), t, reduction="none").sum(1)
    return loss.detach(), z.detach(), T.sigmoid(z.detach()), rows, xr.grad, [sd[k].grad for k in bh.param_keys(layout)]


def _compare(T, tag, layout, x, params, t, upstream=1.0, fixture=None):
    """One head step three ways; prints both errors of every quantity, asserts the rule.  Returns the HIP outputs."""
    from gw_whisper_amd import ops
    B, C = t.shape
    g = T.tensor([upstream], dtype=T.float32, device=x.device)
    loss, logits, probs, row_loss, saved = ops.bin_head_forward(layout, x, params, t)
    dx, grads = ops.bin_head_backward(saved, g)
    l64, z64, p64, rows64, dx64, g64, margin = bh.head64(x, params, t, upstream)
    assert margin >= bh.MARGIN, f"{tag}: a hidden pre-activation of the test's own inputs is {margin:.2e} from zero"
    if fixture is not None:       # the stored fp64 values of the reference's classifier classes
        z64, p64 = T.from_numpy(fixture[0]).to(x.device), T.from_numpy(fixture[1]).to(x.device)
        l64 = T.tensor(float(fixture[2]), dtype=T.float64, device=x.device)
    lt, zt, pt, rowst, dxt, gt = _torch_head(T, layout, params, x, t, upstream)
    zmax = float(z64.abs().max())
    for name, a, b, c, floor in (("logits", logits, zt, z64, EPS20 * zmax), ("probs", probs, pt, p64, EPS20)):
        e_hip, e_t = float((a.double() - c).abs().max()), float((b.double() - c).abs().max())
        print(f"{tag}: {name} max err hip {e_hip:.2e} torch {e_t:.2e} (max|logit| {zmax:.3f})")
        assert e_hip <= 2 * e_t + floor, (tag, name, e_hip, e_t)
    rows = [("loss", loss.reshape(()), lt, l64), ("row_loss", row_loss, rowst, rows64), ("d_pooled", dx, dxt, dx64)]
    rows += [(f"d_{k}", a, b, c) for k, a, b, c in zip(bh.param_keys(layout), grads, gt, g64)]
    for name, a, b, c in rows:
        assert bool(T.isfinite(a).all()), (tag, name)
        eh_, et = _rel(a, c), _rel(b, c)
        print(f"{tag}: {name:12s} rel err hip {eh_:.2e} torch {et:.2e}")
        assert eh_ <= 2 * et + EPS20, (tag, name, eh_, et)
    # the batch mean is the fp64 sum of the fp32 row losses over B C, rounded once
    assert abs(float(loss) - float(row_loss.double().sum()) / (B * C)) <= 2.0 ** -23 * abs(float(loss))
    assert tuple(dx.shape) == tuple(x.shape) and [tuple(a.shape) for a in grads] == [tuple(p.shape) for p in params]
    return loss, logits, probs, row_loss, saved, dx, grads


def _fixture_case(T, g, ci):
    layout, d_in, C, B = bh.CASES[ci]
    x, t = bh.case_inputs(d_in, C, B, int(g["seeds"][ci]))
    return layout, T.from_numpy(x).cuda(), T.from_numpy(t).cuda(), [T.from_numpy(p).cuda() for p in bh.case_params(ci, layout, d_in, C)]


@pytest.mark.parametrize("ci", range(len(bh.CASES)))
def test_head_step_against_the_fixture(T, gww, golden, ci):
    """(layout, d_in, C, B) of binary_helpers.CASES; hard targets.  Measured on MI355X, worst of the ten cases, HIP /
    torch: logits 7.6e-8 / 5.1e-8 (max|logit| 0.14, floor 1.7e-7), probs 4.2e-8 / 5.5e-8, loss 4.0e-8 / 9.3e-8, row losses 4.2e-8 / 5.8e-8, pooled-token
    gradient 5.6e-7 / 5.4e-7, worst parameter gradient (the two-detector head's last hidden weight at d_in = 2560, B = 33)
    1.3e-6 / 7.1e-7 relative (profiles/binary_head.md)."""
    g = golden("binary_head.npz")
    assert tuple(g["cases"][ci].tolist()) == bh.CASES[ci]
    layout, x, t, params = _fixture_case(T, g, ci)
    _compare(T, f"case {ci} {bh.CASES[ci]}", layout, x, params, t,
             fixture=(g[f"head{ci}_logits"], g[f"head{ci}_probs"], g[f"head{ci}_loss"]))


@pytest.mark.parametrize("ci", (3, 9))
def test_head_step_soft_targets_and_upstream_gradient(T, gww, golden, ci):
    """Targets anywhere in [0, 1] with exact 0 and 1 among them, C = 3 (one detector) and C = 2 (two), upstream gradient
    0.37."""
    layout, x, t, params = _fixture_case(T, golden("binary_head.npz"), ci)
    soft = T.rand(t.shape, generator=T.Generator().manual_seed(5)).cuda()
    soft[0], soft[1] = t[0], 1.0 - t[1]
    assert bool((soft == 0).any() | (soft == 1).any())
    _compare(T, f"case {ci} soft targets, upstream 0.37", layout, x, params, soft, upstream=0.37)


@pytest.mark.parametrize("ci", (1, 5))
def test_head_step_confident_and_wrong_rows(T, gww, golden, ci):
    """One row with a logit of +120 labelled 0 and one with -120 labelled 1 (B = 17, both layouts; the rows of
    binary_helpers.with_extreme_rows): the loss has no clamp (the rows' losses are 120, not 100), everything is finite, and
    the sigmoid of the two rows is exactly 1 and 0; their dz is exactly +-1 / B."""
    g = golden("binary_head.npz")
    layout, d_in, C, B = bh.CASES[ci]
    x, t = bh.case_inputs(d_in, C, B, int(g["seeds"][ci]))
    params = bh.case_params(ci, layout, d_in, C)
    x, hi, lo = bh.with_extreme_rows(x, params, 120.0)
    t[hi], t[lo] = 0.0, 1.0
    x, t, params = T.from_numpy(x).cuda(), T.from_numpy(t).cuda(), [T.from_numpy(p).cuda() for p in params]
    z64 = bh.head64(x, params, t)[1]
    assert abs(float(z64[hi, 0]) - 120.0) < 1e-2 and abs(float(z64[lo, 0]) + 120.0) < 1e-2
    rest = [i for i in range(B) if i not in (hi, lo)]
    assert float(z64[rest].abs().max()) < 1.0
    loss, logits, probs, row_loss, saved, dx, grads = _compare(T, f"case {ci} logits +-120", layout, x, params, t)
    assert float(probs[hi, 0]) == 1.0 and float(probs[lo, 0]) == 0.0
    assert abs(float(row_loss[hi]) - 120.0) < 1e-2 and abs(float(row_loss[lo]) - 120.0) < 1e-2
    dz = saved[4]
    assert float(dz[hi, 0]) == np.float32(1.0 / B) and float(dz[lo, 0]) == np.float32(-1.0 / B)
    assert float(loss) > 240.0 / B


def test_head_step_is_deterministic_and_scores_equal_the_forward(T, gww, golden):
    """A second identical call gives identical bits (outputs, saved activations, dz, every gradient); the scores entry and
    binary.head_logits give the forward's logits bit for bit."""
    from gw_whisper_amd import binary, ops
    g = golden("binary_head.npz")
    for ci in (2, 3, 6, 7, 8):
        layout, x, t, params = _fixture_case(T, g, ci)
        up = T.tensor([0.5], device="cuda")
        outs = []
        for _ in range(2):
            loss, logits, probs, row_loss, saved = ops.bin_head_forward(layout, x, params, t)
            dx, grads = ops.bin_head_backward(saved, up)
            outs.append([loss, logits, probs, row_loss, dx, *grads, *saved[3], saved[4]])
        for a, b in zip(*outs):
            assert T.equal(a, b)
        assert T.equal(ops.bin_head_scores(layout, x, params), logits), ci
        assert T.equal(binary.head_logits(_classifier(T, layout, params), x), logits), ci


def test_one_detector_logits_are_the_detection_heads(T, gww):
    """The one-detector layout at C = 2 is the detection head's chain: at equal weights its logits (and saved activations)
    are the bits of ops.det_head_forward's."""
    from gw_whisper_amd import ops, synth
    for d_in, B in ((384, 33), (1280, 5)):
        sd = synth.head_state_dict([d_in, 512, 256, 128, 64, 2], seed=31)
        params = [T.from_numpy(sd[k]).cuda() for k in bh.param_keys(bh.ONE)]
        x, t = bh.case_inputs(d_in, 2, B, 77)
        x, t = T.from_numpy(x).cuda(), T.from_numpy(t).cuda()
        onehot = T.stack((t[:, 0], 1.0 - t[:, 0]), dim=1).contiguous()
        _, zdet, _, _, sdet = ops.det_head_forward(x, params, onehot)
        _, zbin, _, _, sbin = ops.bin_head_forward(ops.BIN_HEAD_ONE, x, params, t)
        assert T.equal(zbin, zdet)
        for a, b in zip(sbin[3], sdet[2]):
            assert T.equal(a, b)
        assert T.equal(ops.bin_head_scores(ops.BIN_HEAD_ONE, x, params), zdet)


def test_one_detector_backward_is_the_detection_heads(T, gww):
    """... and so is its backward: from the same dz and upstream gradient, dx and all ten gradients are the bits of
    ops.det_head_backward's.  B = 17: one full 16-row block and a ragged one; d_in = 128: the smallest width; C = 2: below a
    16-column tile."""
    from gw_whisper_amd import ops, synth
    d_in, B, C = 128, 17, 2
    sd = synth.head_state_dict([d_in, 512, 256, 128, 64, C], seed=31)
    params = [T.from_numpy(sd[k]).cuda() for k in bh.param_keys(bh.ONE)]
    x, t = bh.case_inputs(d_in, C, B, 77)
    x, t = T.from_numpy(x).cuda(), T.from_numpy(t).cuda()
    ops.det_head_forward(x, params, t)
    *_, (_, xs, ps, h, dz) = ops.bin_head_forward(ops.BIN_HEAD_ONE, x, params, t)
    up = T.tensor([0.37], device="cuda")
    dx_bin, g_bin = ops.bin_head_backward((ops.BIN_HEAD_ONE, xs, ps, h, dz), up)
    dx_det, g_det = ops.det_head_backward((xs, ps, h, dz), up)
    assert len(g_bin) == len(g_det) == 10
    for a, b in zip([dx_bin, *g_bin], [dx_det, *g_det]):
        assert T.equal(a.view(T.int32), b.view(T.int32))


@pytest.mark.parametrize("ci", (2, 8))
def test_binary_eval_accumulate_gives_the_forwards_loss(T, gww, golden, ci):
    """roc.BinaryEvalState on the kernel's logits against the forward's loss.  Both are fp64 evaluations of the same fp32
    logits; the forward rounds each row loss to fp32 (2^-25 relative each, so at most 2^-25 of their mean) and its mean
    once more, the state rounds its mean once: they differ by less than 3 * 2^-25 <= 2^-23 of the loss."""
    from gw_whisper_amd import roc
    layout, x, t, params = _fixture_case(T, golden("binary_head.npz"), ci)
    from gw_whisper_amd import ops
    loss, logits, probs, _, _ = ops.bin_head_forward(layout, x, params, t)
    state = roc.BinaryEvalState(x.shape[0], x.device, with_snr=False)
    state.add(logits, t)
    r = state.read()
    assert r["batches"] == 1
    assert abs(r["loss"] - float(loss)) <= 2.0 ** -23 * float(loss), (r["loss"], float(loss))
    # both sigmoids are fp64 evaluations of the same logit, rounded to fp32 once
    assert float(np.abs(r["scores"].astype(np.float64) - probs.reshape(-1).cpu().numpy()).max()) <= 2.0 ** -24


def test_autograd_function_routes_the_gradients(T, gww, golden):
    """binary.head_bce_with_logits: the loss, the classifier's parameter gradients and the pooled-token gradient are the
    bits of the raw ops; the logits carry no gradient."""
    from gw_whisper_amd import binary, ops
    for ci in (1, 5):
        layout, x, t, params = _fixture_case(T, golden("binary_head.npz"), ci)
        cls = _classifier(T, layout, params)
        xr = x.clone().requires_grad_(True)
        loss, logits = binary.head_bce_with_logits(cls, xr, t)
        assert loss.dim() == 0 and loss.requires_grad and not logits.requires_grad
        (loss * 0.37).backward()
        l0, z0, _, _, saved = ops.bin_head_forward(layout, x, params, t)
        dx0, g0 = ops.bin_head_backward(saved, T.tensor([0.37], device="cuda"))
        assert T.equal(loss.detach().reshape(1), l0) and T.equal(logits, z0) and T.equal(xr.grad, dx0)
        sd = cls.state_dict(keep_vars=True)
        for k, gg in zip(bh.param_keys(layout), g0):
            assert T.equal(sd[k].grad, gg), k
