"""gww_info_nce_forward_f32 / gww_info_nce_backward_f32 (csrc/contrastive.hip) per row against the fp64 reference of
tests/nce_like.py, in the regimes contrastive pretraining reaches: pairs that dominate their rows (a loss of 1e-6 and
below), a collapsed batch, duplicated pairs and samples (ties at the row maximum, across and within the kernels' waves),
row norms from 0 over sub-eps to 1e15, at the (B, P) where the kernels' index arithmetic changes.  The bounds are
``nce_like.bounds``: derived from the reference and fp32's constants; tests/test_nce_like_host.py shows on the CPU that a
naive logsumexp - S_pair, an exp + exp - 2 pair coefficient and a one-sided coefficient each violate them."""

import numpy as np
import pytest

from tests import nce_like as nl

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def T():
    import torch
    assert torch.cuda.is_available()
    return torch


def _bits(t):
    return t.detach().cpu().contiguous().view(-1).numpy().view(np.uint32)


def _run(T, gww, z1, z2, tau, g):
    """One forward + backward through gw_whisper_amd.ops on the device: the dict ``nce_like.ratios`` takes, plus nrm."""
    from gw_whisper_amd import ops
    loss, (n, nrm, lse, term) = ops.info_nce_forward(z1, z2, tau)
    dz1, dz2 = ops.info_nce_backward((n, nrm, lse, term), tau, T.tensor([g], dtype=T.float32, device="cuda"))
    return dict(term=term.cpu(), lse=lse.cpu(), loss=loss.cpu()[0], dz=T.cat((dz1, dz2)).cpu(), nrm=nrm.cpu(), n=n.cpu())


def _family_cases(B, P):
    return [c for c in nl.cases() if (c[1], c[2]) == (B, P)]


@pytest.mark.parametrize("B,P", nl.SHAPES)
def test_info_nce_meets_the_per_row_bounds_in_every_family(T, gww, B, P):
    """Every (family, tau) of nce_like at one (B, P), with the case's upstream scalar (1, 0.37, -2.5 in turn): per-row
    term and lse, the loss and every element of dz1 / dz2 and of the normalised rows within nce_like.bounds; |z| to
    (P/64 + 8) 2^-24; everything finite; a second call gives the same bits; mlgwsc_train.info_nce under autograd with
    (c * loss).backward() gives the bits of the ops path.

    Worst err / bound over the families and temperatures, measured on an MI355X (gfx950):
      (B, P)      term   lse    n      loss   dz     |z|
      (1, 1)      0.000  0.013  0.073  0.000  0.000  0.000
      (2, 1)      0.034  0.055  0.073  0.034  0.005  0.000
      (3, 63)     0.119  0.209  0.196  0.073  0.044  0.152
      (3, 64)     0.190  0.295  0.192  0.105  0.070  0.152
      (3, 65)     0.109  0.182  0.203  0.072  0.062  0.142
      (5, 257)    0.145  0.302  0.163  0.022  0.036  0.117
      (33, 1024)  0.078  0.172  0.101  0.011  0.020  0.069
      (32, 128)   0.103  0.278  0.190  0.039  0.050  0.144
      (37, 100)   0.162  0.283  0.186  0.023  0.061  0.141"""
    from gw_whisper_amd.mlgwsc_train import info_nce
    failures, worst = [], {}
    for case in _family_cases(B, P):
        family, _, _, tau = case
        g = nl.dloss_of(case)
        ref = nl.case_reference(family, B, P, tau, g)
        z1, z2 = (t.cuda() for t in nl.inputs(family, B, P))
        got, again = _run(T, gww, z1, z2, tau, g), _run(T, gww, z1, z2, tau, g)
        for k in got:
            assert np.array_equal(_bits(got[k]), _bits(again[k])), (case, k, "two calls differ")
            assert T.isfinite(got[k]).all(), (case, k, "not finite")
        a1, a2 = z1.clone().requires_grad_(True), z2.clone().requires_grad_(True)
        loss = info_nce(a1, a2, tau)
        (g * loss).backward()
        assert np.array_equal(_bits(loss), _bits(got["loss"])), (case, "autograd loss")
        assert np.array_equal(_bits(T.cat((a1.grad, a2.grad))), _bits(got["dz"])), (case, "autograd gradients")
        r = nl.ratios(ref, got, nl.case_bounds(family, B, P, tau, g))
        r["nrm"] = float(((got["nrm"].double() - ref["nrm"]).abs() / ((P / 64 + 8) * nl.U * ref["nrm"]).clamp_min(1e-300)).max())
        print(f"InfoNCE {family:>16} B {B:>2} P {P:>4} tau {tau:<4} g {g:>5}: loss {float(got['loss']):.6e} (fp64 "
              f"{float(ref['loss']):.6e})  err / bound: " + "  ".join(f"{k} {v:.3f}" for k, v in r.items()))
        for k, v in r.items():
            worst[k] = max(worst.get(k, 0.0), v)
            if not v <= 1.0:
                failures.append((case, k, v))
    print(f"InfoNCE B {B} P {P}: worst err / bound " + "  ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    assert not failures, failures


@pytest.mark.parametrize("B,P", [(2, 1), (3, 65), (33, 1024)])
def test_a_zero_upstream_gradient_gives_exact_zeros(T, gww, B, P):
    """dloss = 0 (and -0.0): every element of dz1 and dz2 is a zero, in every family and at every temperature."""
    for family, _, _, tau in _family_cases(B, P):
        z1, z2 = (t.cuda() for t in nl.inputs(family, B, P))
        for zero in (0.0, -0.0):
            dz = _run(T, gww, z1, z2, tau, zero)["dz"]
            assert (dz == 0).all(), (family, tau, zero)


@pytest.mark.parametrize("B,P", [(3, 65), (5, 257), (32, 128)])
def test_bf16_z1_with_fp32_z2_returns_gradients_in_the_input_dtypes(T, gww, B, P):
    """mlgwsc_train.info_nce on a bf16 z1 and an fp32 z2: the loss and dz2 under the bounds of the reference on the
    rounded inputs, dz1 in bf16 under the same bounds plus its own rounding 2^-8 (|ref| + bound) (bf16 keeps 8 significant
    bits, so round-to-nearest moves a value by at most 2^-8 of itself), dz2 in fp32.

    Worst err / bound measured on an MI355X (gfx950) over the three shapes: loss 0.066, dz 0.979 -- the bf16 rounding
    of dz1 is nearly the whole of its bound, and an element just above a power of two uses all of it."""
    from gw_whisper_amd.mlgwsc_train import info_nce
    failures = []
    for case in _family_cases(B, P):
        family, _, _, tau = case
        g = nl.dloss_of(case)
        z1, z2 = nl.inputs(family, B, P)
        z1 = z1.to(T.bfloat16)
        ref = nl.reference(z1.float(), z2, tau, g)
        bnd = nl.bounds(ref, nl.symmetric_ok(family, B, P))
        a1, a2 = z1.cuda().requires_grad_(True), z2.cuda().requires_grad_(True)
        loss = info_nce(a1, a2, tau)
        (g * loss).backward()
        assert a1.grad.dtype == T.bfloat16 and a2.grad.dtype == T.float32 and loss.dtype == T.float32
        extra = 2.0 ** -8 * (ref["dz"].abs() + bnd["dz"])
        extra[B:] = 0.0
        got = dict(loss=loss.detach().cpu(), dz=T.cat((a1.grad.float(), a2.grad)).cpu())
        assert T.isfinite(got["dz"]).all() and T.isfinite(got["loss"]), case
        r = nl.ratios(ref, got, bnd, extra_dz=extra)
        print(f"InfoNCE bf16 z1 {family:>16} B {B} P {P} tau {tau}: err / bound loss {r['loss']:.3f} dz {r['dz']:.3f}")
        failures += [(case, k, v) for k, v in r.items() if not v <= 1.0]
    assert not failures, failures


def test_dz1_and_dz2_are_the_rows_of_z1_and_z2(T, gww):
    """duplicate_sample at (5, 257): z1[0] == z1[1] == z1[4] while their partners in z2 differ, so the reference's
    dz1 and dz2 differ by far more than the bound in every row and an exchange of the two outputs cannot pass."""
    from gw_whisper_amd import ops
    family, B, P, tau = "duplicate_sample", 5, 257, 0.2
    ref = nl.case_reference(family, B, P, tau, 1.0)
    bnd = nl.case_bounds(family, B, P, tau, 1.0)
    swapped = T.cat((ref["dz"][B:], ref["dz"][:B]))
    assert ((swapped - ref["dz"]).abs().max(1).values > 100 * bnd["dz"].max(1).values).all()
    z1, z2 = (t.cuda() for t in nl.inputs(family, B, P))
    loss, saved = ops.info_nce_forward(z1, z2, tau)
    dz1, dz2 = ops.info_nce_backward(saved, tau, T.ones(1, device="cuda"))
    assert dz1.shape == z1.shape and dz2.shape == z2.shape
    assert ((dz1.cpu().double() - ref["dz"][:B]).abs() <= bnd["dz"][:B]).all()
    assert ((dz2.cpu().double() - ref["dz"][B:]).abs() <= bnd["dz"][B:]).all()
