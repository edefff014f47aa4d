"""The InfoNCE check itself, on the CPU: the families of tests/nce_like.py reach their regimes under the fp64 reference
alone, the reference is the reference's InfoNCE, an fp32 restatement of the kernels' stable formulas meets every bound of
``nce_like.bounds`` in every listed case, and each of three subtly wrong fp32 forms (a naive logsumexp - S_pair, the
pair coefficient as exp + exp - 2, a one-sided coefficient 2 p_rj) violates a bound in at least one listed case -- the
proof that tests/test_gpu_nce_like.py would notice such a kernel.  No GPU."""

import math

import pytest
import torch

from tests import nce_like as nl

CASES = nl.cases()


def _naive_loss(z1, z2, tau):
    """ContrastivePretrainer._info_nce as the reference writes it, in the dtype of its inputs."""
    a, b = torch.nn.functional.normalize(z1, dim=1), torch.nn.functional.normalize(z2, dim=1)
    B = a.shape[0]
    s12, s11, s22 = a @ b.T / tau, a @ a.T / tau, b @ b.T / tau
    off = ~torch.eye(B, dtype=torch.bool)
    pos = s12.diag().exp()
    den1 = s12.exp().sum(1) + (s11.exp() * off).sum(1)
    den2 = s12.exp().sum(0) + (s22.exp() * off).sum(1)
    return (-(pos / den1).log() - (pos / den2).log()).mean()


@pytest.mark.parametrize("family", ["gaussian", "paired0.3", "norm_spread"])
@pytest.mark.parametrize("B,P", [(3, 65), (37, 100)])
def test_reference_is_the_reference_loss_and_its_autograd(family, B, P):
    z1, z2 = (t.double().requires_grad_(True) for t in nl.inputs(family, B, P))
    tau, g = 0.2, -2.5
    loss = _naive_loss(z1, z2, tau)
    d1, d2 = torch.autograd.grad(g * loss, (z1, z2))
    ref = nl.reference(*nl.inputs(family, B, P), tau, g)
    assert abs(loss.item() - ref["loss"].item()) <= 1e-12 * abs(loss.item())
    auto = torch.cat((d1, d2))
    scale = auto.abs().max(1).values[:, None]
    assert ((auto - ref["dz"]).abs() <= 1e-10 * scale).all()
    assert torch.allclose(ref["c"], ref["c"].T, rtol=0, atol=1e-15)
    assert torch.allclose(ref["p_pair"] + ref["one_minus_p_pair"], torch.ones(2 * B, dtype=torch.float64), rtol=0, atol=1e-15)


def test_families_reach_their_regimes():
    for B, P in nl.SHAPES:
        if P >= 63:
            ref = nl.case_reference("paired0.05", B, P, 0.05)
            assert (ref["p_pair"] > 0.999).all() and 0 < float(ref["loss"]) < 1e-4, (B, P)
            # the fp64 logsumexp - S_pair itself loses this regime: the reference must not be written that way
            ref = nl.case_reference("paired0.02", B, P, 0.01)
            if B > 1:
                assert (ref["term"] > 0).all() and float(ref["loss"]) < 1e-30, (B, P, float(ref["loss"]))
        ref = nl.case_reference("collapsed", B, P, 0.07)
        if B > 1:
            assert (ref["term"] - math.log(2 * B - 1)).abs().max() <= 1e-12, (B, P)
            assert ref["dz"].abs().max() <= 1e-12 and nl.case_bounds("collapsed", B, P, 0.07)["symmetric"].all(), (B, P)
        if B >= 2:
            ref = nl.case_reference("duplicate_sample", B, P, 0.05)
            S = ref["S"]
            for i, j in nl.duplicates(B):
                assert torch.equal(nl.inputs("duplicate_sample", B, P)[0][i], nl.inputs("duplicate_sample", B, P)[0][j])
                for r in (B + i, B + j) if P >= 63 else ():
                    assert S[r, i] == S[r, j] == S[r].max(), (B, P, r)       # an exact tie at the maximum, off the pair
            assert nl.duplicates(B)[0][1] % 4 != nl.duplicates(B)[0][0] % 4
            assert B < 5 or (nl.duplicates(B)[1][1] - nl.duplicates(B)[1][0]) % 4 == 0
        ref = nl.case_reference("duplicate_pair", B, P, 0.05)
        assert torch.equal(*nl.inputs("duplicate_pair", B, P))
        assert (ref["S"][torch.arange(2 * B), nl._pair(B)] == ref["S"].max(1).values).all()
        nrm = nl.case_reference("norm_spread", B, P, 0.05)["nrm"]
        for k in range(2 * B):
            want = nl.NORMS[k % 5]
            assert abs(float(nrm[k]) - want) <= 1e-6 * want, (B, P, k)
        if B >= 3:
            assert (nrm == 0).any() and ((nrm > 0) & (nrm < nl.EPS)).any()


def test_the_gaussian_control_is_never_taken_for_symmetric():
    for B, P in nl.SHAPES:
        for tau in nl.TAUS:
            sym = nl.case_bounds("gaussian", B, P, tau)["symmetric"]
            if P >= 63 and B >= 2:
                assert not sym.any(), (B, P, tau)
            elif P == 1:
                assert sym.all(), (B, P, tau)                              # n = +-1: dn is parallel to n


def _worst(variant):
    worst = {}
    for case in CASES:
        family, B, P, tau = case
        g = nl.dloss_of(case)
        ref = nl.case_reference(family, B, P, tau, g)
        r = nl.ratios(ref, nl.restatement(*nl.inputs(family, B, P), tau, g, variant), nl.case_bounds(family, B, P, tau, g))
        for k, v in r.items():
            if v > worst.get(k, (-1.0, None))[0]:
                worst[k] = (v, case)
    return worst


def test_the_stable_fp32_restatement_meets_every_bound():
    worst = _worst("stable")
    print("stable fp32 restatement, worst err / bound:", worst)
    for k, (v, case) in worst.items():
        assert v <= 1.0, (k, v, case)


@pytest.mark.parametrize("variant", nl.VARIANTS[1:])
def test_each_mutant_violates_a_bound(variant):
    worst = _worst(variant)
    print(f"{variant}, worst err / bound:", worst)
    assert max(v for v, _ in worst.values()) > 3.0, worst
    paired = [nl.ratios(nl.case_reference(f, B, P, tau, nl.dloss_of((f, B, P, tau))),
                        nl.restatement(*nl.inputs(f, B, P), tau, nl.dloss_of((f, B, P, tau)), variant),
                        nl.case_bounds(f, B, P, tau, nl.dloss_of((f, B, P, tau))))
              for (f, B, P, tau) in CASES if f.startswith("paired") and (B, P) == (33, 1024)]
    assert max(max(r.values()) for r in paired) > 3.0, "a paired case must show it"
