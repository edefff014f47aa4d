"""InfoNCE in the regimes contrastive pretraining reaches: seeded input families, the fp64 reference of
``gww_info_nce_forward_f32`` / ``gww_info_nce_backward_f32`` (csrc/contrastive.hip), the per-row error bounds the GPU test
(tests/test_gpu_nce_like.py) applies, and an fp32 torch restatement of the kernels' formulas with three mutants that the
CPU test (tests/test_nce_like_host.py) holds against the same bounds.

Every bound is computed from the reference's fp64 quantities and fp32 format constants, never from a kernel's output.

Notation: N = 2B rows Z = [normalize(z1); normalize(z2)], S = Z Z^T / tau without its diagonal, pair(r) = r +- B,
p_rj = softmax_j(S_r.), term_r = LSE_j S_rj - S_r,pair = -log p_r,pair, loss = (1/B) sum_r term_r.

delta -- the absolute error of one computed S_rj:  delta_r = (P/64 + 10) 2^-24 / tau + 2^-24 max_j |S_rj|.
    A lane of the kernel sums P/64 products, the butterfly adds 6 more roundings; both rows were normalised in fp32
    (square sum, sqrt, division: the remaining units of the 10); one division by tau rounds at 2^-24 |S|.

n -- |err_rp| <= (P/64 + 10) 2^-24 |n_rp|, the normalisation's share of delta: the square sum (P/64 additions and a
    butterfly), the square root, the division, and eps itself, which the kernel holds in fp32.  A zero row is exact.

term -- |err_r| <= 2 delta (1 - p_pair) + 2^-22 |term_r| + 2B 2^-126.
    term_r = log(1 + sum_{j != pair} exp(S_rj - S_r,pair)): a shift of every S by at most delta moves each exponent by at
    most 2 delta, and d term / d exponent_j = p_rj, which sum to 1 - p_pair over j != pair.  The evaluation itself (expf,
    log1pf, two additions) is relative to term; the last summand is the fp32 underflow of the 2B exponentials of `rest`.

lse -- |err_r| <= delta + 2^-24 |lse_r|.
    The softmax weights sum to 1, so errors of at most delta in every S move lse by at most delta.  The one operation
    delta does not hold is the last addition M + log1p(rest), which rounds at 2^-24 |lse|.  (expf and log1pf round a
    few 2^-24 more on log1p(rest) <= log 2B; they get no allowance of their own -- delta counts every addition of the
    cosine at its worst case.)

loss -- |err| <= (1/B) sum_r bound(term_r).

gradient, per row r, per element p --
    |dz_rp - ref| <= 1e-5 max_p |ref_r| + (P/256 + 12) 2^-24 (max_p |dn_r| + |n_r . dn_r|) / |z_r|
                     + coef_rp + (|g| / (B tau)) 4B 2^-126 / |z_r|,          |z_r| read as max(|z_r|, eps) throughout.
    The first summand is the project's InfoNCE bound (tests/test_gpu_mlgwsc_train.py) applied to the row instead of the
    batch; the second is the rounding of the projection dn - n (n . dn) (P/256 elements per thread, a butterfly, the
    combination of four waves, the product, the difference and the division), which cancels when dn is parallel to n.
    Rows with |z| < eps take the reference's dn / eps branch under the same bound.

    coef is a rounding source the first two summands do not hold: the coefficients of
    dn_r = (g / (B tau)) sum_j c_rj n_j,  c_rj = p_rj + p_jr - 2 [j == pair],  are expf(S_rj - lse), and S and lse each
    carry delta, so the exponent is off by up to 2 max(delta_r, delta_j) and |err c_rj| <= 2 max(delta_r, delta_j) |c_rj|
    to first order (the pair's expm1(-term) likewise, by the bound of term).  At tau = 0.01 one fp32 rounding of S ~ 100
    is 4e-6, which alone is a relative 4e-6 of every coefficient, and the worst case delta allows is 1e-4: an fp32
    evaluation cannot hold 1e-5 of a row there, whatever its formulas.  On dn that is
        e_rp = (|g| / (B tau)) sum_j 2 max(delta_r, delta_j) |c_rj| |n_jp|
    and through the projection  coef_rp = (e_rp + |n_rp| sum_q |n_rq| e_rq) / |z_r|.
    The last summand is the fp32 underflow of the two exponentials of each of the 2B coefficients (rows whose pair
    dominates at tau = 0.01 have gradients near 1e-31 and coefficients below the smallest normal number).

rows whose gradient vanishes by symmetry -- there every summand above is (almost) zero when sum_j c_rj n_j cancels
    exactly (collapsed rows, P = 1), while the kernel's sum keeps the rounding of its additions: a wave adds 2B/4
    products, the four waves, g / (B tau) and the division by |z| add 8 more roundings, and |n_jp| <= 1:
        + (|g| / (B tau)) sum_j |c_rj| (2B/4 + 8) 2^-24 / |z_r|
    (with coef above this is the bound (|g| / (B tau)) sum_j |c_rj| (2 delta + (2B/4 + 8) 2^-24) / |z_r|).
    It is added to the row's bound only where the fp64 |dz_r| is at most 1e-12 of the size the row's gradient has without
    the symmetry, (|g| / (B tau)) sum_j |c_rj| max_p |n_jp| / |z_r| -- which is what a Gaussian control row's gradient
    is made of (tests/test_nce_like_host.py asserts that the control's rows are never taken for symmetric at P >= 63,
    B >= 2).  ``bounds`` applies that condition itself, and asserts that such rows occur only where a symmetry
    exists (``symmetric_ok``): in a collapsed batch, at P = 1 (n = +-1, so dn is parallel to n) and at B = 1, where every
    c is 0 and the bound is an exact zero.

what the gradient bound does not see -- coef takes delta at its worst case (every addition of the cosine rounding the
    same way), about 5 x what the first two summands allow at tau >= 0.05.  It is a bound, not an estimate; a tighter
    one would have to assume independent roundings.  In the paired cases at (33, 1024) and (32, 128) the naive_lse and
    exp_exp_2 forms exceed it by 5 x to 10^4 x at tau = 0.07 and 0.05; at tau = 0.2 no pair dominates its row (p_pair near
    0.7), those forms lose nothing there and stay below 0.05 of the bound; at tau = 0.01 and (33, 1024) the paired(0.05)
    and paired(0.02) gradients (1e-30 and below) lie under the underflow summand, so those two cases check the forward
    and finiteness only.
"""

import functools
import math

import numpy as np
import torch

EPS = 1e-12                                    # F.normalize's eps
U = 2.0 ** -24                                 # fp32 unit roundoff
FAMILIES = ("paired0.3", "paired0.05", "paired0.02", "collapsed", "duplicate_pair", "duplicate_sample", "norm_spread",
            "gaussian")
SHAPES = ((1, 1), (2, 1), (3, 63), (3, 64), (3, 65), (5, 257), (33, 1024), (32, 128), (37, 100))
TAUS = (0.2, 0.07, 0.05, 0.01)
DLOSS = (1.0, 0.37, -2.5, 0.0)
NORMS = (1e-15, 1e-13, 1.0, 1e15, 0.0)         # norm_spread's row norms, cyclic over the 2B rows
VARIANTS = ("stable", "naive_lse", "exp_exp_2", "one_sided")


def cases():
    """Every (family, B, P, tau) of the tables above; duplicate_sample needs two rows in z1."""
    return [(f, B, P, tau) for f in FAMILIES for (B, P) in SHAPES for tau in TAUS if not (f == "duplicate_sample" and B < 2)]


def dloss_of(case):
    """The upstream scalar a case runs with: 1, 0.37 and -2.5 in turn over the list of cases (0 is tested on its own)."""
    return DLOSS[cases().index(case) % 3]


def duplicates(B):
    """(i, j) with z1[i] == z1[j] in duplicate_sample: columns i and j of S fall to different waves of the kernels
    (j - i not a multiple of 4) and, from B = 5 on, to the same wave as well."""
    d = [(0, 1)]
    if B >= 7:
        d.append((2, 6))
    elif B >= 5:
        d.append((0, 4))
    return d


@functools.lru_cache(maxsize=None)
def inputs(family, B, P):
    """(z1, z2) fp32 [B, P] of a family, seeded by (family, B, P); do not modify."""
    rng = np.random.default_rng([FAMILIES.index(family), B, P])
    z1 = rng.standard_normal((B, P))
    noise = rng.standard_normal((B, P))
    if family.startswith("paired"):
        z2 = z1 + float(family[len("paired"):]) * noise
    elif family == "collapsed":
        z1 = np.repeat(z1[:1], B, axis=0)
        z2 = z1.copy()
    elif family == "duplicate_pair":
        z2 = z1.copy()
    elif family == "duplicate_sample":
        for i, j in duplicates(B):
            z1[j] = z1[i]
        z2 = z1 + 0.3 * noise                  # the pair is each row's maximum, so rows B + i, B + j tie there off the pair
    elif family == "norm_spread":
        z = np.concatenate((z1, noise))
        z /= np.linalg.norm(z, axis=1, keepdims=True)
        z *= np.asarray([NORMS[k % len(NORMS)] for k in range(2 * B)])[:, None]
        z1, z2 = z[:B], z[B:]
    elif family == "gaussian":
        z2 = noise
    else:
        raise ValueError(family)
    return torch.from_numpy(z1.astype(np.float32)), torch.from_numpy(z2.astype(np.float32))


def _pair(B):
    return torch.cat((torch.arange(B, 2 * B), torch.arange(0, B)))


def reference(z1, z2, tau, g=1.0):
    """fp64 InfoNCE on the given (fp32 or bf16) inputs in the max-subtracted log1p form: a dict of ``term``, ``lse``,
    ``p_pair``, ``one_minus_p_pair``, ``loss``, ``S`` (diagonal -inf), ``n``, ``nrm`` (|z|), ``c`` (c_rj, diagonal 0),
    ``dn`` and ``dz`` ([2B, P]: the rows of z1, then of z2), the gradients scaled by the upstream scalar g."""
    z = torch.cat((z1, z2)).to(torch.float64)
    N, P = z.shape
    B = N // 2
    nrm = z.square().sum(1).sqrt()
    n = z / nrm.clamp_min(EPS)[:, None]
    S = (n[:, None, :] * n[None, :, :]).sum(-1) / tau      # one summation order for every element: equal rows tie exactly
    eye = torch.eye(N, dtype=torch.bool)
    S = S.masked_fill(eye, -math.inf)
    rows, pair = torch.arange(N), _pair(B)
    M, jstar = S.max(1)
    E = (S - M[:, None]).exp()
    E[rows, jstar] = 0.0                                   # the maximum is the 1 of log1p
    lp = E.sum(1).log1p()
    lse = M + lp
    term = (M - S[rows, pair]) + lp
    c = (S - lse[:, None]).exp() + (S - lse[None, :]).exp()
    c[rows, pair] = torch.expm1(-term) + torch.expm1(-term[pair])
    c = c.masked_fill(eye, 0.0)
    dn = (g / (B * tau)) * (c @ n)
    dot = (n * dn).sum(1)
    dz = torch.where((nrm >= EPS)[:, None], (dn - n * dot[:, None]) / nrm.clamp_min(EPS)[:, None], dn / EPS)
    return dict(term=term, lse=lse, p_pair=(-term).exp(), one_minus_p_pair=-torch.expm1(-term), loss=term.sum() / B, S=S, n=n,
                nrm=nrm, c=c, dn=dn, dz=dz, dot=dot, B=B, P=P, tau=tau, g=g)


@functools.lru_cache(maxsize=None)
def case_reference(family, B, P, tau, g=1.0):
    """``reference`` of a listed case, computed once; do not modify."""
    return reference(*inputs(family, B, P), tau, g)


def case_bounds(family, B, P, tau, g=1.0):
    """``bounds`` of a listed case."""
    return bounds(case_reference(family, B, P, tau, g), symmetric_ok(family, B, P))


def symmetric_ok(family, B, P):
    """Whether rows of this case may have a gradient that vanishes by symmetry."""
    return family == "collapsed" or P == 1 or B == 1


def bounds(ref, symmetric_ok):
    """dict of ``term`` [2B], ``lse`` [2B], ``loss`` (float), ``dz`` [2B, P] and
    ``symmetric`` [2B] (bool: the rows that got the symmetry bound); see the module docstring.  ``symmetric_ok``: whether
    the case may have such rows at all (``symmetric_ok(family, B, P)``); asserted."""
    B, P, tau, g = ref["B"], ref["P"], ref["tau"], ref["g"]
    N = 2 * B
    S = ref["S"]
    smax = S.masked_fill(torch.eye(N, dtype=torch.bool), 0.0).abs().max(1).values
    delta = (P / 64 + 10) * U / tau + U * smax
    term = 2 * delta * ref["one_minus_p_pair"] + 2.0 ** -22 * ref["term"].abs() + N * 2.0 ** -126
    lse = delta + U * ref["lse"].abs()
    den = ref["nrm"].clamp_min(EPS)
    k = abs(g) / (B * tau)
    n_abs, cabs = ref["n"].abs(), ref["c"].abs()
    row = 1e-5 * ref["dz"].abs().max(1).values + (P / 256 + 12) * U * (ref["dn"].abs().max(1).values + ref["dot"].abs()) / den
    row = row + k * 2 * N * 2.0 ** -126 / den
    coef = k * ((cabs * 2 * torch.maximum(delta[:, None], delta[None, :])) @ n_abs)             # [2B, P], on dn
    coef = (coef + n_abs * (n_abs * coef).sum(1, keepdim=True)) / den[:, None]                  # through the projection
    unsym = k * (cabs * n_abs.max(1).values[None, :]).sum(1) / den
    symmetric = ref["dz"].abs().max(1).values <= 1e-12 * unsym
    assert symmetric_ok or not symmetric.any(), "a row without a symmetry fell under the threshold of the symmetry bound"
    row = torch.where(symmetric, row + k * cabs.sum(1) * (N / 4 + 8) * U / den, row)
    dz = row[:, None] + coef
    n = (P / 64 + 10) * U * n_abs
    return dict(term=term, lse=lse, loss=float(term.sum() / B), dz=dz, n=n, symmetric=symmetric)


def ratios(ref, got, bnd, extra_dz=None):
    """Worst err / bound of ``got`` (a dict of ``term``, ``lse`` [2B], ``loss``, ``dz`` and ``n`` [2B, P]; missing keys are
    left out) per quantity.  A zero error under a zero bound is ratio 0, a nonzero error under a zero bound is inf, anything
    that is not finite is inf.  ``extra_dz`` [2B, P] is added to the gradient's bound (the rounding of a bf16 result)."""
    out = {}

    def ratio(err, b):
        err = torch.as_tensor(err, dtype=torch.float64)
        b = torch.as_tensor(b, dtype=torch.float64).expand_as(err)
        r = torch.where(err == 0, torch.zeros_like(err), err / b)      # x / 0 = inf for x > 0
        r = torch.where(torch.isfinite(err), r, torch.full_like(err, math.inf))
        return float(r.max())

    for k in ("term", "lse", "n"):
        if k in got:
            out[k] = ratio((got[k].double() - ref[k]).abs(), bnd[k])
    if "loss" in got:
        out["loss"] = ratio(abs(float(got["loss"]) - float(ref["loss"])), bnd["loss"])
    if "dz" in got:
        b = bnd["dz"]
        if extra_dz is not None:
            b = b + extra_dz
        out["dz"] = ratio((got["dz"].double() - ref["dz"]).abs(), b)
    return out


def restatement(z1, z2, tau, g=1.0, variant="stable"):
    """The kernels' formulas in fp32 torch on the CPU (``variant`` "stable"), or one of the three subtly wrong forms the
    bounds must tell from it: "naive_lse" (term = logsumexp - S_pair), "exp_exp_2" (the pair's coefficient as
    exp + exp - 2) and "one_sided" (c_rj = 2 p_rj).  Returns the dict ``ratios`` takes."""
    assert variant in VARIANTS
    f = torch.float32
    z = torch.cat((z1, z2)).to(f)
    N, P = z.shape
    B = N // 2
    tau32, eps32 = torch.tensor(tau, dtype=f), torch.tensor(EPS, dtype=f)
    nrm = z.square().sum(1).sqrt()
    n = z / torch.maximum(nrm, eps32)[:, None]
    eye = torch.eye(N, dtype=torch.bool)
    S = ((n @ n.T) / tau32).masked_fill(eye, -math.inf)
    S = torch.minimum(S, S.T)                              # the kernels compute S_rj and S_jr by the same instructions
    rows, pair = torch.arange(N), _pair(B)
    if variant == "naive_lse":
        lse = torch.logsumexp(S, 1)
        term = lse - S[rows, pair]
    else:
        M, jstar = S.max(1)
        E = (S - M[:, None]).exp()
        E[rows, jstar] = 0.0
        lp = E.sum(1).log1p()
        lse = M + lp
        term = (M - S[rows, pair]) + lp
    p = (S - lse[:, None]).exp()                           # p_rj
    c = 2 * p if variant == "one_sided" else p + p.T
    if variant == "one_sided":
        c[rows, pair] = 2 * torch.expm1(-term)
    elif variant != "exp_exp_2":
        c[rows, pair] = torch.expm1(-term) + torch.expm1(-term[pair])
    else:
        c[rows, pair] = c[rows, pair] - 2
    c = c.masked_fill(eye, 0.0)
    dn = torch.tensor(g, dtype=f) / (torch.tensor(float(B), dtype=f) * tau32) * (c @ n)
    dot = (n * dn).sum(1)
    dz = torch.where((nrm >= eps32)[:, None], (dn - n * dot[:, None]) / nrm[:, None], dn / eps32)
    return dict(term=term, lse=lse, loss=term.sum() / torch.tensor(float(B), dtype=f), dz=dz, n=n)
