"""Inputs, float64 reference, float32 yardstick and the relative checker for the attention maps of
csrc/attention_probs.hip (P = softmax(q k^T), fp32 [B, H, T, T]).  Plain numpy: tests/test_attention_maps_host.py proves
on the CPU that the checker tells a subtly wrong map from a right one, tests/test_gpu_attention_maps.py holds the three
kernel variants (fp32, bf16 natural q, bf16 log2-unit q) to it.

Every input is bf16-valued fp32, so the three variants read the same numbers, every q k product is exact in fp32 and one
float64 reference serves the fp32 and the bf16 natural-q kernel.  The log2-unit buffer stores bf16(q log2 e); its
reference is that stored q divided by log2 e in float64."""
import functools

import numpy as np

from .test_gpu_kernels import _bf, _to_log2q

LOG2E = 1.4426950408889634
FLOOR = 2.0 ** -100
VARIANTS = ("f32", "bf16", "log2q")          # kernel variants; the first two share the natural-q reference

OFFSETS = {"offset+12": 12.0, "offset-12": -12.0, "offset+100": 100.0, "offset-100": -100.0}

# (kind, B, T, H): the grid of the GPU test.  T around the 32-key tile and the 128-row query tile, several blocks and
# batches, H = 20 (row stride 3840 elements), T = 1500 (the product shape).  The staircases stay at T <= 196: beyond
# that most of a row underflows against its maximum and the case stops comparing anything.
GRID = (
    [("bland", 1, t, 1) for t in (4, 28, 32, 36, 64, 124, 128, 132)]
    + [("bland", 2, 260, 3), ("bland", 3, 36, 20), ("bland", 1, 1500, 2)]
    + [("peaked", 1, 132, 1), ("peaked", 2, 260, 3), ("peaked", 1, 36, 20), ("peaked", 1, 1500, 2)]
    + [(k, 1, 132, 2) for k in OFFSETS]
    + [(k, b, t, h) for k in ("spike_lo", "spike_hi") for (b, t, h) in ((1, 132, 1), (1, 260, 3))]
    + [(k, b, t, h) for k in ("stair_up", "stair_down") for (b, t, h) in ((1, 132, 1), (1, 196, 3))]
    + [("equal_keys", 1, 36, 1), ("equal_keys", 1, 132, 2)]
)
HOST_GRID = [c for c in GRID if c[2] != 1500]


def case_id(case):
    return "%s-%d-%d-%d" % case


def case_seed(kind, B, T, H):
    """``bland`` at (2, 200, 2) is then exactly tests/test_gpu_memory_contract.py::test_attention_probs's input."""
    return B * 100 + T + H


def spike_key(kind, T):
    """The hot key of a spike case: near 3T/4, in the half of the lane pair the kind names.  Lane half hh of the kernel
    owns the keys with (j % 8) // 4 == hh."""
    j = 3 * T // 4
    if kind == "spike_lo" and j % 8 >= 4:
        j -= 4
    if kind == "spike_hi" and j % 8 < 4:
        j += 4
    assert 0 <= j < T
    return j


def make_case(kind, B, T, H, seed):
    """bf16-valued fp32 qkv [B, T, 3 H 64] with q in natural units (pre-scaled, as the kernels expect)."""
    rng = np.random.default_rng(seed)
    d = H * 64
    shape = (B, T, 3 * d)
    if kind == "bland":
        qkv = rng.standard_normal(shape) * 0.3
    elif kind == "peaked":
        qkv = rng.standard_normal(shape) * 1.2
    elif kind in OFFSETS:
        qkv = rng.standard_normal(shape) * 0.4
        qkv[:, :, 0] = 1.0                      # q[:, 0] = 1 in head 0 ...
        qkv[:, :, d] = OFFSETS[kind]            # ... and k[:, 0] = offset: every score of head 0 moves by it
    elif kind in ("spike_lo", "spike_hi"):
        qkv = rng.standard_normal(shape) * 0.3
        qkv[:, min(17, T - 1), :64] = 2.0                   # one query of head 0 ...
        qkv[:, spike_key(kind, T), d:d + 64] = 2.0          # ... and one key: score 256
        qkv[:, T // 2, :64] = -3.0                          # a query whose score against that key is -384
    elif kind in ("stair_up", "stair_down"):
        qkv = rng.standard_normal(shape) * 0.2
        qkv[:, :, 0] = 1.0
        qkv[:, :, d] = (14.0 if kind == "stair_up" else -14.0) * (np.arange(T) // 32)   # per 32-key tile of pass 1
    elif kind == "equal_keys":
        qkv = rng.standard_normal(shape) * 0.3
        qkv[:, :, d:2 * d] = qkv[:, :1, d:2 * d]
    else:
        raise KeyError(kind)
    return _bf(qkv.astype(np.float32))


def to_log2q(qkv):
    return _to_log2q(qkv)


def _heads(a, H, dtype):
    B, T, d = a.shape
    return a.reshape(B, T, H, 64).transpose(0, 2, 1, 3).astype(dtype)


def reference(qkv, H, q_log2=False):
    """float64 (scores, P): scores [B, H, T, T] in natural units, P = softmax over the keys."""
    d = H * 64
    q, k = _heads(qkv[..., :d], H, np.float64), _heads(qkv[..., d:2 * d], H, np.float64)
    if q_log2:
        q = q / LOG2E
    s = q @ k.transpose(0, 1, 3, 2)
    p = np.exp(s - s.max(-1, keepdims=True))
    return s, p / p.sum(-1, keepdims=True)


def softmax64(s):
    p = np.exp(s - s.max(-1, keepdims=True))
    return p / p.sum(-1, keepdims=True)


def restatement32(qkv, H, q_log2=False):
    """The same map in numpy float32 throughout: matmul, max, subtraction, exp, sum, division.  With q in log2 units
    the scores stay in those units and the exponential is exp2, as the kernel documents for itself.  This is the
    yardstick for what fp32 arithmetic costs on a case, not a model of the kernel."""
    d = H * 64
    q, k = _heads(qkv[..., :d], H, np.float32), _heads(qkv[..., d:2 * d], H, np.float32)
    s = np.matmul(q, k.transpose(0, 1, 3, 2))
    assert s.dtype == np.float32
    x = s - s.max(-1, keepdims=True)
    p = np.exp2(x) if q_log2 else np.exp(x)
    p = p / p.sum(-1, keepdims=True, dtype=np.float32)
    assert p.dtype == np.float32
    return p


def worst_rel(got, ref, floor=FLOOR):
    """max |got - ref| / ref over the entries with ref >= floor"""
    hi = ref >= floor
    return float((np.abs(np.asarray(got, np.float64) - ref)[hi] / ref[hi]).max())


def tolerance(qkv, H, q_log2, ref):
    """(tol, e32): tol = 8 e32 + 2^-20, e32 = the worst relative error of restatement32 against ref on this case.
    Three doublings over the yardstick: the MFMA's accumulation order is not numpy's, v_exp_f32 is a 1-ulp instruction
    where numpy's exp is better, and the bf16 path multiplies the exponent by log2 e in fp32."""
    e32 = worst_rel(restatement32(qkv, H, q_log2), ref)
    return 8.0 * e32 + 2.0 ** -20, e32


def check(got, ref, tol, floor=FLOOR):
    """got against the float64 map ref; returns the worst relative error, raises AssertionError naming (b, h, i, j).
    ref >= floor: |got - ref| <= tol ref.  ref < floor: 0 <= got <= 2 floor (the bf16 kernels flush results below
    2^-126 to zero, so a zero is right there).  Everything finite and >= 0, every row sums to 1 within 1e-5."""
    got = np.asarray(got, np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)

    def fail(bad, what):
        at = tuple(int(v) for v in np.unravel_index(int(np.argmax(bad)), bad.shape))
        raise AssertionError(f"{what} at (b, h, i, j) = {at}: got {got[at]!r}, reference {ref[at]!r}, tol {tol:.3e}")

    bad = ~np.isfinite(got)
    if bad.any():
        fail(bad, "not finite")
    if (got < 0).any():
        fail(got < 0, "negative probability")
    hi = ref >= floor
    rel = np.where(hi, np.abs(got - ref) / np.where(hi, ref, 1.0), 0.0)
    worst = float(rel.max())
    if worst > tol:
        fail(rel, f"relative error {worst:.3e}")
    lo_bad = ~hi & (got > 2.0 * floor)
    if lo_bad.any():
        fail(lo_bad, "above 2 floor where the reference is below the floor")
    rows = np.abs(got.sum(-1) - 1.0)
    if float(rows.max()) >= 1e-5:
        at = tuple(int(v) for v in np.unravel_index(int(np.argmax(rows)), rows.shape))
        raise AssertionError(f"row (b, h, i) = {at} sums to 1 {rows[at]:+.3e}")
    return worst


def check_conditions(kind, ref, tol, floor=FLOOR):
    """What keeps a case worth running: tol < 1e-3 (a quarter of the 3.9e-3 that rounding P to bf16 produces), at least
    85 % of the entries compared relatively, and a row with max p > 0.99 in every peaked and spike case."""
    assert tol < 1e-3, tol
    frac = float((ref >= floor).mean())
    assert frac >= 0.85, frac
    if kind == "peaked" or kind.startswith("spike"):
        assert float(ref.max()) > 0.99, float(ref.max())


@functools.lru_cache(maxsize=2)
def case_data(case):
    """Per variant: the input buffer, the float64 map and (tol, e32), computed once per case and left unchanged."""
    kind, B, T, H = case
    qkv = make_case(kind, B, T, H, case_seed(*case))
    ql2 = to_log2q(qkv)
    nat = {"qkv": qkv, "ref": reference(qkv, H, False)[1]}
    nat["tol"], nat["e32"] = tolerance(qkv, H, False, nat["ref"])
    l2 = {"qkv": ql2, "ref": reference(ql2, H, True)[1]}
    l2["tol"], l2["e32"] = tolerance(ql2, H, True, l2["ref"])
    for v in (nat, l2):
        v["qkv"].setflags(write=False)
        v["ref"].setflags(write=False)
    return {"f32": nat, "bf16": nat, "log2q": l2}
