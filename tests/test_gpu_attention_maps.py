"""The attention-map kernel (csrc/attention_probs.hip, ops.attention_probs) entry by entry, relatively, against float64:
all three variants (fp32, bf16 natural q, bf16 log2-unit q) on bland, peaked, uniformly shifted, spiked, staircase and
equal-key rows, at T around the 32-key and the 128-row tile, several blocks, H = 20 and T = 1500; P @ V against the
forward kernels' context; bit-identical repeats; refusals and the empty batch.  Needs an MI355X.

tests/attention_maps_helpers.py holds the inputs, the reference and the checker, tests/test_attention_maps_host.py
shows on the CPU which defects that checker rejects."""

import numpy as np
import pytest

from . import attention_maps_helpers as mh

pytestmark = pytest.mark.gpu

# Bounds.  Per case and reference, tol = 8 e32 + 2^-20, where e32 is the worst relative error of a plain numpy float32
# restatement of the map against float64 on that case (attention_maps_helpers.tolerance); asserted below 1e-3.
# Measured maxima on an MI355X (-s prints every case): the worst relative error over the entries >= 2^-100 and over the
# kind's shapes, fp32 / bf16 natural q / bf16 log2-unit q, next to the largest yardstick e32 (natural / log2-unit q)
# of those shapes and the bounds it gave:
#   bland:       1.2e-6 / 9.1e-7 / 9.6e-7   e32 7.8e-7 / 9.6e-7   -> 7.2e-6 / 8.6e-6   (T = 1500)
#   peaked:      1.8e-5 / 1.4e-5 / 1.1e-5   e32 1.4e-5 / 1.4e-5   -> 1.2e-4 / 1.1e-4   (T = 1500)
#   offset+-12:  5.8e-6 / 3.1e-6 / 4.4e-6   e32 4.6e-6 / 6.8e-6   -> 3.8e-5 / 5.5e-5
#   offset+-100: 6.0e-5 / 3.0e-5 / 3.9e-5   e32 6.0e-5 / 9.5e-5   -> 4.8e-4 / 7.6e-4
#   spike:       1.4e-6 / 3.6e-6 / 2.3e-6   e32 2.0e-6 / 2.3e-6   -> 1.7e-5 / 1.9e-5   (T = 260, either lane half)
#   stair_up:    7.9e-5 / 3.1e-5 / 2.3e-5   e32 7.4e-5 / 6.0e-5   -> 5.9e-4 / 4.8e-4   (T = 196)
#   stair_down:  3.2e-5 / 1.7e-5 / 1.7e-5   e32 3.5e-5 / 4.5e-5   -> 2.8e-4 / 3.6e-4
#   equal_keys:  3.0e-8 / 3.0e-8 / 3.0e-8   e32 3.0e-8 / 3.0e-8   -> 1.2e-6 / 1.2e-6   (fp32(1 / T) exactly)
# No case is further than 1.95x from its yardstick (spike, T = 260, bf16 natural q: 3.63e-6 against 1.87e-6).
# A trial build whose bf16 scores were 0.2 % too large failed 27 of the 29 cases below (all but equal_keys, which no
# score scale changes) and passed every absolute-bound map test of test_gpu_encoder_outputs.py and
# test_gpu_memory_contract.py.
#   P V against the forward's ctx (max |difference|, max |ctx|; natural / log2-unit q), bound 6e-3 + 2^-7 |P V|:
#   bland 3.9e-4 / 3.9e-4 on 0.11, peaked 1.6e-2 / 1.9e-2 on 5.4, spike 2.0e-3 / 2.7e-3 on 1.1


@pytest.fixture(scope="module")
def T():
    import torch
    assert torch.cuda.is_available()
    return torch


def _run(T, variant, qkv, H):
    from gw_whisper_amd import ops
    x = T.from_numpy(np.array(qkv)).cuda()
    if variant != "f32":
        x = x.bfloat16()
    return ops.attention_probs(x, H, q_log2=(variant == "log2q"))


# ----------------------------------------------------------------------------------- 1. every entry, relatively
@pytest.mark.parametrize("case", [pytest.param(c, id=mh.case_id(c)) for c in mh.GRID])
def test_maps_against_fp64(T, gww, case):
    kind, B, Tn, H = case
    data = mh.case_data(case)
    got = {v: _run(T, v, data[v]["qkv"], H) for v in mh.VARIANTS}
    failures = []
    for v in mh.VARIANTS:
        d = data[v]
        mh.check_conditions(kind, d["ref"], d["tol"])
        assert got[v].shape == (B, H, Tn, Tn) and got[v].dtype == T.float32
        g = got[v].cpu().numpy()
        print(f"{mh.case_id(case)} {v}: worst rel {mh.worst_rel(g, d['ref']):.2e}  e32 {d['e32']:.2e}  tol {d['tol']:.2e}")
        try:
            mh.check(g, d["ref"], d["tol"])
        except AssertionError as e:
            failures.append(f"{v}: {e}")
    assert not failures, "\n".join(failures)


# ------------------------------------------------------------------------- 2. the maps are the forward's own P
@pytest.mark.parametrize("case", [("bland", 2, 260, 3), ("peaked", 2, 260, 3), ("spike_lo", 2, 260, 3),
                                  ("peaked", 1, 1500, 2)], ids=mh.case_id)
def test_p_times_v_is_the_forward_context(T, gww, case):
    """attentions[l] is read as "the P that produced this layer's context": the kernel's bf16 map times the V section
    (float64) against gww_attention_bf16's ctx on the same buffer, the log2-unit map against gww_attention_log2q_bf16's.
    The bound is the forward tests' own (test_gpu_kernels.py::test_attention_bf16, ::test_attention_log2q)."""
    from gw_whisper_amd import ops
    kind, B, Tn, H = case
    data = mh.case_data(case)
    d = H * 64
    for v, fwd in (("bf16", ops.attention), ("log2q", ops.attention_log2q)):
        qkv = data[v]["qkv"]
        P = _run(T, v, qkv, H).cpu().numpy().astype(np.float64)
        V = qkv[..., 2 * d:].reshape(B, Tn, H, 64).transpose(0, 2, 1, 3).astype(np.float64)
        want = (P @ V).transpose(0, 2, 1, 3).reshape(B, Tn, d)
        ctx = fwd(T.from_numpy(np.array(qkv)).cuda().bfloat16(), H).float().cpu().numpy()
        print(f"{mh.case_id(case)} {v}: max |P V - ctx| {np.abs(want - ctx).max():.2e}, max |ctx| {np.abs(ctx).max():.2f}")
        np.testing.assert_allclose(ctx, want, atol=6e-3, rtol=2 ** -7)


# -------------------------------------------------------------------------------------------- 3. determinism
@pytest.mark.parametrize("variant", mh.VARIANTS)
def test_two_calls_give_identical_bits(T, gww, variant):
    case = ("peaked", 2, 260, 3)
    qkv = mh.case_data(case)[variant]["qkv"]
    a, b = _run(T, variant, qkv, 3), _run(T, variant, qkv, 3)
    assert T.equal(a, b)


# ------------------------------------------------------------------------------ 4. refusals and the empty batch
@pytest.mark.parametrize("variant", mh.VARIANTS)
@pytest.mark.parametrize("Tn", [6, 130])
def test_t_not_a_multiple_of_4_is_refused(T, gww, variant, Tn):
    qkv = np.zeros((1, Tn, 3 * 2 * 64), np.float32)
    with pytest.raises(gww.GwwError, match="multiple of 4"):
        _run(T, variant, qkv, 2)


def test_wrong_width_and_log2_fp32_are_refused(T, gww):
    from gw_whisper_amd import ops
    with pytest.raises(gww.GwwError, match="n_heads"):
        ops.attention_probs(T.zeros((1, 8, 3 * 64), device="cuda"), 2)
    with pytest.raises(gww.GwwError, match="log2"):
        ops.attention_probs(T.zeros((1, 8, 3 * 64), device="cuda"), 1, q_log2=True)


@pytest.mark.parametrize("variant", mh.VARIANTS)
def test_empty_batch(T, gww, variant):
    out = _run(T, variant, np.zeros((0, 36, 3 * 3 * 64), np.float32), 3)
    assert out.shape == (0, 3, 36, 36) and out.dtype == T.float32
