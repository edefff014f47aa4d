"""The out_proj GEMM in front of the fused block walks k-tile major and starts on the first sixth of ctx and the first third of
x; the other requests ride between its ring pieces or land under its first two tiles (csrc/mlp_fused.hip: CSP / XPR,
DESIGN.md section 27; needs an MI355X, -m gpu).

Every comparison is exact (``torch.equal`` on integer views).  Two kinds of reference, both computed in the test:

* ``exact``: ctx, W_o, bo and x hold small integers, so ``x + ctx W_o^T (+ bo)`` has ONE value whatever the order of the sum
  (every partial sum is an integer below 2^24 in fp32 and below 2^8 where it is rounded to bf16).  The block on (x, ctx) must
  then return bit for bit what it returns on (x + ctx W_o^T, 0): a fragment of ctx that is read before it has landed, a k-tile
  that meets the wrong tile of W_o or an accumulator tile that starts from something other than its x shows here, on every
  row.  The rows M = 1 .. 129 are ragged single panels and the panel boundary; M = 1500 is twelve panels, the last ragged.
* ``forms``: the layer-0 instantiation with its flag cleared reads the same x but keeps all of x in front of the GEMM: it must
  agree with the plain instantiation bit for bit on seeded normal data.
"""

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

D, F, NQ = 384, 1536, 1152
MS = [1, 31, 32, 33, 127, 128, 129, 1500]


@pytest.fixture(scope="module")
def T():
    import torch
    assert torch.cuda.is_available()
    return torch


def _bits_equal(T, a, b):
    a, b = a.contiguous(), b.contiguous()
    v = T.int16 if a.dtype == T.bfloat16 else T.int32
    return a.shape == b.shape and a.dtype == b.dtype and T.equal(a.view(v), b.view(v))


_OPS = {}


def _operands(T, M):
    """Integer-valued x, ctx, W_o, bo (a quarter of the products non-zero: |ctx W_o^T + bo| stays below 2^8, asserted) and seeded
    normal weights for the rest of the block, folded once per M."""
    if M in _OPS:
        return _OPS[M]
    from gw_whisper_amd import ops
    from tests.test_gpu_memory_contract import _block
    _, d = _block(T, M, 9100 + M)
    rng = np.random.default_rng(9200 + M)
    tern = lambda shape: rng.integers(-1, 2, size=shape) * rng.integers(0, 2, size=shape)
    ctx, wo = tern((M, D)), tern((D, D))
    # every k-tile of every row carries weight: a k-tile dropped or taken twice moves the sum
    ctx[:, ::64] = 1
    wo[:, ::64] = np.where(wo[:, ::64] == 0, 1, wo[:, ::64])
    x = rng.integers(-40, 41, size=(M, D))
    bo = rng.integers(-3, 4, size=D)
    prod = ctx @ wo.T
    assert np.abs(prod + bo).max() < 256 and np.abs(x + prod).max() < 2 ** 20
    f32 = lambda a: T.from_numpy(a.astype(np.float32)).cuda()
    d.update(x=f32(x), ctx=f32(ctx).bfloat16(), wo=f32(wo).bfloat16(), bo=f32(bo), xw=f32(x + prod), x_mid=f32(x + prod + bo),
             zero=T.zeros((M, D), dtype=T.bfloat16, device="cuda"))
    d["w1f"], d["u"], d["cb"] = ops.ln_fold_weights(d["w1"], d["lw"], d["lb"], d["b1"])
    d["wqf"], d["uq"], d["cq"] = ops.ln_fold_weights(d["wq"], d["lw1"], d["lb1"], d["bq"])
    _OPS[M] = d
    return d


def _mlp(w):
    return w["wo"], w["bo"], w["w1f"], w["w2"], w["u"], w["cb"], w["b2"]


@pytest.mark.parametrize("M", MS)
def test_exact_block_with_qkv_tail(T, M):
    """k_mlp_fused<1, true>: q / k / v of the next layer and x_next on (x, ctx) against (x + ctx W_o^T, 0)."""
    from gw_whisper_amd import ops
    w = _operands(T, M)
    tail = (w["wqf"], w["uq"], w["cq"])
    q_got, x_got = ops.attn_out_mlp_fused(w["x"], w["ctx"], *_mlp(w), qkv=tail)
    q_ref, x_ref = ops.attn_out_mlp_fused(w["xw"], w["zero"], *_mlp(w), qkv=tail)
    assert bool(T.isfinite(x_got).all())
    assert _bits_equal(T, x_got, x_ref), f"M = {M}: x_next differs in {int((x_got != x_ref).any(1).sum())} rows"
    assert _bits_equal(T, q_got, q_ref), f"M = {M}: the q / k / v tail differs"


@pytest.mark.parametrize("M", MS)
def test_exact_last_block(T, M):
    """k_mlp_fused<3, true>: x_mid is the exact sum itself; last_hidden_state on (x, ctx) against (x + ctx W_o^T, 0)."""
    from gw_whisper_amd import ops
    w = _operands(T, M)
    y_got, mid_got = ops.attn_out_mlp_final(w["x"], w["ctx"], *_mlp(w), w["lw1"], w["lb1"])
    y_ref, mid_ref = ops.attn_out_mlp_final(w["xw"], w["zero"], *_mlp(w), w["lw1"], w["lb1"])
    assert _bits_equal(T, mid_got, w["x_mid"]), f"M = {M}: x_mid is not x + ctx W_o^T + bo in {int((mid_got != w['x_mid']).any(1).sum())} rows"
    assert _bits_equal(T, mid_ref, w["x_mid"])
    assert _bits_equal(T, y_got, y_ref), f"M = {M}: last_hidden_state differs"


@pytest.mark.parametrize("M", MS)
def test_exact_row_order_block(T, M):
    """k_mlp_fused<0, true> (the row-order seam, x_new = x + bf16(ctx W_o^T + bo)) takes the same k-tile major stream: x_new is
    the exact sum, the block's output the one of (x + ctx W_o^T, 0)."""
    from gw_whisper_amd import ops
    w = _operands(T, M)
    c_got, new_got = ops.attn_out_mlp_fused(w["x"], w["ctx"], *_mlp(w))
    c_ref, new_ref = ops.attn_out_mlp_fused(w["xw"], w["zero"], *_mlp(w))
    assert _bits_equal(T, new_got, w["x_mid"]), f"M = {M}: x_new is not x + ctx W_o^T + bo"
    assert _bits_equal(T, new_ref, w["x_mid"])
    assert _bits_equal(T, c_got, c_ref), f"M = {M}: the block's output differs"


# B segments of Tn tokens, M = B * Tn rows (the layer-0 entry point takes whole segments of at least one panel): one and two
# panels with a ragged second, and twelve panels that straddle three segments
@pytest.mark.parametrize("B,Tn", [(1, 128), (1, 129), (3, 500)])
def test_forms_agree(T, B, Tn):
    """The plain instantiation (x n-tiles 1 and 2 land under the GEMM) against the layer-0 one with its flag cleared (all of x in
    front of the GEMM), on seeded normal operands."""
    from gw_whisper_amd import ops
    from tests.test_gpu_memory_contract import _block
    M = B * Tn
    _, d = _block(T, M, 9300 + M)
    w1f, u, cb = ops.ln_fold_weights(d["w1"], d["lw"], d["lb"], d["b1"])
    tail = ops.ln_fold_weights(d["wq"], d["lw1"], d["lb1"], d["bq"])
    nan = lambda *s: T.full(s, float("nan"), dtype=T.float32, device="cuda")
    flag0 = T.zeros((1,), dtype=T.int32, device="cuda")
    q_ref, x_ref = ops.attn_out_mlp_fused(d["x"], d["ctx"], d["wo"], d["bo"], w1f, d["w2"], u, cb, d["b2"], qkv=tail)
    q_got, x_got = ops.attn_out_mlp_fused_x0(nan(B, 64, D), nan(B, D), nan(Tn, D), flag0, d["ctx"], d["wo"], d["bo"], w1f, d["w2"], u,
                                             cb, d["b2"], tail, x=d["x"])
    assert bool(T.isfinite(x_ref).all())
    assert _bits_equal(T, x_got, x_ref) and _bits_equal(T, q_got, q_ref), f"B = {B}, T = {Tn}: the two instantiations differ"
