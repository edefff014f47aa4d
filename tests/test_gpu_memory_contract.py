"""Memory contract of every entry point of include/gww.h that takes a device buffer (needs an MI355X, -m gpu).

Each case runs its op four times -- on plain tensors, then under tests/guard.py's guard-band allocator with the bands and
every ``empty`` interior filled with 0xFF (NaN), 0x7F (3.39e38) and 0x00 -- with the inputs ``place``d in guarded blocks
of exactly their documented size.  After each guarded run every band must still hold its fill (no stray store), every
output the case inspects must come from the guard and hold no leftover fill (no missing store); the documented extent of
every output must be finite and bit-identical across the four runs (nothing depends on bytes outside the contract).
Where the fp64 reference of the op is a line or two it is compared too, at exactly the tolerance the existing test of that
op asserts (named in a comment): "identical and finite" alone could be met by a constant.  No tolerance is new here.

The few kernels that sum with float atomics (``gww_dora_grads``, the d = 128 DoRA training step, the Q-adapter CNN's
weight gradients) differ from run to run in their last bits by design; they are compared at the run-to-run bound their
own tests assert, which a NaN or a 3.39e38 leaking in still fails.

Nothing here launches a kernel with less memory than the library asks for: the bands live inside allocations the test
owns, and the undersized-workspace cases stop at the host check (GWW_ERR_WORKSPACE) before any launch.  That these checks
can fail is shown on the CPU, by tests/test_guard_host.py."""

import ctypes as C
import math

import numpy as np
import pytest

from gw_whisper_amd import synth
from oracle import dora as odora
from oracle import encoder as oenc
from oracle import logmel as olm
from tests.guard import FILLS, Guard, encoder_arena_row_bytes, run_contract

pytestmark = pytest.mark.gpu

LOG2E = 1.4426950408889634


@pytest.fixture(scope="module")
def T():
    import torch
    assert torch.cuda.is_available()
    return torch


def _bf(x):
    return oenc.bf16_round(np.asarray(x, np.float32))


def _dev(T, a, dtype=None):
    t = T.from_numpy(np.ascontiguousarray(a)).cuda()
    return t.to(dtype) if dtype is not None else t


def _stream(T):
    return T.cuda.current_stream().cuda_stream


def _ok(rc, what):
    from gw_whisper_amd._lib import check
    check(rc, what)


# ------------------------------------------------------------------ GEMMs
# shapes of test_gpu_kernels.py::test_gemm_bf16 (smallest, ragged, the v2 and v4 kernels) + M one past a 256-row tile
@pytest.mark.parametrize("M,N,K", [(128, 128, 64), (300, 384, 384), (1501, 1152, 384), (257, 128, 128), (64, 1536, 384),
                                   (4096, 384, 384), (256, 256, 128), (512, 512, 256)])
@pytest.mark.parametrize("epi", [0, 1, 2])
def test_gemm_bf16(T, gww, M, N, K, epi):
    from gw_whisper_amd import ops
    rng = np.random.default_rng(M * 7 + N + K + epi)
    a = _bf(rng.standard_normal((M, K)))
    w = _bf(rng.standard_normal((N, K)) / np.sqrt(K))
    bias = rng.standard_normal(N).astype(np.float32)
    resid = rng.standard_normal((M, N)).astype(np.float32)
    ad, wd, bd, rd = _dev(T, a, T.bfloat16), _dev(T, w, T.bfloat16), _dev(T, bias), _dev(T, resid)

    def case(g):
        return {"c": ops.gemm(g.place(ad), g.place(wd), g.place(bd), epilogue=epi, resid=g.place(rd) if epi == 2 else None)}
    got = run_contract(case)["c"].float().cpu().numpy()
    ref = a.astype(np.float64) @ w.astype(np.float64).T + bias
    ref = oenc.gelu(ref) if epi == 1 else ref + resid if epi == 2 else ref
    # tolerances of test_gpu_kernels.py::test_gemm_bf16
    if epi == 2:
        np.testing.assert_allclose(got, ref, atol=2e-5 * np.sqrt(K), rtol=1e-5)
    else:
        np.testing.assert_allclose(got, ref, atol=1e-5 * np.sqrt(K), rtol=2 ** -8)


@pytest.mark.parametrize("M,N,K", [(256, 256, 128), (512, 512, 256), (2560, 3072, 128)])
@pytest.mark.parametrize("epi", [0, 1, 2])
def test_gemm_v4_split(T, gww, M, N, K, epi):
    """gww_gemm_bf16_v4_split with the automatic split, one tile per item and all tiles in one item."""
    from gw_whisper_amd import ops
    rng = np.random.default_rng(M + N + K + epi)
    a = _bf(rng.standard_normal((M, K)))
    w = _bf(rng.standard_normal((N, K)) / np.sqrt(K))
    bias = rng.standard_normal(N).astype(np.float32)
    resid = rng.standard_normal((M, N)).astype(np.float32)
    ad, wd, bd, rd = _dev(T, a, T.bfloat16), _dev(T, w, T.bfloat16), _dev(T, bias), _dev(T, resid)

    def case(g):
        pa, pw, pb, pr = g.place(ad), g.place(wd), g.place(bd), g.place(rd) if epi == 2 else None
        return {f"split{s}": ops.gemm_v4_split(pa, pw, pb, epilogue=epi, resid=pr, n_split=s) for s in (0, 1, N // 256)}
    r = run_contract(case)
    assert T.equal(r["split0"], r["split1"]) and T.equal(r["split0"], r[f"split{N // 256}"])
    ref = a.astype(np.float64) @ w.astype(np.float64).T + bias
    ref = oenc.gelu(ref) if epi == 1 else ref + resid if epi == 2 else ref
    # tolerances of test_gpu_kernels.py::test_gemm_v4_result_does_not_depend_on_the_column_split
    tol = dict(atol=2e-5 * np.sqrt(K), rtol=1e-5) if epi == 2 else dict(atol=1e-5 * np.sqrt(K), rtol=2 ** -8)
    np.testing.assert_allclose(r["split0"].float().cpu().numpy(), ref, **tol)


@pytest.mark.parametrize("M,N,K", [(64, 64, 32), (300, 384, 384), (1501, 128, 96), (1, 64, 32)])
@pytest.mark.parametrize("epi", [0, 1, 2])
def test_gemm_f32(T, gww, M, N, K, epi):
    from gw_whisper_amd import ops
    rng = np.random.default_rng(M + N + K + epi)
    a = rng.standard_normal((M, K)).astype(np.float32)
    w = (rng.standard_normal((N, K)) / np.sqrt(K)).astype(np.float32)
    bias = rng.standard_normal(N).astype(np.float32)
    resid = rng.standard_normal((M, N)).astype(np.float32)
    ad, wd, bd, rd = _dev(T, a), _dev(T, w), _dev(T, bias), _dev(T, resid)

    def case(g):
        return {"c": ops.gemm(g.place(ad), g.place(wd), g.place(bd), epilogue=epi, resid=g.place(rd) if epi == 2 else None)}
    got = run_contract(case)["c"].cpu().numpy()
    ref = a.astype(np.float64) @ w.astype(np.float64).T + bias
    ref = oenc.gelu(ref) if epi == 1 else ref + resid if epi == 2 else ref
    np.testing.assert_allclose(got, ref, atol=3e-6 * np.sqrt(K), rtol=1e-5)     # test_gpu_kernels.py::test_gemm_f32


@pytest.mark.parametrize("M,N,K", [(1, 128, 384), (256, 128, 384), (257, 128, 384), (777, 1536, 384), (512, 256, 256),
                                   (300, 512, 512)])
@pytest.mark.parametrize("epi", [0, 1])
def test_gemm_astat(T, gww, M, N, K, epi):
    """C is allocated up to the next multiple of 256 rows (the wrapper does what the header says): whole panels are stored,
    rows >= M are scratch, nothing lies beyond the padded rows."""
    from gw_whisper_amd import ops
    rng = np.random.default_rng(M * 3 + N + K + epi)
    a = _bf(rng.standard_normal((M, K)))
    w = _bf(rng.standard_normal((N, K)) / np.sqrt(K))
    bias = rng.standard_normal(N).astype(np.float32)
    ad, wd, bd = _dev(T, a, T.bfloat16), _dev(T, w, T.bfloat16), _dev(T, bias)

    def case(g):
        return {"c": ops.gemm_astat(g.place(ad), g.place(wd), g.place(bd), epilogue=epi)}
    got = run_contract(case)["c"].float().cpu().numpy()
    assert got.shape == (M, N)
    ref = a.astype(np.float64) @ w.astype(np.float64).T + bias
    ref = oenc.gelu(ref) if epi == 1 else ref
    np.testing.assert_allclose(got, ref, atol=1e-5 * np.sqrt(K), rtol=2 ** -8)   # test_gpu_kernels.py::test_gemm_astat_bf16


@pytest.mark.parametrize("M,N,K", [(256, 1152, 384), (257, 1152, 384), (1500, 1536, 384), (700, 512, 512)])
@pytest.mark.parametrize("epi", [0, 1])
@pytest.mark.parametrize("with_delta", [False, True])
def test_gemm_astat_fused_layernorm_and_ln_fold_weights(T, gww, M, N, K, epi, with_delta):
    """The LN-fused form: x and delta are exact-size [M, K] buffers (their rows >= M do not exist), x_out likewise."""
    from gw_whisper_amd import ops
    rng = np.random.default_rng(M + N + K + epi)
    x = (rng.standard_normal((M, K)) * 2 + 0.3).astype(np.float32)
    x[::7] += 25.0
    dl = _bf(rng.standard_normal((M, K)) * 0.5) if with_delta else None
    lw = (1 + 0.1 * rng.standard_normal(K)).astype(np.float32)
    lb = (0.1 * rng.standard_normal(K)).astype(np.float32)
    w = (rng.standard_normal((N, K)) / np.sqrt(K)).astype(np.float32)
    bias = rng.standard_normal(N).astype(np.float32)
    xd, wd, lwd, lbd, bd = (_dev(T, t) for t in (x, w, lw, lb, bias))
    dd = _dev(T, dl, T.bfloat16) if with_delta else None

    def case(g):
        wf, u, cb = ops.ln_fold_weights(g.place(wd), g.place(lwd), g.place(lbd), g.place(bd))
        px = g.place(xd)
        c, x_new = ops.gemm_astat(px, wf, None, epilogue=epi, ln=(u, cb), delta=g.place(dd) if with_delta else None,
                                  return_x=True)
        assert T.equal(px, xd), "x is only read"
        return {"wf": wf, "u": u, "cb": cb, "c": c, "x_new": x_new}
    r = run_contract(case)
    xn = x + dl if with_delta else x
    # bounds of test_gpu_kernels.py::test_gemm_astat_fused_layernorm
    np.testing.assert_array_equal(r["wf"].float().cpu().numpy(), _bf(w * lw[None, :]))
    np.testing.assert_allclose(r["u"].cpu().numpy(), _bf(w * lw[None, :]).astype(np.float64).sum(1), rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(r["cb"].cpu().numpy(), bias + w.astype(np.float64) @ lb, rtol=1e-5, atol=1e-5)
    np.testing.assert_array_equal(r["x_new"].cpu().numpy(), xn.astype(np.float32))
    ref = oenc.layer_norm(xn.astype(np.float64), lw, lb) @ w.astype(np.float64).T + bias
    ref = oenc.gelu(ref) if epi == 1 else ref
    got = r["c"].float().cpu().numpy()
    np.testing.assert_allclose(got, ref, atol=3e-2, rtol=2 ** -7)
    assert np.sqrt(((got - ref) ** 2).mean()) < 6e-3


@pytest.mark.parametrize("inplace", [False, True], ids=["separate", "in_place"])
@pytest.mark.parametrize("M,N,K", [(1, 128, 384), (257, 128, 384), (777, 1536, 384), (3000, 128, 256), (777, 1536, 512)])
def test_gemm_astat_gelu_backward_epilogue(T, gww, M, N, K, inplace):
    """Epilogue 5.  Separate: delta is an exact-size [M, N] buffer ("delta rows >= M are never read" -- if they were, the
    NaN behind it would have to stay out of rows < M).  In place: C = delta, allocated to whole 256-row panels, the padded
    rows holding the fill."""
    from gw_whisper_amd import _lib, ops
    g_ = T.Generator().manual_seed(M + N + K)
    rb = lambda t: t.to(T.bfloat16).double()
    a = rb(T.randn((M, K), generator=g_, dtype=T.float64))
    w = rb(T.randn((N, K), generator=g_, dtype=T.float64) * (1.5 / math.sqrt(K)))
    bias = (T.randn(N, generator=g_, dtype=T.float64) * 0.3).float()
    gg = rb(T.randn((M, N), generator=g_, dtype=T.float64))
    Mp = (M + 255) // 256 * 256
    ad, wd, bd, gd = a.float().cuda().bfloat16(), w.float().cuda().bfloat16(), bias.cuda(), gg.float().cuda().bfloat16()

    def case(g):
        if inplace:
            buf = g.empty((Mp, N), T.bfloat16)
            buf[:M].copy_(gd)
            out = ops.gemm_astat(g.place(ad), g.place(wd), g.place(bd), epilogue=_lib.EPI_DGELU, delta=buf, out=buf)
            assert out.data_ptr() == buf.data_ptr()
        else:
            pg = g.place(gd)
            out = ops.gemm_astat(g.place(ad), g.place(wd), g.place(bd), epilogue=_lib.EPI_DGELU, delta=pg)
            assert T.equal(pg, gd), "the incoming gradient must not be written"
        return {"c": out[:M]}
    got = run_contract(case)["c"].cpu().double()
    z = a @ w.t() + bias.double()
    ref = gg * (0.5 * (1 + T.erf(z / math.sqrt(2))) + z * T.exp(-0.5 * z * z) / math.sqrt(2 * math.pi))
    # bound of test_gpu_backward_widths.py::test_gemm_astat_gelu_backward_epilogue
    err = (got - ref).abs()
    bound = 2 ** -7 * ref.abs() + 2e-5 * gg.abs() + 1e-30
    assert (err <= bound).all(), float((err / bound).max())


@pytest.mark.parametrize("M,N,K", [(128, 384, 64), (129, 384, 64), (1500, 384, 1536), (777, 384, 1152), (300, 512, 2048)])
@pytest.mark.parametrize("epi", [0, 1])
def test_gemm_fulln(T, gww, M, N, K, epi):
    from gw_whisper_amd import ops
    rng = np.random.default_rng(M * 5 + N + K + epi)
    a = _bf(rng.standard_normal((M, K)))
    w = _bf(rng.standard_normal((N, K)) / np.sqrt(K))
    bias = rng.standard_normal(N).astype(np.float32)
    ad, wd, bd = _dev(T, a, T.bfloat16), _dev(T, w, T.bfloat16), _dev(T, bias)

    def case(g):
        return {"c": ops.gemm_fulln(g.place(ad), g.place(wd), g.place(bd), epilogue=epi)}
    got = run_contract(case)["c"].float().cpu().numpy()
    ref = a.astype(np.float64) @ w.astype(np.float64).T + bias
    ref = oenc.gelu(ref) if epi == 1 else ref
    np.testing.assert_allclose(got, ref, atol=1e-5 * np.sqrt(K), rtol=2 ** -8)   # test_gpu_kernels.py::test_gemm_fulln_bf16


# ------------------------------------------------------------------ fused MLP block (d_model 384)
def _block(T, M, seed, F=1536, NQ=1152):
    """Operands of one block on the device (the construction of test_gpu_kernels.py::_block_operands)."""
    from tests.test_gpu_kernels import _block_operands
    o = _block_operands(np.random.default_rng(seed), M, F=F, NQ=NQ)
    o["dl"] = _bf(np.random.default_rng(seed + 1).standard_normal((M, 384)) * 0.5)
    bf = {"ctx", "wo", "w2", "dl"}
    return o, {k: _dev(T, v, T.bfloat16 if k in bf else None) for k, v in o.items()}


def _folded(T, ops, g, d):
    w1f, u, cb = ops.ln_fold_weights(g.place(d["w1"]), g.place(d["lw"]), g.place(d["lb"]), g.place(d["b1"]))
    wqf, uq, cq = ops.ln_fold_weights(g.place(d["wq"]), g.place(d["lw1"]), g.place(d["lb1"]), g.place(d["bq"]))
    return w1f, u, cb, wqf, uq, cq


def _mlp_ref(o):
    """fp64 x_new = x + delta and the MLP output of it (test_gpu_kernels.py::test_mlp_fused)."""
    xn = o["x"] + o["dl"]
    h = oenc.gelu(oenc.layer_norm(xn.astype(np.float64), o["lw"], o["lb"]) @ o["w1"].astype(np.float64).T + o["b1"])
    return xn, h @ o["w2"].astype(np.float64).T + o["b2"]


def _check_qkv(o, x_next, qkv):
    """q / k / v of the tail against LayerNorm_1(x_next) Wqkv^T + b: test_gpu_kernels.py::test_mlp_fused_with_next_layers_qkv."""
    ref = oenc.layer_norm(x_next.astype(np.float64), o["lw1"], o["lb1"]) @ o["wq"].astype(np.float64).T + o["bq"]
    np.testing.assert_allclose(qkv, ref, atol=3e-2, rtol=2 ** -7)
    assert np.sqrt(((qkv - ref) ** 2).mean()) < 6e-3


@pytest.mark.parametrize("M,F", [(128, 128), (129, 1536), (777, 512), (1500, 1536)])
def test_mlp_fused_and_mlp_pack(T, gww, M, F):
    from gw_whisper_amd import ops
    o, d = _block(T, M, M + F, F=F)

    def case(g):
        w1f, u, cb, _, _, _ = _folded(T, ops, g, d)
        wt = ops.mlp_pack(w1f, g.place(d["w2"]))
        px = g.place(d["x"])
        c, x_new = ops.mlp_fused(px, g.place(d["dl"]), wt, u, cb, g.place(d["b2"]))
        assert T.equal(px, d["x"]), "without the q / k / v tail x is only read"
        return {"wt": wt, "c": c, "x_new": x_new}
    r = run_contract(case)
    xn, ref = _mlp_ref(o)
    np.testing.assert_array_equal(r["x_new"].cpu().numpy(), xn.astype(np.float32))
    got = r["c"].float().cpu().numpy()
    np.testing.assert_allclose(got, ref, atol=4e-2, rtol=2 ** -7)          # test_gpu_kernels.py::test_mlp_fused
    assert np.sqrt(((got - ref) ** 2).mean()) < 8e-3


@pytest.mark.parametrize("M", [128, 129, 777, 1500])
def test_mlp_fused_qkv_tail_writes_x_next_over_x(T, gww, M):
    """With the tail the library writes x_next back over x and C is NULL.  The wrapper hands it a clone the proxy does not
    see, so the C entry point is called directly on a ``place``d, exact-size x: rows >= M of x and x_out do not exist and
    must not be written (their bands stay intact); qkv_out has its rows padded to 128."""
    from gw_whisper_amd import ops
    from gw_whisper_amd._lib import lib
    o, d = _block(T, M, M)
    NQ, F, Mp = 1152, 1536, (M + 127) // 128 * 128

    def case(g):
        w1f, u, cb, wqf, uq, cq = _folded(T, ops, g, d)
        wt = ops.mlp_pack(w1f, g.place(d["w2"]), wqf)
        px, pdl, pb2 = g.place(d["x"]), g.place(d["dl"]), g.place(d["b2"])
        x_out, qkv = g.empty((M, 384), T.float32), g.empty((Mp, NQ), T.bfloat16)
        _ok(lib().gww_mlp_fused_bf16(px.data_ptr(), pdl.data_ptr(), x_out.data_ptr(), u.data_ptr(), cb.data_ptr(),
                                     wt.data_ptr(), pb2.data_ptr(), None, M, 384, F, uq.data_ptr(), cq.data_ptr(),
                                     qkv.data_ptr(), NQ, _stream(T)), "gww_mlp_fused_bf16")
        return {"wt": wt, "x_next": px, "x_out": x_out, "qkv": qkv[:M]}
    r = run_contract(case)
    xn, _ = _mlp_ref(o)
    np.testing.assert_array_equal(r["x_out"].cpu().numpy(), xn.astype(np.float32))     # x_out keeps x + delta
    _check_qkv(o, r["x_next"].cpu().numpy(), r["qkv"].float().cpu().numpy())
    w1f, u, cb = ops.ln_fold_weights(d["w1"], d["lw"], d["lb"], d["b1"])
    wqf, uq, cq = ops.ln_fold_weights(d["wq"], d["lw1"], d["lb1"], d["bq"])
    want = ops.mlp_fused(d["x"], d["dl"], ops.mlp_pack(w1f, d["w2"], wqf), u, cb, d["b2"], qkv=(uq, cq))
    assert T.equal(want[0], r["qkv"]) and T.equal(want[1], r["x_next"]), "the wrapper's clone path gives other bits"


@pytest.mark.parametrize("with_qkv", [False, True], ids=["plain", "qkv"])
@pytest.mark.parametrize("M", [128, 129, 777, 1500])
def test_attn_out_mlp_fused_and_mlp_pack_op(T, gww, M, with_qkv):
    from gw_whisper_amd import ops
    from gw_whisper_amd._lib import lib
    o, d = _block(T, M, M + 5)
    NQ, F, Mp = (1152 if with_qkv else 0), 1536, (M + 127) // 128 * 128

    def case(g):
        w1f, u, cb, wqf, uq, cq = _folded(T, ops, g, d)
        if not with_qkv:
            px = g.place(d["x"])
            c, x_new = ops.attn_out_mlp_fused(px, g.place(d["ctx"]), g.place(d["wo"]), g.place(d["bo"]), w1f, g.place(d["w2"]),
                                              u, cb, g.place(d["b2"]))
            assert T.equal(px, d["x"])
            return {"c": c, "x_mid": x_new}
        pwo, pw2 = g.place(d["wo"]), g.place(d["w2"])
        wt = g.empty((384 * 384 + 2 * 384 * F + NQ * 384,), T.bfloat16)
        _ok(lib().gww_mlp_pack_op_bf16(pwo.data_ptr(), w1f.data_ptr(), pw2.data_ptr(), wqf.data_ptr(), wt.data_ptr(), 384, F, NQ,
                                       _stream(T)), "gww_mlp_pack_op_bf16")
        px, pctx, pbo, pb2 = g.place(d["x"]), g.place(d["ctx"]), g.place(d["bo"]), g.place(d["b2"])
        x_out, qkv = g.empty((M, 384), T.float32), g.empty((Mp, NQ), T.bfloat16)
        _ok(lib().gww_attn_out_mlp_fused_bf16(px.data_ptr(), pctx.data_ptr(), pbo.data_ptr(), x_out.data_ptr(), u.data_ptr(),
                                              cb.data_ptr(), wt.data_ptr(), pb2.data_ptr(), None, M, 384, F, uq.data_ptr(),
                                              cq.data_ptr(), qkv.data_ptr(), NQ, _stream(T)), "gww_attn_out_mlp_fused_bf16")
        return {"wt": wt, "x_next": px, "x_mid": x_out, "qkv": qkv[:M]}
    r = run_contract(case, arena_row_bytes=2 * 1536)
    if not with_qkv:
        # x_mid = x + bf16(ctx Wo^T + bo): the bound of test_gpu_kernels.py::test_attn_out_mlp_fused
        delta = o["ctx"].astype(np.float64) @ o["wo"].astype(np.float64).T + o["bo"]
        x_mid_ref = o["x"].astype(np.float64) + _bf(delta).astype(np.float64)
        err = np.abs(r["x_mid"].cpu().numpy() - x_mid_ref)
        assert (err <= np.abs(delta) * 2.0 ** -7 + 1e-6 + 2e-5).all() and err.mean() < 1e-4
        return
    # the bounds of test_gpu_kernels.py::test_attn_out_mlp_qkv_fused_against_fp64 (x_next, then q / k / v of it)
    from tests.test_gpu_kernels import _block_fp64
    x_mid, mlp = _block_fp64(o)
    got_x = r["x_next"].cpu().numpy().astype(np.float64)
    assert (np.abs(got_x - (x_mid + mlp)) <= np.abs(mlp) * 2.0 ** -7 + np.abs(x_mid - o["x"]) * 2.0 ** -7 + 4e-2).all()
    assert np.sqrt(((got_x - (x_mid + mlp)) ** 2).mean()) < 8e-3
    assert np.abs(r["x_mid"].cpu().numpy() - x_mid).max() <= np.abs(x_mid - o["x"]).max() * 2.0 ** -7 + 1e-3
    _check_qkv(o, r["x_next"].cpu().numpy(), r["qkv"].float().cpu().numpy())


@pytest.mark.parametrize("M", [128, 129, 777, 1500])
def test_attn_out_mlp_final_and_lnqkv_fused(T, gww, M):
    from gw_whisper_amd import ops
    from tests.test_gpu_kernels import _block_fp64
    o, d = _block(T, M, M + 23)

    def case(g):
        w1f, u, cb, wqf, uq, cq = _folded(T, ops, g, d)
        px = g.place(d["x"])
        y, x_mid = ops.attn_out_mlp_final(px, g.place(d["ctx"]), g.place(d["wo"]), g.place(d["bo"]), w1f, g.place(d["w2"]), u, cb,
                                          g.place(d["b2"]), g.place(d["lw1"]), g.place(d["lb1"]))
        wtq = ops.mlp_pack(None, None, wqf)
        qkv = ops.lnqkv_fused(px, wtq, uq, cq)
        assert T.equal(px, d["x"]), "x is only read by both"
        return {"y": y, "x_mid": x_mid, "wtq": wtq, "qkv": qkv}
    r = run_contract(case)
    x_mid, mlp = _block_fp64(o)
    # bounds of test_gpu_kernels.py::test_attn_out_mlp_final_layernorm_against_fp64
    assert np.abs(r["x_mid"].cpu().numpy() - x_mid).max() <= np.abs(x_mid - o["x"]).max() * 2.0 ** -7 + 1e-3
    ref = oenc.layer_norm(r["x_mid"].cpu().numpy().astype(np.float64) + mlp, o["lw1"], o["lb1"])
    got = r["y"].cpu().numpy().astype(np.float64)
    np.testing.assert_allclose(got, ref, atol=3e-2, rtol=0)
    assert np.sqrt(((got - ref) ** 2).mean()) < 4e-3
    # test_gpu_kernels.py::test_lnqkv_fused
    refq = oenc.layer_norm(o["x"].astype(np.float64), o["lw1"], o["lb1"]) @ o["wq"].astype(np.float64).T + o["bq"]
    gq = r["qkv"].float().cpu().numpy()
    np.testing.assert_allclose(gq, refq, atol=6e-2, rtol=2e-2)
    assert np.abs(gq - refq).mean() < 6e-3


# ------------------------------------------------------------------ conv stem, LayerNorm, element-wise
@pytest.mark.parametrize("B,Tn,d", [(3, 100, 384), (2, 257, 384), (1, 128, 512), (2, 129, 768), (1, 1, 1024)])
def test_conv1_gelu(T, gww, B, Tn, d):
    """Rows 0 and T + 1 of every segment are zero, and nothing lies beyond [B, T + 2, d]."""
    from gw_whisper_amd import ops
    rng = np.random.default_rng(B * 7 + Tn + d)
    mel = T.from_numpy(rng.standard_normal((B, 80, Tn)).astype(np.float32) * 0.8)
    w = T.from_numpy((rng.standard_normal((d, 80, 3)) / np.sqrt(240)).astype(np.float32))
    b = T.from_numpy(rng.standard_normal(d).astype(np.float32) * 0.3)
    md, wd, bd = mel.cuda(), w.cuda(), b.cuda()
    got = run_contract(lambda g: {"c1": ops.conv1_gelu(g.place(md), g.place(wd), g.place(bd))})["c1"]
    assert got.shape == (B, Tn + 2, d) and got.dtype == T.bfloat16
    got = got.float().cpu()
    assert T.count_nonzero(got[:, 0]) == 0 and T.count_nonzero(got[:, Tn + 1]) == 0
    r16 = lambda t: t.to(T.bfloat16).to(T.float64)
    ref = T.nn.functional.gelu(T.nn.functional.conv1d(r16(mel), r16(w), b.double(), padding=1)).transpose(1, 2)
    err = (got[:, 1:Tn + 1].double() - ref).abs()
    # bound of test_gpu_kernels.py::test_conv1_gelu_from_the_feature_layout
    assert float((err - (2.0 ** -8) * ref.abs()).max()) < 1e-3, float(err.max())


@pytest.mark.parametrize("M", [1, 1003])
@pytest.mark.parametrize("d", [128, 384, 1280])
def test_layernorm_and_cast(T, gww, d, M):
    from gw_whisper_amd import ops
    rng = np.random.default_rng(d + M)
    x = (rng.standard_normal((M, d)) * 3 + 0.5).astype(np.float32)
    w = (1 + 0.1 * rng.standard_normal(d)).astype(np.float32)
    b = (0.1 * rng.standard_normal(d)).astype(np.float32)
    xd, wd, bd = _dev(T, x), _dev(T, w), _dev(T, b)

    def case(g):
        px, pw, pb = g.place(xd), g.place(wd), g.place(bd)
        return {"y": ops.layernorm(px, pw, pb), "yb": ops.layernorm(px, pw, pb, out_bf16=True), "xb": ops.cast_bf16(px)}
    r = run_contract(case)
    ref = oenc.layer_norm(x.astype(np.float64), w, b)
    np.testing.assert_allclose(r["y"].cpu().numpy(), ref, atol=3e-6, rtol=1e-5)       # test_gpu_kernels.py::test_layernorm
    np.testing.assert_allclose(r["yb"].float().cpu().numpy(), _bf(r["y"].cpu().numpy()), atol=0, rtol=2 ** -7)
    np.testing.assert_array_equal(r["xb"].float().cpu().numpy(), _bf(x))              # ::test_cast_bf16_round_to_nearest_even


@pytest.mark.parametrize("M", [1, 517])
@pytest.mark.parametrize("d", [128, 384, 1024])
@pytest.mark.parametrize("dy_f32", [True, False], ids=["dy_fp32", "dy_bf16"])
def test_layernorm_backward_and_param_grads(T, gww, d, M, dy_f32):
    """gww_layernorm_bwd plain, and accumulating into a ``place``d dx with the bf16 copy; gww_layernorm_param_grads with its
    workspace at the queried size (the wrapper allocates exactly that)."""
    from gw_whisper_amd import ops
    from tests.test_gpu_backward_widths import _ln_rows
    x, g_ = _ln_rows(T, M, d, 1000 * d + M)
    gamma = (1 + 0.1 * T.randn(d, generator=g_, dtype=T.float64)).float()
    dy = T.randn((M, d), generator=g_)
    dy = dy if dy_f32 else dy.bfloat16()
    base = T.randn((M, d), generator=g_)
    xp = T.randn((M, d), generator=g_) * 2 + 0.5          # the rows of test_layernorm_param_grads_match_fp64
    xd, gd, dyd, based, xpd = x.cuda(), gamma.cuda(), dy.cuda(), base.cuda(), xp.cuda()

    def case(g):
        px, pg, pdy = g.place(xd), g.place(gd), g.place(dyd)
        dx, dxb = ops.layernorm_bwd(px, pg, pdy, want_bf16=True)
        acc = g.place(based)
        _, accb = ops.layernorm_bwd(px, pg, pdy, dx=acc, want_bf16=True)
        dgamma, dbeta = ops.layernorm_param_grads(g.place(xpd), pdy)
        return {"dx": dx, "dxb": dxb, "acc": acc, "accb": accb, "dgamma": dgamma, "dbeta": dbeta}
    r = run_contract(case)
    x64, gy = x.double(), dy.double() * gamma.double()
    mu = x64.mean(1, keepdim=True)
    rstd = 1 / T.sqrt(((x64 - mu) ** 2).mean(1, keepdim=True) + 1e-5)
    xh = (x64 - mu) * rstd
    ref = rstd * (gy - gy.mean(1, keepdim=True) - xh * (gy * xh).mean(1, keepdim=True))
    # bounds of test_gpu_backward_widths.py::test_layernorm_backward_every_width
    T.testing.assert_close(r["dx"].cpu().double(), ref, atol=2e-5, rtol=1e-4)
    T.testing.assert_close(r["dxb"].cpu().double(), ref, atol=1e-5, rtol=2 ** -8)
    T.testing.assert_close(r["acc"].cpu().double(), base.double() + ref, atol=3e-5, rtol=1e-4)
    assert T.equal(r["accb"].cpu(), r["acc"].cpu().bfloat16())
    # bounds of test_gpu_full_finetune.py::test_layernorm_param_grads_match_fp64
    dy64, xp64 = dy.double(), xp.double()
    xh = (xp64 - xp64.mean(1, keepdim=True)) / T.sqrt(xp64.var(1, unbiased=False, keepdim=True) + 1e-5)
    assert ((r["dgamma"].cpu().double() - (dy64 * xh).sum(0)).abs() <= 1e-4 * (dy64.abs() * xh.abs()).sum(0) + 1e-5).all()
    assert ((r["dbeta"].cpu().double() - dy64.sum(0)).abs() <= 1e-4 * dy64.abs().sum(0) + 1e-5).all()


@pytest.mark.parametrize("shape", [(1, 8), (777, 384)])
def test_gelu_bf16(T, gww, shape):
    """Forward and backward form: identical and finite under every fill, and the forward against torch's erf GELU of
    the same bf16 input to one bf16 rounding."""
    from gw_whisper_amd import ops
    g_ = T.Generator().manual_seed(shape[0])
    z = (T.randn(shape, generator=g_) * 2).bfloat16().cuda()
    dg = T.randn(shape, generator=g_).bfloat16().cuda()

    def case(g):
        pz = g.place(z)
        return {"y": ops.gelu_bf16(pz), "dz": ops.gelu_bf16(pz, g.place(dg))}
    r = run_contract(case)
    assert r["y"].shape == z.shape and r["dz"].shape == z.shape


# ------------------------------------------------------------------ attention forward
ATT_SHAPES = [(1, 64, 1), (1, 1, 1), (2, 65, 2), (3, 129, 6), (1, 1500, 2)]


def _attn_ref(qkv, H, bf16):
    d = qkv.shape[-1] // 3
    q, k, v = qkv[..., :d], qkv[..., d:2 * d], qkv[..., 2 * d:]
    return oenc.attention(q.astype(np.float64), k.astype(np.float64), v.astype(np.float64), H, bf16, np.float64)


def _lse_ref(q, k, H):
    out = []
    for h in range(H):
        s = np.einsum("bqd,bkd->bqk", q[..., h * 64:(h + 1) * 64], k[..., h * 64:(h + 1) * 64])
        m = s.max(-1, keepdims=True)
        out.append((m + np.log(np.exp(s - m).sum(-1, keepdims=True)))[..., 0])
    return np.stack(out, 1)


@pytest.mark.parametrize("B,Tn,H", ATT_SHAPES)
def test_attention_bf16_forwards(T, gww, B, Tn, H):
    """gww_attention_bf16, gww_attention_lse_bf16 and gww_attention_log2q_bf16 with and without lse."""
    from gw_whisper_amd import ops
    from tests.test_gpu_kernels import _attn_ref_log2q, _to_log2q
    rng = np.random.default_rng(B * 1000 + Tn + H)
    qkv = _bf(rng.standard_normal((B, Tn, 3 * H * 64)) * 0.7)
    qkv_l2 = _to_log2q(qkv)
    qd, ql = _dev(T, qkv, T.bfloat16), _dev(T, qkv_l2, T.bfloat16)

    def case(g):
        pq, pl = g.place(qd), g.place(ql)
        ctx_lse, lse = ops.attention_lse(pq, H)
        ctx_l2, lse_l2 = ops.attention_log2q(pl, H, want_lse=True)
        return {"ctx": ops.attention(pq, H), "ctx_lse": ctx_lse, "lse": lse, "ctx_l2": ctx_l2, "lse_l2": lse_l2,
                "ctx_l2_nolse": ops.attention_log2q(pl, H)}
    r = run_contract(case)
    assert T.equal(r["ctx_l2"], r["ctx_l2_nolse"])
    ref = _attn_ref(qkv, H, True)
    d = H * 64
    for name in ("ctx", "ctx_lse"):
        # test_gpu_kernels.py::test_attention_bf16
        np.testing.assert_allclose(r[name].float().cpu().numpy(), ref, atol=6e-3, rtol=2 ** -7)
    # test_gpu_kernels.py::test_attention_log2q (ctx and lse)
    np.testing.assert_allclose(r["ctx_l2"].float().cpu().numpy(), _attn_ref_log2q(qkv_l2, H), atol=6e-3, rtol=2 ** -7)
    lse_ref = _lse_ref(qkv_l2[..., :d].astype(np.float64) / LOG2E, qkv_l2[..., d:2 * d].astype(np.float64), H)
    np.testing.assert_allclose(r["lse_l2"].cpu().numpy(), lse_ref, atol=2e-2, rtol=1e-3)
    # test_gpu_backward_widths.py::_check_attention_bwd (natural-unit lse)
    lse_nat = _lse_ref(qkv[..., :d].astype(np.float64), qkv[..., d:2 * d].astype(np.float64), H)
    np.testing.assert_allclose(r["lse"].cpu().numpy(), lse_nat, atol=4e-3, rtol=1e-4)


@pytest.mark.parametrize("B,Tn,H", [(1, 32, 1), (1, 1, 1), (2, 65, 2), (2, 200, 2), (1, 1500, 2)])
def test_attention_f32_forwards(T, gww, B, Tn, H):
    from gw_whisper_amd import ops
    rng = np.random.default_rng(B * 1000 + Tn + H + 1)
    qkv = (rng.standard_normal((B, Tn, 3 * H * 64)) * 0.7).astype(np.float32)
    qd = _dev(T, qkv)

    def case(g):
        pq = g.place(qd)
        ctx2, lse = ops.attention_lse_f32(pq, H)
        return {"ctx": ops.attention(pq, H), "ctx_lse": ctx2, "lse": lse}
    r = run_contract(case)
    assert T.equal(r["ctx"], r["ctx_lse"]), "gww_attention_lse_f32's ctx is bit-identical to gww_attention_f32's"
    np.testing.assert_allclose(r["ctx"].cpu().numpy(), _attn_ref(qkv, H, False), atol=2e-5, rtol=1e-4)   # ::test_attention_f32


@pytest.mark.parametrize("B,Tn,H", [(1, 4, 1), (1, 64, 1), (2, 200, 2), (1, 260, 3)])
def test_attention_probs(T, gww, B, Tn, H):
    """gww_attention_probs_bf16 (natural and log2-unit q) and _f32 called directly: probs is exactly [B, H, T, T]."""
    from gw_whisper_amd._lib import lib
    from tests.test_gpu_kernels import _to_log2q
    from tests.test_gpu_encoder_outputs import FP64_ATT, _check_rows
    rng = np.random.default_rng(B * 100 + Tn + H)
    qkv = _bf(rng.standard_normal((B, Tn, 3 * H * 64)) * 0.3)
    qkv_l2 = _to_log2q(qkv)
    q16, ql2, q32 = _dev(T, qkv, T.bfloat16), _dev(T, qkv_l2, T.bfloat16), _dev(T, qkv)

    def case(g):
        p16, pl2, p32 = g.place(q16), g.place(ql2), g.place(q32)
        out = {k: g.empty((B, H, Tn, Tn), T.float32) for k in ("bf16", "log2q", "f32")}
        _ok(lib().gww_attention_probs_bf16(p16.data_ptr(), 0, out["bf16"].data_ptr(), B, Tn, H, _stream(T)), "probs_bf16")
        _ok(lib().gww_attention_probs_bf16(pl2.data_ptr(), 1, out["log2q"].data_ptr(), B, Tn, H, _stream(T)), "probs_bf16")
        _ok(lib().gww_attention_probs_f32(p32.data_ptr(), out["f32"].data_ptr(), B, Tn, H, _stream(T)), "probs_f32")
        return out
    r = run_contract(case)
    d = H * 64
    heads = lambda a: a.reshape(B, Tn, H, 64).transpose(0, 2, 1, 3).astype(np.float64)

    def softmax64(q, k):
        s = heads(q) @ heads(k).transpose(0, 1, 3, 2)
        p = np.exp(s - s.max(-1, keepdims=True))
        return p / p.sum(-1, keepdims=True)
    ref = softmax64(qkv[..., :d], qkv[..., d:2 * d])
    ref_l2 = softmax64(qkv_l2[..., :d].astype(np.float64) / LOG2E, qkv_l2[..., d:2 * d])
    # the bounds of test_gpu_encoder_outputs.py::test_full_geometry_against_fp64 (FP64_ATT, _check_rows)
    for name, want, prec in (("f32", ref, "fp32"), ("bf16", ref, "bf16"), ("log2q", ref_l2, "bf16")):
        _check_rows(T, r[name])
        assert np.abs(r[name].cpu().numpy() - want).max() < FP64_ATT[prec], name


# ------------------------------------------------------------------ attention backward
@pytest.mark.parametrize("q_log2", [False, True], ids=["natural_q", "log2_q"])
@pytest.mark.parametrize("B,Tn,H", [(1, 64, 1), (1, 1, 2), (3, 129, 3), (2, 65, 2), (1, 1500, 2)])
def test_attention_backward_bf16(T, gww, B, Tn, H, q_log2):
    """d_scratch at exactly the documented B * H * (T + ceil(T / 64)) fp32 words (what the wrapper allocates), poisoned."""
    from gw_whisper_amd import ops
    from tests.test_gpu_backward_widths import _attn64
    g_ = T.Generator().manual_seed(B * 10000 + Tn * 10 + H)
    rb = lambda t: t.to(T.bfloat16).double()
    qkv = rb(T.randn((B, Tn, 3 * H * 64), generator=g_, dtype=T.float64) * 0.6)
    if q_log2:
        qkv[..., :H * 64] = rb(qkv[..., :H * 64] * LOG2E)
    dctx = rb(T.randn((B, Tn, H * 64), generator=g_, dtype=T.float64) * 0.5)
    dctx[:, : Tn // 2] = 0                         # dead query tiles: the live-tile flags of d_scratch are exercised
    qd, dcd = qkv.float().cuda().bfloat16(), dctx.float().cuda().bfloat16()
    ctx, lse = ops.attention_log2q(qd, H, want_lse=True) if q_log2 else ops.attention_lse(qd, H)

    def case(g):
        return {"dqkv": ops.attention_bwd(g.place(qd), g.place(ctx), g.place(dcd), g.place(lse), H, q_log2=q_log2)}
    got = run_contract(case)["dqkv"].cpu().double().reshape(B, Tn, 3, H, 64)
    ref = _attn64(T, qkv, dctx, H, q_log2)[2].reshape(B, Tn, 3, H, 64)
    # bounds of test_gpu_backward_widths.py::_check_attention_bwd
    err = (got - ref).abs()
    scale = T.maximum(ref.abs().amax(dim=(1, 4)), 1e-3 * ref.abs().amax(dim=(0, 1, 3, 4))[None, :, None])
    assert not ((err.amax(dim=(1, 4)) > 2e-2 * scale) | (err.pow(2).mean(dim=(1, 4)).sqrt() > 3e-3 * scale)).any()


@pytest.mark.parametrize("B,Tn,H", [(1, 77, 2), (3, 1, 16), (2, 33, 2), (1, 300, 2)])
def test_attention_backward_f32(T, gww, B, Tn, H):
    """d_scratch at gww_attention_bwd_f32_scratch_bytes (what the wrapper allocates)."""
    from gw_whisper_amd import ops
    g_ = T.Generator().manual_seed(B * 100 + Tn + H)
    qkv = (T.randn((B, Tn, 3 * H * 64), generator=g_) * 0.6).cuda()
    dctx = (T.randn((B, Tn, H * 64), generator=g_) * 0.5)
    dctx[:, : Tn // 2] = 0
    dctx = dctx.cuda()
    ctx, lse = ops.attention_lse_f32(qkv, H)

    def case(g):
        return {"dqkv": ops.attention_bwd_f32(g.place(qkv), g.place(ctx), g.place(dctx), g.place(lse), H)}
    run_contract(case)


# ------------------------------------------------------------------ DoRA merge
def _merge_case(T, d_out, d_in, r, seed):
    rng = np.random.default_rng(d_out + r + seed)
    W0 = (rng.standard_normal((d_out, d_in)) / np.sqrt(d_in)).astype(np.float32)
    A, B, m = synth.dora_adapter(d_out, d_in, r, W0, seed=3 + seed)
    return (W0, A, B, m), tuple(_dev(T, t) for t in (W0, A, B, m))


@pytest.mark.parametrize("d_out,d_in,r", [(384, 384, 8), (1536, 384, 8), (384, 1536, 4), (128, 128, 1)])
def test_dora_merge(T, gww, d_out, d_in, r):
    """norm_out given (the wrapper) and NULL (the C entry point called directly)."""
    from gw_whisper_amd import ops
    from gw_whisper_amd._lib import lib
    host, dev = _merge_case(T, d_out, d_in, r, 0)
    s = 32.0 / r

    def case(g):
        p = [g.place(t) for t in dev]
        w, nrm = ops.dora_merge(*p, s, return_norm=True)
        w2 = g.empty((d_out, d_in), T.float32)
        _ok(lib().gww_dora_merge_f32(*[t.data_ptr() for t in p], s, d_out, d_in, r, w2.data_ptr(), None, _stream(T)),
            "gww_dora_merge_f32")
        return {"w": w, "nrm": nrm, "w_no_norm": w2}
    out = run_contract(case)
    assert T.equal(out["w"], out["w_no_norm"])
    W0, A, B, m = (t.astype(np.float64) for t in host)
    # tolerances of test_gpu_kernels.py::test_dora_merge
    np.testing.assert_allclose(out["w"].cpu().numpy(), odora.dora_merge(W0, A, B, m, s), atol=2e-6, rtol=1e-5)
    np.testing.assert_allclose(out["nrm"].cpu().numpy(), odora.dora_weight_norm(W0, A, B, s), rtol=1e-5)


def test_dora_merge_batch(T, gww):
    """45 modules of mixed shape (more than one 40-op descriptor table) through the wrapper, and five with norm_out NULL."""
    from gw_whisper_amd import _lib, ops
    shapes = [(384, 384, 8), (768, 768, 16), (1536, 384, 8), (384, 1536, 4), (512, 512, 32)] * 9
    cases = [_merge_case(T, *s, seed=i) for i, s in enumerate(shapes)]

    def case(g):
        items = [tuple(g.place(t) for t in dev) + (32.0 / s[2],) for (_, dev), s in zip(cases, shapes)]
        got = ops.dora_merge_batch(items)
        out = {}
        for i, (w, nrm) in enumerate(got):
            out[f"w{i}"], out[f"n{i}"] = w, nrm
        arr = (_lib.DoraMergeItem * 5)()
        for i in range(5):
            w0, a, b, m, s = items[i]
            out[f"bare{i}"] = g.empty(tuple(w0.shape), T.float32)
            arr[i] = _lib.DoraMergeItem(w0.data_ptr(), a.data_ptr(), b.data_ptr(), m.data_ptr(), out[f"bare{i}"].data_ptr(), None,
                                        s, w0.shape[0], w0.shape[1], a.shape[0])
        _ok(_lib.lib().gww_dora_merge_batch_f32(arr, 5, _stream(T)), "gww_dora_merge_batch_f32")
        return out
    r = run_contract(case)
    for i in range(5):
        assert T.equal(r[f"bare{i}"], r[f"w{i}"])
        W0, A, B, m = (t.astype(np.float64) for t in cases[i][0])
        # tolerance of test_gpu_kernels.py::test_dora_merge_batch_equals_the_single_merges
        np.testing.assert_allclose(r[f"w{i}"].cpu().numpy(), odora.dora_merge(W0, A, B, m, 32.0 / shapes[i][2]), atol=2e-6,
                                   rtol=1e-5)


# ------------------------------------------------------------------ adapter gradients, weight gradients
@pytest.mark.parametrize("M", [31, 777])
@pytest.mark.parametrize("d", [128, 384, 768])
def test_dora_grads_on_packed_qkv_sections(T, gww, d, M):
    """gww_dora_grads on the q / k / v sections of exact-size packed [M, 3 d] buffers with ldy = 3 d: the section at
    column 2 d ends where the buffer ends.  The kernel adds with float atomics: compared at the run-to-run bound of
    test_gpu_backward_widths.py::test_dora_grads_on_packed_qkv_sections (2e-5 of the largest entry)."""
    from gw_whisper_amd import ops
    g_ = T.Generator().manual_seed(7 * d + M)
    x = T.randn((M, d), generator=g_).bfloat16().cuda()
    dy = (T.randn((M, 3 * d), generator=g_) * 0.3).bfloat16().cuda()
    y = T.randn((M, 3 * d), generator=g_).bfloat16().cuda()
    secs = []
    for sec in range(3):
        W0 = (T.randn((d, d), generator=g_) / math.sqrt(d)).numpy()
        A, Bm, m = (T.from_numpy(a).cuda() for a in synth.dora_adapter(d, d, 8, W0, seed=4 + sec))
        nrm = T.linalg.norm(T.from_numpy(W0).cuda() + 4.0 * (Bm @ A), dim=1)
        secs.append((A, Bm, m, nrm, (T.randn(d, generator=g_) * 0.1).cuda()))

    def case(g):
        px, pdy, py = g.place(x), g.place(dy), g.place(y)
        out = {}
        for sec, (A, Bm, m, nrm, bias) in enumerate(secs):
            ysc = 0.125 * LOG2E if sec == 0 else 1.0
            out[f"dA{sec}"], out[f"dB{sec}"], out[f"dm{sec}"] = ops.dora_grads(
                px, pdy, py, g.place(bias), ysc, 4.0, g.place(A), g.place(Bm), g.place(m), g.place(nrm), col_off=sec * d)
        return out
    names = [f"{k}{s}" for k in ("dA", "dB", "dm") for s in range(3)]
    run_contract(case, atomic={n: 2e-5 for n in names})


@pytest.mark.parametrize("d,M,np_", [(384, 3000, 3), (512, 1111, 3), (384, 100, 2), (384, 31, 3)])
def test_dora_grads_multi(T, gww, d, M, np_):
    """Shapes of test_gpu_training.py::test_dora_parameter_gradients_fused_qkv; exact-size [M, np d] dy / y."""
    from gw_whisper_amd import ops
    g_ = T.Generator().manual_seed(d + M)
    x = T.randn((M, d), generator=g_).bfloat16().cuda()
    dy = (T.randn((M, np_ * d), generator=g_) * 0.3).bfloat16().cuda()
    y = T.randn((M, np_ * d), generator=g_).bfloat16().cuda()
    per = []
    for p in range(np_):
        W0 = (T.randn((d, d), generator=g_) / math.sqrt(d)).numpy()
        A, Bm, m = (T.from_numpy(a).cuda() for a in synth.dora_adapter(d, d, 8, W0, seed=9 + p))
        nrm = T.linalg.norm(T.from_numpy(W0).cuda() + 4.0 * (Bm @ A), dim=1)
        per.append(((T.randn(d, generator=g_) * 0.1).cuda(), A, Bm, m, nrm))

    def case(g):
        pl = [[g.place(t) for t in p] for p in per]
        got = ops.dora_grads_multi(g.place(x), g.place(dy), g.place(y), [p * d for p in range(np_)], [p[0] for p in pl],
                                   [0.125 * LOG2E] + [1.0] * (np_ - 1), [4.0] * np_, [p[1] for p in pl], [p[2] for p in pl],
                                   [p[3] for p in pl], [p[4] for p in pl])
        return {f"{k}{i}": t for i, trip in enumerate(got) for k, t in zip(("dA", "dB", "dm"), trip)}
    # k_dora_reduce adds five partial sums into every dm element by float atomics (dA / dB have one adder per element and
    # are exact): the run-to-run bound of test_gpu_backward_widths.py::test_dora_grads_on_packed_qkv_sections, which runs
    # this kernel with one projection
    run_contract(case, atomic={f"dm{i}": 2e-5 for i in range(np_)})


@pytest.mark.parametrize("f32", [False, True], ids=["bf16", "fp32"])
@pytest.mark.parametrize("M,d_in,d_out,r", [(1, 128, 128, 1), (31, 384, 1536, 8), (777, 1536, 384, 16), (257, 512, 512, 64)])
def test_adapter_grads(T, gww, M, d_in, d_out, r, f32):
    """gww_adapter_grads / _f32 with scratch NULL (the wrappers: stream-ordered, library-owned) and with a poisoned scratch
    of exactly the queried bytes; both must give the same bits; rows strided (ldx, ldy larger than the row)."""
    from gw_whisper_amd import ops
    from gw_whisper_amd._lib import lib
    from tests.test_gpu_adapter_targets import _kernel_case, _kernel_ref
    x, dy, y, W0, A, Bm, m, b = _kernel_case(T, M, d_in, d_out, r, seed=1000 * d_in + M, stride_pad=8)
    s = 32.0 / r
    dt = T.float32 if f32 else T.bfloat16
    n = T.linalg.norm(W0 + s * (Bm @ A), dim=1)
    # (_kernel_case returns [M, d + 8] host tensors: the first d columns are the operands; the stride gap is the guard's)
    x, dy, y = x[:, :d_in], dy[:, :d_out], y[:, :d_out]
    xc, dyc, yc = x.to(dt).cuda().contiguous(), dy.to(dt).cuda().contiguous(), y.to(dt).cuda().contiguous()
    small = [t.float().cuda() for t in (b, A, Bm, m, n)]
    fn = lib().gww_adapter_grads_f32 if f32 else lib().gww_adapter_grads
    need = (lib().gww_adapter_grads_f32_scratch_bytes if f32 else lib().gww_adapter_grads_scratch_bytes)(M, d_in, d_out, r)
    wrapper = ops.adapter_grads_f32 if f32 else ops.adapter_grads

    def case(g):
        px, pdy, py = g.place(xc, pitch=d_in + 8), g.place(dyc, pitch=d_out + 8), g.place(yc, pitch=d_out + 8)
        assert px.shape == (M, d_in) and px.stride(0) == d_in + 8
        pb, pA, pB, pm, pn = (g.place(t) for t in small)
        dA, dB, dm = wrapper(px, pdy, py, pb, 1.0, s, pA, pB, pm, pn)
        out = {"dA": dA, "dB": dB, "dm": dm}
        scratch = g.empty((max(need, 1),), T.uint8)
        for k, shape in (("dA_s", (r, d_in)), ("dB_s", (d_out, r)), ("dm_s", (d_out,))):
            out[k] = g.zeros(shape, T.float32)
        _ok(fn(px.data_ptr(), px.stride(0), pdy.data_ptr(), py.data_ptr(), pdy.stride(0), pb.data_ptr(), 1.0, s, pA.data_ptr(),
               pB.data_ptr(), pm.data_ptr(), pn.data_ptr(), out["dA_s"].data_ptr(), out["dB_s"].data_ptr(),
               out["dm_s"].data_ptr(), M, d_in, d_out, r, scratch.data_ptr(), need, _stream(T)), "gww_adapter_grads")
        return out
    out = run_contract(case, arena_row_bytes=4 * max(d_in, d_out))
    for k in ("dA", "dB", "dm"):
        assert T.equal(out[k], out[k + "_s"]), f"{k}: caller scratch and library scratch give different bits"
    if not f32:
        # bound of test_gpu_adapter_targets.py::test_adapter_grads_kernel_vs_fp64
        ref = _kernel_ref(T, x, dy, y, W0, A, Bm, m, b, s, 1.0)
        for k, r_ in zip(("dA", "dB", "dm"), ref):
            g_ = out[k].double().cpu()
            assert float(T.linalg.norm(g_ - r_) / (T.linalg.norm(r_) + 1e-30)) <= 0.02, k


@pytest.mark.parametrize("M,N,K", [(64, 384, 384), (1, 64, 16), (3001, 128, 512), (257, 1536, 384)])
def test_gemm_wgrad(T, gww, M, N, K):
    """Workspace at exactly gww_gemm_wgrad_workspace_bytes (the wrapper), dW / db accumulated into zeros."""
    from gw_whisper_amd import ops
    from tests.test_gpu_full_finetune import _bf16, _check_wgrad
    dy = _bf16(T, (M, N), M + N, 0.5)
    x = _bf16(T, (M, K), M + K + 1)

    def case(g):
        dw, db = ops.gemm_wgrad(g.place(dy), g.place(x), db=True)
        return {"dw": dw, "db": db}
    r = run_contract(case, arena_row_bytes=4 * max(N, K))
    _check_wgrad(T, dy, x, r["dw"], r["db"])          # the bound of test_gpu_full_finetune.py::test_wgrad_matches_fp64


def test_gemm_wgrad_strided_conv_views(T, gww):
    """The two im2col views of test_gpu_full_finetune.py::test_wgrad_strided_conv_views over exact-size buffers: the
    last row of each overlapping view ends at the buffer's last element."""
    from gw_whisper_amd import ops
    from tests.test_gpu_full_finetune import _bf16, _check_wgrad
    B, Tn, d, C_ = 2, 300, 384, 80
    M2 = B * (Tn + 1)
    c1 = _bf16(T, (2 * M2 + 1, d), 11)               # row M2 - 1 reads c1 rows 2 (M2 - 1) .. 2 M2: exactly to the end
    dz2 = _bf16(T, (M2, d), 12, 0.5)
    M1 = B * (2 * Tn + 2)
    melT = _bf16(T, ((M1 - 1) * C_ + 256,), 13)
    dz1 = _bf16(T, (M1, d), 14, 0.5)

    def case(g):
        pc1, pm = g.place(c1), g.place(melT)
        dw2, db2 = ops.gemm_wgrad(g.place(dz2), pc1.as_strided((M2, 3 * d), (2 * d, 1)), db=True, k=3 * d)
        dw1, db1 = ops.gemm_wgrad(g.place(dz1), pm.as_strided((M1, 256), (C_, 1)), db=True, k=256)
        return {"dw2": dw2, "db2": db2, "dw1": dw1, "db1": db1}
    r = run_contract(case, arena_row_bytes=4 * 3 * d)
    _check_wgrad(T, dz2, c1.as_strided((M2, 3 * d), (2 * d, 1)), r["dw2"], r["db2"])
    _check_wgrad(T, dz1, melT.as_strided((M1, 256), (C_, 1)), r["dw1"], r["db1"])


def _untouched(g, t):
    """Under a guard: every element of ``t`` (a part of an output the contract leaves alone) still holds the fill."""
    if isinstance(g, Guard):
        assert g.unwritten(t) == t.numel(), f"{t.numel() - g.unwritten(t)} element(s) outside the contract were written"


# ------------------------------------------------------------------ front ends
@pytest.mark.parametrize("n_mels", [80, 128])
@pytest.mark.parametrize("n", [1, 159, 12345])
def test_logmel_device_with_stride_gap(T, gww, n, n_mels):
    """gww_logmel_f32 with wave_stride > n_samples, the gap holding the fill; seg_max is the wrapper's [n_seg] scratch."""
    from gw_whisper_amd import ops
    w = synth.strain_segments(3, seed=100 + n, n_samples=n)
    wd = _dev(T, w)

    def case(g):
        pw = g.place(wd, pitch=n + 1000)
        full = T.as_strided(pw, (3, n + 1000), (n + 1000, 1), storage_offset=pw.storage_offset())    # rows incl. the gap
        return {"mel": ops.logmel(full, n_samples=n, n_mels=n_mels)}
    got = run_contract(case)["mel"]
    assert got.shape == (3, n_mels, 3000)
    if n_mels == 80:
        np.testing.assert_allclose(got.cpu().numpy(), olm.log_mel(w), atol=2e-5, rtol=0)   # test_gpu_kernels.py::test_logmel_*


@pytest.mark.parametrize("n,seed,shape", [(1, 0, (128, 128)), (5, 1, (128, 128)), (2, 4, (80, 300))])
def test_qscan_energy_and_interp(T, gww, n, seed, shape):
    from gw_whisper_amd.qscan import QScan
    from oracle import qscan as oq
    from tests.test_gpu_qscan import _signals
    x = _signals(n, seed)
    xd = _dev(T, x.astype(np.float32))
    qs = QScan(duration=1.0, sample_rate=2048, spectrogram_shape=list(shape), qrange=[4, 128])

    def case(g):
        out = qs(g.place(xd))
        return {"out": out, "plane": qs.last_plane}
    r = run_contract(case, arena_row_bytes=4 * 2048)
    ref, best = oq.qscan(x, spectrogram_shape=shape, return_plane=True)
    assert int(r["plane"].item()) == best
    # bound of test_gpu_qscan.py::test_qscan_matches_restatement
    assert np.abs(r["out"].cpu().numpy() - ref).max() < 2e-3 * max(np.abs(ref).max(), 1.0)


@pytest.mark.parametrize("variant,n,hw", [("train", 1, 128), ("train", 3, 128), ("inference", 2, 256)])
def test_qadapter_cnn_forward_and_backward(T, gww, variant, n, hw):
    """Both CNN entry points called with poisoned workspaces of exactly the queried bytes.  The weight gradients are
    summed with float atomics (qadapter_cnn.hip): compared at the 6e-3-of-scale bound of
    test_gpu_qscan.py::test_adapter_cnn_backward_kernels_match_the_fp64_torch_gradients; y at the 1e-4 of
    ::test_adapter_cnn_kernels_match_the_fp64_torch_cnn."""
    from gw_whisper_amd._lib import lib
    from gw_whisper_amd.qscan import QTransformAdapter
    T.manual_seed(11 + n)
    ad = (QTransformAdapter.inference_variant() if variant == "inference" else QTransformAdapter.train_variant()).cuda()
    with T.no_grad():
        for p in ad.freq_adapter.parameters():
            p.mul_(1.5).add_(0.02 * T.randn_like(p))
    g_ = T.Generator().manual_seed(5)
    q = T.rand(n, hw, hw, generator=g_, dtype=T.float64) * 2.0
    q[:, hw // 3: hw // 3 + 7, hw // 2: hw // 2 + 40] += 20.0
    q[0, 0, :] = 9.0
    dy = T.randn(n, hw // 4, hw // 4, generator=g_)
    qd, dyd = q.float().cuda(), dy.cuda()
    ps = [p.detach().float().contiguous() for p in ad._cnn_params()]
    c1, c2, c3 = (int(ps[i].shape[0]) for i in (0, 2, 4))
    names = ["dw1", "db1", "dw2", "db2", "dw3", "db3", "dw4", "db4"]

    def case(g):
        pp = [g.place(t) for t in ps]
        packed = g.empty((lib().gww_qadapter_cnn_packed_bytes(c1, c2, c3),), T.uint8)
        _ok(lib().gww_qadapter_cnn_pack_f32(*[t.data_ptr() for t in pp], c1, c2, c3, packed.data_ptr(), _stream(T)), "cnn_pack")
        pq, pdy = g.place(qd), g.place(dyd)
        need = lib().gww_qadapter_cnn_workspace_bytes(n, hw, hw, c1, c2)
        ws = g.empty((need,), T.uint8)
        y = g.empty((n, hw // 4, hw // 4), T.float32)
        _ok(lib().gww_qadapter_cnn_forward_f32(pq.data_ptr(), n, hw, hw, packed.data_ptr(), c1, c2, c3, ws.data_ptr(), need,
                                               y.data_ptr(), _stream(T)), "gww_qadapter_cnn_forward_f32")
        needb = lib().gww_qadapter_cnn_backward_workspace_bytes(n, hw, hw, c1, c2, c3)
        wsb = g.empty((needb,), T.uint8)
        grads = {k: g.empty(tuple(t.shape), T.float32) for k, t in zip(names, ps)}
        _ok(lib().gww_qadapter_cnn_backward_f32(pq.data_ptr(), pdy.data_ptr(), n, hw, hw, packed.data_ptr(), pp[2].data_ptr(),
                                                pp[4].data_ptr(), c1, c2, c3, wsb.data_ptr(), needb,
                                                *[grads[k].data_ptr() for k in names], _stream(T)),
            "gww_qadapter_cnn_backward_f32")
        return dict(grads, y=y)
    r = run_contract(case, arena_row_bytes=4 * hw * max(c1, c2, c3), atomic={k: 6e-3 for k in names})
    ref = ad.freq_adapter.double().cpu()(q[:, None])[:, 0]
    assert (r["y"].double().cpu() - ref).abs().max().item() < 1e-4 * ref.abs().max().item()


@pytest.mark.parametrize("Hin,Win", [(32, 32), (33, 50), (128, 128)])
def test_qadapter_tail_forward_and_backward(T, gww, Hin, Win):
    """The tail writes detector 0 of a stacked [B, 2, F, T] tensor (out_batch_stride = 2 F T > F T): detector 1, the gap
    between the rows it owns, must keep the fill.  The backward reads g with that batch stride."""
    from gw_whisper_amd import ops
    from gw_whisper_amd._lib import lib
    T.manual_seed(Hin * 1000 + Win)
    B, F, Tn = 3, 80, 3000
    y = T.randn(B, Hin, Win, device="cuda")
    sc, bi = T.tensor([0.7], device="cuda"), T.tensor([-0.2], device="cuda")
    gam, bet = T.tensor([1.3, 0.8], device="cuda"), T.tensor([0.05, -0.1], device="cuda")
    gout = T.randn(B, 2, F, Tn, device="cuda")

    def case(g):
        py, ps, pb, pg, pe = g.place(y), g.place(sc), g.place(bi), g.place(gam), g.place(bet)
        out = g.empty((B, 2, F, Tn), T.float32)
        _ok(lib().gww_qadapter_tail_f32(py.data_ptr(), B, Hin, Win, ps.data_ptr(), pb.data_ptr(), pg.data_ptr(), pe.data_ptr(),
                                        out.data_ptr(), out.stride(0), F, Tn, _stream(T)), "gww_qadapter_tail_f32")
        _untouched(g, out[:, 1])
        d_y, d_s, d_b, d_g, d_e = ops.qadapter_tail_backward(g.place(gout)[:, 0], py, ps, pb, pg[:1], F, Tn)
        return {"out": out[:, 0], "d_y": d_y, "d_scale": d_s, "d_bias": d_b, "d_gamma": d_g, "d_beta": d_e}
    r = run_contract(case, arena_row_bytes=4 * Tn)
    ref = (sc * T.nn.functional.adaptive_avg_pool2d(y[:, None], (F, Tn))[:, 0] + bi) * gam[0] + bet[0]
    assert (r["out"] - ref).abs().max().item() < 2e-6     # test_gpu_qscan.py::test_adapter_tail_kernel_matches_the_torch_composition


# ------------------------------------------------------------------ whitening, clustering
@pytest.mark.parametrize("n_seg,n_bins", [(1, 2), (7, 513), (256, 37)])
def test_welch_power_with_row_gap(T, gww, n_seg, n_bins):
    """spec rows have ld = 2 n_bins + 6 > 2 n_bins: the six floats behind every row hold the fill."""
    from gw_whisper_amd._lib import lib
    g_ = T.Generator().manual_seed(n_seg + n_bins)
    spec = T.randn((n_seg, 2 * n_bins), generator=g_).cuda()
    ld = 2 * n_bins + 6

    def case(g):
        ps = g.place(spec, pitch=ld)
        power = g.empty((n_seg, n_bins), T.float32)
        _ok(lib().gww_welch_power_f32(ps.data_ptr(), ld, n_seg, n_bins, 0.25, power.data_ptr(), _stream(T)), "gww_welch_power_f32")
        return {"power": power}
    got = run_contract(case)["power"].double().cpu()
    s = spec.double().cpu().view(n_seg, n_bins, 2)
    ref = (s ** 2).sum(-1) * 0.25
    ref[:, 0] *= 0.5
    ref[:, -1] *= 0.5
    # the PSD bound of test_gpu_inference.py::test_whiten_matches_the_pycbc_restatement
    np.testing.assert_allclose(got.numpy(), ref.numpy(), rtol=2e-4)


@pytest.mark.parametrize("n_seg", [1, 2, 3, 256, 257])
def test_column_median_equals_numpy(T, gww, n_seg):
    """numpy.median exactly, with a column of ties, a column of zeros and a column that is half zeros."""
    from gw_whisper_amd._lib import lib
    n_bins = 37
    rng = np.random.default_rng(n_seg)
    p = (rng.standard_normal((n_seg, n_bins)) ** 2).astype(np.float32)
    p[:, 3] = 0.75
    p[:, 5] = 0.0
    p[: n_seg // 2, 7] = 0.0
    p[:, 9] = np.float32(1.0) + np.float32(2.0 ** -23) * (np.arange(n_seg) % 3)       # neighbouring floats
    pd = _dev(T, p)

    def case(g):
        med, pp = g.empty((n_bins,), T.float32), g.place(pd)
        _ok(lib().gww_column_median_f32(pp.data_ptr(), n_seg, n_bins, med.data_ptr(), _stream(T)), "gww_column_median_f32")
        return {"median": med}
    got = run_contract(case)["median"].cpu().numpy()
    np.testing.assert_array_equal(got, np.median(p, axis=0))


@pytest.mark.parametrize("D", [1, 3])
@pytest.mark.parametrize("taps4", [4, 516, 1028, 8192])
def test_fir(T, gww, taps4, D):
    """xp holds exactly n_out + taps4 samples per row (then the fill up to xp_stride), out_stride > n_out: the tail of every
    output row keeps the fill.  n_out around the 1024-output block."""
    from gw_whisper_amd._lib import lib
    for n_out in (1, 1023, 1024, 1025, 5000):
        rng = np.random.default_rng(taps4 + n_out + D)
        xp = rng.standard_normal((D, n_out + taps4)).astype(np.float32)
        gf = (rng.standard_normal((D, taps4)) * (32.0 / np.sqrt(taps4))).astype(np.float32)    # output std ~ 32, as whitened noise
        xpd, gd = _dev(T, xp), _dev(T, gf)
        xs, os_ = (n_out + taps4 + 3) // 4 * 4 + 4, (n_out + 3) // 4 * 4 + 4

        def case(g):
            px, pg = g.place(xpd, pitch=xs), g.place(gd)
            out = g.empty((D, os_), T.float32)
            _ok(lib().gww_fir_f32(px.data_ptr(), xs, pg.data_ptr(), taps4, D, out.data_ptr(), os_, n_out, _stream(T)),
                "gww_fir_f32")
            _untouched(g, out[:, n_out:])
            return {"out": out[:, :n_out]}
        got = run_contract(case)["out"].double().cpu().numpy()
        win = np.lib.stride_tricks.sliding_window_view(xp.astype(np.float64), taps4, axis=1)[:, :n_out]
        ref = np.einsum("dnu,du->dn", win, gf.astype(np.float64))
        # the bound of test_gpu_inference.py::test_whiten_matches_the_pycbc_restatement (2e-3 of the whitened std 32)
        assert np.abs(got - ref).max() < 2e-3 * 32, (n_out, np.abs(got - ref).max())


@pytest.mark.parametrize("D", [1, 3])
@pytest.mark.parametrize("taps4", [4, 516, 1028, 8192])
def test_fir_f64(T, gww, taps4, D):
    """test_fir for the fp64 form (fp64 samples, taps and sums, fp32 out): the same extents -- xp holds exactly n_out + taps4
    samples per row, out_stride > n_out -- with xp_stride even but no multiple of 4.  Against the fp64 correlation: the sum
    of <= 8192 products carries about 1e-13 of their l1 norm, so the output is that correlation rounded to fp32 (2^-24
    relative), to within one more unit in the last place."""
    from gw_whisper_amd._lib import lib
    for n_out in (1, 1023, 1024, 1025, 5000):
        rng = np.random.default_rng(taps4 + n_out + D)
        xp = rng.standard_normal((D, n_out + taps4))
        gf = rng.standard_normal((D, taps4)) * (32.0 / np.sqrt(taps4))                        # output std ~ 32, as whitened noise
        xpd, gd = _dev(T, xp), _dev(T, gf)
        xs, os_ = (n_out + taps4 + 3) // 4 * 4 + 2, (n_out + 3) // 4 * 4 + 4

        def case(g):
            px, pg = g.place(xpd, pitch=xs), g.place(gd)
            out = g.empty((D, os_), T.float32)
            _ok(lib().gww_fir_f64(px.data_ptr(), xs, pg.data_ptr(), taps4, D, out.data_ptr(), os_, n_out, _stream(T)),
                "gww_fir_f64")
            _untouched(g, out[:, n_out:])
            return {"out": out[:, :n_out]}
        got = run_contract(case)["out"].double().cpu().numpy()
        win = np.lib.stride_tricks.sliding_window_view(xp, taps4, axis=1)[:, :n_out]
        ref = np.einsum("dnu,du->dn", win, gf)
        l1 = np.abs(gf).sum(axis=1, keepdims=True) * np.abs(xp).max()                          # >= every output's sum |g x|
        excess = (np.abs(got - ref) - (2.0 ** -23 * np.abs(ref) + 1e-12 * l1)).max()
        assert excess <= 0, (n_out, excess, np.abs(got - ref).max())


def test_cluster_triggers_with_fewer_slots_than_clusters(T, gww):
    """100 windows one second apart, all above threshold: 100 clusters; max_clusters = 7 of a 20-entry output.  out_count
    reports 100, exactly 7 entries are written, entries 7 .. 19 keep the fill."""
    from gw_whisper_amd._lib import lib
    n, cap = 100, 7
    times = (1000.25 + T.arange(n, dtype=T.float64)).cuda()
    scores = (0.6 + 0.3 * T.rand(n, generator=T.Generator().manual_seed(1))).cuda()

    def case(g):
        out_t, out_v = g.empty((20,), T.float64), g.empty((20,), T.float32)
        cnt, pt, psc = g.zeros((1,), T.int32), g.place(times), g.place(scores)
        _ok(lib().gww_cluster_triggers_f64(pt.data_ptr(), psc.data_ptr(), n, 0.5, 0.35, out_t.data_ptr(),
                                           out_v.data_ptr(), cnt.data_ptr(), cap, _stream(T)), "gww_cluster_triggers_f64")
        _untouched(g, out_t[cap:])
        _untouched(g, out_v[cap:])
        return {"times": out_t[:cap], "vals": out_v[:cap], "count": cnt}
    r = run_contract(case)
    assert int(r["count"]) == n
    assert T.equal(r["times"], times[:cap]) and T.equal(r["vals"], scores[:cap])


# ------------------------------------------------------------------ MLGWSC-1 training kernels
@pytest.mark.parametrize("B,P", [(1, 8), (3, 128), (33, 1024), (32, 100)])
def test_info_nce_forward_and_backward(T, gww, B, P):
    from gw_whisper_amd import ops
    g_ = T.Generator().manual_seed(B + P)
    z1, z2 = T.randn((B, P), generator=g_).cuda(), T.randn((B, P), generator=g_).cuda()
    dl = T.tensor([0.37], device="cuda")
    tau = 0.1

    def case(g):
        loss, saved = ops.info_nce_forward(g.place(z1), g.place(z2), tau)
        dz1, dz2 = ops.info_nce_backward(saved, tau, g.place(dl))
        return {"loss": loss, "n": saved[0], "nrm": saved[1], "lse": saved[2], "term": saved[3], "dz1": dz1, "dz2": dz2}
    r = run_contract(case)
    z = T.nn.functional.normalize(T.cat([z1, z2]).double(), dim=1)
    S = z @ z.t() / tau
    S.fill_diagonal_(float("-inf"))
    pair = T.arange(2 * B, device="cuda").roll(B)
    ref = float((T.logsumexp(S, 1) - S[T.arange(2 * B, device="cuda"), pair]).sum() / B)
    # bound of test_gpu_mlgwsc_train.py::test_info_nce_kernels_match_the_fp64_reference
    if B > 1:          # (B = 1: each row's only other row is its pair, the loss is zero in exact arithmetic)
        assert abs(float(r["loss"]) - ref) <= 1e-5 * abs(ref) + 1e-7


def test_assemble_batch_with_an_out_of_range_row(T, gww):
    """The wrapper on a valid plan (bit for bit torch's noise + snr * wave), then the C entry point with one index outside
    its array: that row comes out NaN, no other row is touched by it."""
    from gw_whisper_amd import ops
    from gw_whisper_amd._lib import lib
    g_ = T.Generator().manual_seed(3)
    row_len, n_noise, n_wave, R = 2 * 2048, 5, 4, 9
    noise, wave = T.randn((n_noise, row_len), generator=g_).cuda(), T.randn((n_wave, row_len), generator=g_).cuda()
    idx_n = np.array([0, 4, 2, 2, 1, 3, 0, 4, 1])
    idx_w = np.array([1, -1, 3, 0, -1, 2, 2, 0, 3])
    snr = np.linspace(5, 15, R).astype(np.float32)
    bad_n, bad_w = idx_n.copy(), idx_w.copy()
    bad_n[3], bad_w[6] = n_noise, n_wave                 # one past the end of each array
    dn, dw = (T.from_numpy(a.astype(np.int32)).cuda() for a in (bad_n, bad_w))
    ds = T.from_numpy(snr).cuda()
    good = [r for r in range(R) if r not in (3, 6)]

    def case(g):
        pn, pw = g.place(noise), g.place(wave)
        out = ops.assemble_batch(pn, pw, idx_n, idx_w, snr)
        out2, pdn, pdw, pds = g.empty((R, row_len), T.float32), g.place(dn), g.place(dw), g.place(ds)
        _ok(lib().gww_assemble_batch_f32(pn.data_ptr(), n_noise, pw.data_ptr(), n_wave, row_len, pdn.data_ptr(), pdw.data_ptr(),
                                         pds.data_ptr(), R, out2.data_ptr(), _stream(T)), "gww_assemble_batch_f32")
        assert T.isnan(out2[[3, 6]]).all(), "a row with an index outside its array is written NaN"
        out2[[3, 6]] = 0.0            # (checked; cleared so that the other rows can be compared bit for bit)
        return {"out": out, "direct": out2}
    r = run_contract(case)
    w_idx = T.from_numpy(np.maximum(idx_w, 0)).cuda()
    ref = noise[T.from_numpy(idx_n).cuda()] + T.where(T.from_numpy(idx_w).cuda()[:, None] >= 0,
                                                      T.from_numpy(snr).cuda()[:, None] * wave[w_idx], T.zeros((), device="cuda"))
    keep = T.from_numpy(idx_w).cuda() >= 0
    assert T.equal(r["out"][keep], ref[keep]) and T.equal(r["out"][~keep], noise[T.from_numpy(idx_n).cuda()][~keep])
    assert T.equal(r["direct"][good], r["out"][good]) and not r["direct"][[3, 6]].any()


# ------------------------------------------------------------------ glitch head
@pytest.mark.parametrize("train", [False, True], ids=["eval", "train"])
@pytest.mark.parametrize("B,C,d_in", [(1, 1, 128), (7, 6, 384), (33, 64, 1280), (257, 22, 512)])
def test_head_step(T, gww, B, C, d_in, train):
    """Forward (train / eval), backward with ws at gww_head_workspace_bytes (the wrapper), the dropout mask and the
    evaluation accumulate into guarded int64 / fp64 state."""
    from gw_whisper_amd import glitch, ops
    from tests.test_gpu_glitch import _conditioned_case
    seed, offset = 99, 5
    masks = [ops.head_dropout_mask(seed, offset, l, B, w, 0.3) for l, w in enumerate(ops.HEAD_WIDTHS)] if train else None
    x, y, params = _conditioned_case(T, d_in, C, B, 17 * B + C, masks)
    up = T.tensor([0.37], device="cuda")

    def case(g):
        pp = [g.place(p) for p in params]
        loss, logits, row_loss, pred, saved = ops.head_forward(g.place(x), pp, g.place(y), 0.3, train, seed, offset)
        dx, grads = ops.head_backward(saved, g.place(up))
        state = glitch.EvalState(C, "cuda")
        for lo, hi in ((0, B // 2), (B // 2, B)):
            if hi > lo:
                state.add(logits[lo:hi], g.place(y[lo:hi]), row_loss[lo:hi])
        out = {"loss": loss, "logits": logits, "row_loss": row_loss, "pred": pred, "dz": saved[3], "dx": dx,
               "confusion": state.confusion, "loss_sum": state.loss_sum, "n": state.n}
        out.update({f"h{i}": h for i, h in enumerate(saved[2])})
        out.update({f"g{i}": t for i, t in enumerate(grads)})
        out.update({f"mask{l}": ops.head_dropout_mask(seed, offset, l, B, w, 0.3) for l, w in enumerate(ops.HEAD_WIDTHS)})
        return out
    r = run_contract(case)
    assert T.equal(r["pred"], r["logits"].argmax(1)) and int(r["n"]) == B
    cm = np.zeros((C, C), np.int64)
    np.add.at(cm, (y.cpu().numpy(), r["pred"].cpu().numpy()), 1)
    assert np.array_equal(r["confusion"].cpu().numpy(), cm)
    # the loss-sum bound of test_gpu_glitch.py::test_eval_accumulate_ragged_batches_tie_and_nan
    ref_sum = float(r["row_loss"].double().sum())
    assert abs(float(r["loss_sum"]) - ref_sum) <= 1e-12 * abs(ref_sum)
    if train:
        for l in range(3):
            assert T.equal(r[f"mask{l}"], masks[l])
            assert (r[f"h{l}"][masks[l] == 0] == 0).all()


# ====================================================================================== encoder level
# the small encoders of the suite (the ENCODERS tables of test_gpu_adapter_targets.py / test_gpu_full_finetune.py)
ENCODERS = {"micro": synth.ENCODER_SIZES["micro"], "tiny": synth.ENCODER_SIZES["tiny"], "base_l2": (512, 2, 8, 2048),
            "small_l2": (768, 2, 12, 3072), "medium_l2": (1024, 2, 16, 4096)}
QKV = ("self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj")
ALL = QKV + ("self_attn.out_proj", "fc1", "fc2")


def _encoder(name, precision, seed=3):
    from gw_whisper_amd.encoder import WhisperConfig, WhisperEncoder
    d, L, H, F = ENCODERS[name]
    sd = synth.encoder_state_dict(d, L, H, F, seed=seed)
    return WhisperEncoder.from_numpy_state_dict(sd, WhisperConfig(d, L, H, F), precision=precision), sd


def _prec(precision):
    from gw_whisper_amd import _lib
    return {"bf16": _lib.PREC_BF16, "fp32": _lib.PREC_F32}[precision]


def _features(seed, batch):
    from tests.test_gpu_encoder_outputs import _features as f
    return f(seed, batch)


def _forward_case(T, enc, mel, wh, wl, precision):
    """One guarded forward with the workspace re-allocated under the guard at exactly gww_encoder_workspace_bytes."""
    from gw_whisper_amd._lib import lib

    def case(g):
        enc._ws = None
        h, l = enc.forward_raw(g.place(mel), want_hidden=wh, want_last=wl)
        assert g.owns(enc._ws), "the encoder's workspace did not come from the guard"
        assert enc._ws.numel() == lib().gww_encoder_workspace_bytes(enc._handle, mel.shape[0], _prec(precision))
        return {k: v for k, v in (("hidden", h), ("last", l)) if v is not None}
    return case


@pytest.mark.parametrize("precision", ["bf16", "fp32"])
@pytest.mark.parametrize("name", list(ENCODERS))
def test_encoder_forward(T, gww, name, precision):
    """Batches 1, 2, 3 and 5, hidden / last-token outputs in both combinations (both at B = 3); B = 2 runs real log-mel
    features and, on the reduced encoder, is compared with the oracle at the tolerances of __graft_entry__.smoke()."""
    enc, sd = _encoder(name, precision)
    enc = enc.cuda()
    d, L, H, F = ENCODERS[name]
    row = encoder_arena_row_bytes(d, F)
    mel_ref = olm.log_mel(synth.strain_segments(2, seed=21))
    for B in (1, 2, 3, 5):
        mel = _dev(T, mel_ref if B == 2 else _features(40 + B, B))
        for wh, wl in ((True, False), (False, True)) + (((True, True),) if B == 3 else ()):
            r = run_contract(_forward_case(T, enc, mel, wh, wl, precision), arena_row_bytes=row)
            if name == "micro" and B == 2:
                ref = oenc.encoder_forward(sd, mel_ref, oenc.EncCfg(d, L, H, F))
                tol = {"fp32": 2e-3, "bf16": 6e-2}[precision]
                got = r["hidden"].cpu().numpy() if wh else r["last"].cpu().numpy()
                assert np.abs(got - (ref if wh else ref[:, -1])).max() < tol


@pytest.mark.parametrize("precision", ["bf16", "fp32"])
@pytest.mark.parametrize("name", ["micro", "tiny"])
def test_encoder_forward_split(T, gww, name, precision):
    """Batches 64 and 65 as two half batches on two streams (set_split): the workspace is the two halves' layouts."""
    enc, _ = _encoder(name, precision)
    enc = enc.cuda()
    enc.set_split(True)
    d, L, H, F = ENCODERS[name]
    plain, _ = _encoder(name, precision)
    plain = plain.cuda()
    for B in (64, 65):
        mel = _dev(T, _features(43, B))
        for wh, wl in ((True, False), (False, True)):
            r = run_contract(_forward_case(T, enc, mel, wh, wl, precision), arena_row_bytes=encoder_arena_row_bytes(d, F))
            want = plain.forward_raw(mel, want_hidden=wh, want_last=wl)[0 if wh else 1]
            assert T.equal(r["hidden" if wh else "last"], want), "split and unsplit forwards differ"


@pytest.mark.parametrize("precision", ["bf16", "fp32"])
@pytest.mark.parametrize("name", ["micro", "tiny"])
def test_encoder_forward_outputs(T, gww, name, precision):
    """gww_encoder_forward_outputs at B = 1 and 3 with the hidden and attention slabs each on and off; with the hidden slab
    and last_hidden NULL (the C entry point called directly) slab layer L is written directly.  A slab that was not
    requested is a NULL pointer: there is nothing to touch.  last_hidden is bit-identical to gww_encoder_forward's."""
    from gw_whisper_amd._lib import lib
    enc, _ = _encoder(name, precision, seed=5)
    enc = enc.cuda()
    d, L, H, F = ENCODERS[name]
    Tn = 1500
    for B in (1, 3):
        mel = _dev(T, _features(41, B))
        plain = enc.forward_raw(mel)[0].clone()
        for want_h, want_a in ((True, False), (False, True), (True, True), (False, False)):
            if want_a and name == "tiny" and B == 3:
                continue            # [4, 3, 6, 1500, 1500] fp32 four times over: the B = 1 maps cover the kernel

            def case(g):
                enc._ws = None
                pm = g.place(mel)
                last, hs, at = enc.forward_outputs_raw(pm, want_h, want_a)
                assert g.owns(enc._ws)
                out = {"last": last}
                if hs is not None:
                    out.update({f"hidden{i}": t for i, t in enumerate(hs)})
                    slab = g.empty((L + 1, B, Tn, d), T.float32)
                    _ok(lib().gww_encoder_forward_outputs(enc._handle, pm.data_ptr(), B, _prec(precision), enc._ws.data_ptr(),
                                                          enc._ws.numel(), None, slab.data_ptr(), None, _stream(T)),
                        "gww_encoder_forward_outputs")
                    out["slab_without_last_hidden"] = slab
                if at is not None:
                    out.update({f"attn{i}": t for i, t in enumerate(at)})
                return out
            r = run_contract(case, arena_row_bytes=encoder_arena_row_bytes(d, F))
            assert T.equal(r["last"], plain)
            if want_h:
                assert T.equal(r["slab_without_last_hidden"], T.stack([r[f"hidden{i}"] for i in range(L + 1)]))
                assert T.equal(r[f"hidden{L}"], plain)
            del r


# ------------------------------------------------------------------ training step
MODES = {"dora_qkv": dict(precision="bf16", r=8, dora=True, projs=QKV),
         "all_r1": dict(precision="bf16", r=1, dora=True, projs=ALL),
         "all_r12": dict(precision="bf16", r=12, dora=True, projs=ALL),
         "all_r64": dict(precision="bf16", r=64, dora=True, projs=ALL),
         "lora": dict(precision="bf16", r=8, dora=False, projs=QKV),
         "full": dict(precision="bf16", full=True),
         "fp32": dict(precision="fp32", r=8, dora=True, projs=QKV)}
# the r = 8 attention-only bf16 step sums its adapter gradients with float atomics (train_ops.hip k_dora_grads, k_dora_reduce's
# dm): the run-to-run bound of test_gpu_training.py::test_gradients_accumulate_into_existing_grad_buffers
ATOMIC_MODES = {"dora_qkv": 1e-4, "lora": 1e-4}


def _train_model(T, name, mode, freeze_stem=False):
    """(model, encoder, [(name, trainable parameter)]) of one training mode, adapters initialised away from B = 0."""
    from gw_whisper_amd.peft import LoraConfig, get_peft_model
    m = MODES[mode]
    d, L, H, F = ENCODERS[name]
    enc, sd = _encoder(name, m["precision"])
    if m.get("full"):
        enc = enc.cuda()
        enc.enable_full_finetune()
        for n, p in enc.named_parameters():
            p.requires_grad = not (freeze_stem and n.startswith("conv"))
        return enc, enc, [(n, p) for n, p in enc.named_parameters() if p.requires_grad]
    targets = [f"layers.{i}.{p}" for i in range(L) for p in m["projs"]]
    peft = get_peft_model(enc, LoraConfig(use_dora=m["dora"], r=m["r"], lora_alpha=32, target_modules=targets)).cuda()
    with T.no_grad():
        for j, tname in enumerate(targets):
            lin = peft.base_model.model.get_submodule(tname)
            W0 = sd[tname + ".weight"]
            A, Bm, mag = synth.dora_adapter(W0.shape[0], W0.shape[1], m["r"], W0, seed=70 + j)
            lin.lora_A["default"].weight.copy_(T.from_numpy(A))
            lin.lora_B["default"].weight.copy_(T.from_numpy(Bm))
            if m["dora"]:
                lin.lora_magnitude_vector["default"].weight.copy_(T.from_numpy(mag))
    return peft, enc, [(n, p) for n, p in peft.named_parameters() if p.requires_grad]


def _expected_train_bytes(enc, mode, B):
    from gw_whisper_amd._lib import lib
    h, m = enc._handle, MODES[mode]
    if m["precision"] == "fp32":
        return lib().gww_train_workspace_bytes_f32(h, B), lib().gww_train_saved_bytes_f32(h, B)
    if m.get("full"):
        ws = lib().gww_train_workspace_bytes_full(h, B)
    elif m["projs"] is ALL or m["r"] != 8:
        ws = lib().gww_train_workspace_bytes_adapters(h, B, m["r"])
    else:
        ws = lib().gww_train_workspace_bytes(h, B)
    return ws, lib().gww_train_saved_bytes(h, B)


def _step_case(T, model, enc, params, mode, mel, wl, pooled, want_mel, repoison=False):
    """One training step: the gradient buffers are guarded zeros the backward accumulates into; ws and saved are what
    training.py allocates (exactly the queried bytes, poisoned by the guard before the forward)."""
    def case(g):
        for _, p in params:
            p.grad = g.zeros(tuple(p.shape), T.float32)
        mel_t = g.place(mel).requires_grad_(want_mel)
        out = model.last_token(mel_t) if pooled else model(mel_t).last_hidden_state
        node = out.grad_fn
        ws, saved = node.ws, node.saved
        assert g.owns(ws) and g.owns(saved) and g.owns(out), "ws / saved / hidden did not come from the guard"
        assert (ws.numel(), saved.numel()) == _expected_train_bytes(enc, mode, mel.shape[0])
        if repoison:
            g.repoison(ws)            # include/gww.h: `workspace` is scratch, `saved` carries the activations
        (out * wl).sum().backward()
        res = {"hidden": out.detach()}
        for n, p in params:
            assert g.owns(p.grad), n
            res[n] = p.grad
        if want_mel:
            d_mel = mel_t.grad
            if isinstance(g, Guard):
                recs = g.allocations(site="training.py", shape=tuple(mel.shape), kind="empty")
                assert recs, "d_mel was not allocated under the guard"
                d_mel = g.interior(recs[-1])
                assert T.equal(d_mel, mel_t.grad)
            res["d_mel"] = d_mel
        for _, p in params:
            p.grad = None
        return res
    return case


def _run_step(T, name, mode, pooled, want_mel, repoison=False, fills=FILLS, freeze_stem=False):
    model, enc, params = _train_model(T, name, mode, freeze_stem)
    d, L, H, F = ENCODERS[name]
    mel = _dev(T, olm.log_mel(synth.strain_segments(2, seed=33)))
    g_ = T.Generator().manual_seed(7)
    wl = T.randn((2, d) if pooled else (2, 1500, d), generator=g_).cuda()
    atomic = {n: ATOMIC_MODES[mode] for n, _ in params} if mode in ATOMIC_MODES else None
    r = run_contract(_step_case(T, model, enc, params, mode, mel, wl, pooled, want_mel, repoison),
                     arena_row_bytes=encoder_arena_row_bytes(d, F), atomic=atomic, fills=fills)
    assert float(r["hidden"].std()) > 0 and any(float(r[n].abs().max()) > 0 for n, _ in params)
    return r


@pytest.mark.parametrize("want_mel", [False, True], ids=["", "d_mel"])
@pytest.mark.parametrize("pooled", [False, True], ids=["hidden", "pooled"])
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("name", ["micro", "tiny"])
def test_training_step(T, gww, name, mode, pooled, want_mel):
    _run_step(T, name, mode, pooled, want_mel)


@pytest.mark.parametrize("pooled,want_mel", [(True, True), (False, False)], ids=["pooled-d_mel", "hidden"])
@pytest.mark.parametrize("mode", ["dora_qkv", "full"])
@pytest.mark.parametrize("name", ["base_l2", "small_l2", "medium_l2"])
def test_training_step_wider_encoders(T, gww, name, mode, pooled, want_mel):
    _run_step(T, name, mode, pooled, want_mel)


@pytest.mark.parametrize("pooled", [False, True], ids=["hidden", "pooled"])
@pytest.mark.parametrize("name,mode", [(n, m) for n in ("micro", "tiny") for m in MODES]
                         + [("base_l2", m) for m in ("dora_qkv", "full", "fp32")])     # (the per-op path: three modes)
def test_training_workspace_is_scratch_between_forward_and_backward(T, gww, name, mode, pooled):
    """include/gww.h: `saved` carries the activations from the forward to the backward and `workspace` is scratch between
    the two calls -- unless the backward is asked for d_mel or a conv-stem gradient, which it forms from the stem's
    transposed input and conv1 output the forward left at the front of the workspace (this test found that dependence with
    d_mel requested: the header said "scratch" without the exception, and says it now).  So: no d_mel, the stem frozen in
    the full fine-tuning mode, the whole workspace re-poisoned between the two calls, and no gradient may change."""
    _run_step(T, name, mode, pooled, False, repoison=True, fills=(0xFF, 0x7F), freeze_stem=True)


# ------------------------------------------------------------------ undersized workspaces
def test_undersized_workspaces_are_refused_before_any_launch(T, gww):
    """Every *_bytes-sized argument one byte short: GWW_ERR_WORKSPACE (-3) from the host check, gww_last_error() naming the
    entry point.  Every buffer handed over has its full size all the same: nothing is ever launched on less.  (The
    adapter-gradient scratch is optional by contract -- a short one makes the call use library-owned memory -- and has no
    such check.  gww_head_backward_f32 refuses as the detection and binary heads' backward do, through the argument check of
    the shared host path: GWW_ERR_ARG (-1) and "workspace" in the text.)"""
    from gw_whisper_amd import _lib
    from gw_whisper_amd.qscan import QTransformAdapter
    L = _lib.lib()
    st = _stream(T)
    keep = []                                                  # every buffer stays alive to the end of the test

    def u8(n):
        keep.append(T.empty((n,), dtype=T.uint8, device="cuda"))
        return keep[-1]

    def f32(*shape):
        keep.append(T.zeros(shape, device="cuda"))
        return keep[-1]

    def refused(rc, name):
        msg = L.gww_last_error().decode()
        assert rc == -3 and name in msg, (name, rc, msg)

    d, Ly, H, F = ENCODERS["micro"]
    for precision in ("bf16", "fp32"):
        enc, _ = _encoder("micro", precision)
        enc = enc.cuda()
        prec = _prec(precision)
        mel = _dev(T, _features(1, 64))
        enc.forward_raw(mel[:2])                                     # weights packed, handle ready
        h = enc._handle
        for split, B in ((False, 2), (True, 64)):
            enc.set_split(split)
            need = L.gww_encoder_workspace_bytes(h, B, prec)
            ws, hid = u8(need), f32(B, 1500, d)
            refused(L.gww_encoder_forward(h, mel.data_ptr(), B, prec, ws.data_ptr(), need - 1, hid.data_ptr(), None, st),
                    "gww_encoder_forward")
            refused(L.gww_encoder_forward_outputs(h, mel.data_ptr(), B, prec, ws.data_ptr(), need - 1, hid.data_ptr(), None,
                                                  None, st), "gww_encoder_forward")
        enc.set_split(False)
        B = 2
        sfx = "_f32" if precision == "fp32" else ""
        need_ws = getattr(L, "gww_train_workspace_bytes" + sfx)(h, B)
        need_sv = getattr(L, "gww_train_saved_bytes" + sfx)(h, B)
        need_full = L.gww_train_workspace_bytes_full(h, B)
        ws, sv, hid = u8(max(need_ws, need_full)), u8(need_sv), f32(B, 1500, d)
        fwd, bwd = getattr(L, "gww_encoder_train_forward" + sfx), getattr(L, "gww_encoder_train_backward" + sfx)
        for wb, sb in ((need_ws - 1, need_sv), (need_ws, need_sv - 1)):
            refused(fwd(h, mel.data_ptr(), B, ws.data_ptr(), wb, sv.data_ptr(), sb, hid.data_ptr(), 0, st),
                    "gww_encoder_train_forward" + sfx)
            refused(bwd(h, B, ws.data_ptr(), wb, sv.data_ptr(), sb, hid.data_ptr(), None, 0, None, None, 0, st),
                    "gww_encoder_train_backward" + sfx)
        if precision == "bf16":
            assert need_full > need_ws
            grads = _lib.EncGrads()
            refused(L.gww_encoder_train_backward_full(h, B, ws.data_ptr(), need_full - 1, sv.data_ptr(), need_sv, hid.data_ptr(),
                                                      None, 0, None, None, 0, C.byref(grads), st),
                    "gww_encoder_train_backward_full")
    # weight-gradient GEMM, LayerNorm parameter gradients
    M, N, K = 3001, 128, 512
    dy, x = T.zeros((M, N), dtype=T.bfloat16, device="cuda"), T.zeros((M, K), dtype=T.bfloat16, device="cuda")
    need = L.gww_gemm_wgrad_workspace_bytes(M, N, K)
    assert need > 0
    refused(L.gww_gemm_wgrad_bf16(dy.data_ptr(), N, x.data_ptr(), K, M, N, K, 1.0, f32(N, K).data_ptr(), None,
                                  u8(need).data_ptr(), need - 1, st), "gemm_wgrad")
    need = L.gww_layernorm_param_grads_workspace_bytes(M, 128)
    refused(L.gww_layernorm_param_grads(f32(M, 128).data_ptr(), f32(M, 128).data_ptr(), 1, M, 128, f32(128).data_ptr(),
                                        f32(128).data_ptr(), u8(need).data_ptr(), need - 1, st), "ln_param_grads")
    # Q-adapter CNN and tail backward
    ad = QTransformAdapter.train_variant().cuda()
    packed, (c1, c2, c3) = ad._packed_cnn()
    B, hw = 1, 128
    q, y = f32(B, hw, hw), f32(B, hw // 4, hw // 4)
    need = L.gww_qadapter_cnn_workspace_bytes(B, hw, hw, c1, c2)
    refused(L.gww_qadapter_cnn_forward_f32(q.data_ptr(), B, hw, hw, packed.data_ptr(), c1, c2, c3, u8(need).data_ptr(), need - 1,
                                           y.data_ptr(), st), "gww_qadapter_cnn_forward_f32")
    ps = [p.detach().float().contiguous() for p in ad._cnn_params()]
    gr = [T.zeros_like(p) for p in ps]
    need = L.gww_qadapter_cnn_backward_workspace_bytes(B, hw, hw, c1, c2, c3)
    refused(L.gww_qadapter_cnn_backward_f32(q.data_ptr(), y.data_ptr(), B, hw, hw, packed.data_ptr(), ps[2].data_ptr(),
                                            ps[4].data_ptr(), c1, c2, c3, u8(need).data_ptr(), need - 1,
                                            *[t.data_ptr() for t in gr], st), "gww_qadapter_cnn_backward_f32")
    Bt, Hin, Win, F_, Tn = 2, 32, 32, 80, 3000
    need = L.gww_qadapter_tail_backward_workspace_bytes(Bt, Hin)
    one = f32(4)
    refused(L.gww_qadapter_tail_backward_f32(f32(Bt, F_, Tn).data_ptr(), F_ * Tn, f32(Bt, Hin, Win).data_ptr(), Bt, Hin, Win, F_, Tn,
                                             one.data_ptr(), one.data_ptr(), one.data_ptr(), f32(Bt, Hin, Win).data_ptr(),
                                             u8(need).data_ptr(), need - 1, one.data_ptr(), one.data_ptr(), one.data_ptr(),
                                             one.data_ptr(), st), "gww_qadapter_tail_backward_f32")
    # glitch head backward
    from gw_whisper_amd import ops
    B, d_in, Cc = 5, 128, 3
    dims = (d_in, *ops.HEAD_WIDTHS, Cc)
    params = [f32(*s) for i in range(4) for s in ((dims[i + 1], dims[i]), (dims[i + 1],))]
    *_, (x, ps, hs, dz, p, train) = ops.head_forward(f32(B, d_in), params, T.zeros((B,), dtype=T.int64, device="cuda"))
    need = L.gww_head_workspace_bytes(B, Cc)
    ws, dx, grads = u8(need), f32(B, d_in), [f32(*t.shape) for t in ps]
    P, A, G = ops._mlp_blocks(ps, hs, None, grads)
    for nbytes, rc in ((need - 1, -1), (need, 0)):
        assert L.gww_head_backward_f32(x.data_ptr(), P, A, dz.data_ptr(), None, B, d_in, Cc, p, int(train), ws.data_ptr(), nbytes,
                                       dx.data_ptr(), G, st) == rc
        msg = L.gww_last_error().decode()
        assert rc == 0 or ("gww_head_backward_f32" in msg and "workspace" in msg), msg
    T.cuda.synchronize()
