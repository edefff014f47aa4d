"""Memory contract of the CNN head's launchers (csrc/cnn_head.hip; the pattern of tests/test_gpu_memory_contract.py): every
caller-visible buffer -- logits, the saved activations, dx, the eight gradients and the workspace at exactly
``gww_cnn_head_workspace_bytes`` -- is allocated under tests/guard.py's guard-band allocator.  Each case runs under the
three fill bytes and unguarded, must leave every band intact, write every element of its outputs, and give the same
bits whatever the workspace held before and whatever lies outside its buffers.  An undersized workspace is refused before
any launch."""

import pytest

from tests.guard import run_contract
from tests.test_gpu_cnn_head import chain_params, make_chain, make_input

pytestmark = pytest.mark.gpu

MODULES = ("gw_whisper_amd.ops",)


@pytest.fixture(scope="module")
def T():
    import torch
    assert torch.cuda.is_available()
    return torch


@pytest.mark.parametrize("B,d,C", [(3, 128, 1), (2, 384, 3), (33, 128, 64)])
def test_cnn_head_forward_and_backward(T, gww, B, d, C):
    """(33, 128, 64): more samples than the weight-gradient partials have slices (two samples per slice, one in the last),
    and the widest Linear."""
    from gw_whisper_amd import ops
    params = [t.cuda() for t in chain_params(make_chain(T, C, seed=1))]
    x = make_input(T, B, d, seed=2).cuda()
    gen = T.Generator().manual_seed(3)
    dl = T.randn(B, C, generator=gen).cuda()

    def case(g):
        pp = [g.place(p) for p in params]
        xx = g.place(x)
        infer = ops.cnn_head_forward(xx, pp)
        logits, saved = ops.cnn_head_forward(xx, pp, train=True)
        dx, grads = ops.cnn_head_backward(saved, g.place(dl))
        out = {"infer": infer, "logits": logits, "acts": saved[2], "dx": dx}
        out.update({f"g{i}": t for i, t in enumerate(grads)})
        return out
    r = run_contract(case, arena_row_bytes=4 * d, modules=MODULES)
    assert T.equal(r["infer"], r["logits"])
    assert tuple(r["acts"].shape) == (B, 448, d) and tuple(r["dx"].shape) == (B, 2, d)
    for i, p in enumerate(params):
        assert r[f"g{i}"].shape == p.shape


def test_undersized_workspace_is_refused_before_any_launch(T, gww):
    from gw_whisper_amd import GwwError, ops
    from gw_whisper_amd._lib import lib
    B, d, C = 2, 128, 3
    params = [t.cuda() for t in chain_params(make_chain(T, C, seed=1))]
    x = make_input(T, B, d, seed=2).cuda()
    _, saved = ops.cnn_head_forward(x, params, train=True)
    need = lib().gww_cnn_head_workspace_bytes(B, d, C)
    assert need % 4 == 0
    with pytest.raises(GwwError, match="gww_cnn_head_backward_f32"):
        ops.cnn_head_backward(saved, T.zeros(B, C, device="cuda"), ws=T.empty((need // 4 - 1,), device="cuda"))
    assert lib().gww_last_error().decode().count("workspace")
    ops.cnn_head_backward(saved, T.zeros(B, C, device="cuda"), ws=T.empty((need // 4,), device="cuda"))
    T.cuda.synchronize()
