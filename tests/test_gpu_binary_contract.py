"""Memory contract of the binary head's launchers (csrc/binary_head.hip; the pattern of
tests/test_gpu_cnn_head_contract.py): every caller-visible buffer -- the saved activations, logits, probs, row_loss, dz,
loss, the scores' logits, dx, every gradient and the workspace at exactly ``gww_bin_head_workspace_bytes`` -- is allocated
under tests/guard.py's guard-band allocator.  Each case runs under the three fill bytes and unguarded, must leave every
band intact, write every element of its outputs (the workspace included: it is the layers' dz, all of it), and give the
same bits whatever the buffers held before and whatever lies outside them.  An undersized workspace is refused before any
launch."""

import pytest

from tests import binary_helpers as bh
from tests.guard import run_contract

pytestmark = pytest.mark.gpu

MODULES = ("gw_whisper_amd.ops",)


@pytest.fixture(scope="module")
def T():
    import torch
    assert torch.cuda.is_available()
    return torch


def _case(T, layout, d_in, C, B, seed):
    from gw_whisper_amd import synth
    sd = synth.head_state_dict([d_in, *bh.WIDTHS[layout], C], seed=seed)
    params = [T.from_numpy(sd[k]).cuda() for k in bh.param_keys(layout)]
    x, t = bh.case_inputs(d_in, C, B, seed + 1)
    return params, T.from_numpy(x).cuda(), T.from_numpy(t).cuda()


@pytest.mark.parametrize("layout,d_in,C,B", [(bh.ONE, 128, 1, 3), (bh.TWO, 256, 64, 33), (bh.TWO, 1536, 1, 2)])
def test_binary_head_forward_scores_and_backward(T, gww, layout, d_in, C, B):
    """(TWO, 256, 64, 33): the widest last layer and a ragged third row block; (TWO, 1536, 1, 2): x walked in three chunks."""
    from gw_whisper_amd import ops
    from gw_whisper_amd._lib import lib
    params, x, t = _case(T, layout, d_in, C, B, seed=41)
    up = T.tensor([0.37], device="cuda")
    need = lib().gww_bin_head_workspace_bytes(layout, B, C)
    assert need == 4 * B * (sum(bh.WIDTHS[layout]) + C)

    def case(g):
        pp = [g.place(p) for p in params]
        xx = g.place(x)
        loss, logits, probs, row_loss, saved = ops.bin_head_forward(layout, xx, pp, g.place(t))
        scores = ops.bin_head_scores(layout, xx, pp)
        ws = g.empty((need // 4,), T.float32)
        dx, grads = ops.bin_head_backward(saved, g.place(up), ws=ws)
        out = {"loss": loss, "logits": logits, "probs": probs, "row_loss": row_loss, "dz": saved[4], "scores": scores,
               "dx": dx, "ws": ws}
        out.update({f"h{i}": h for i, h in enumerate(saved[3])})
        out.update({f"g{i}": gr for i, gr in enumerate(grads)})
        return out
    r = run_contract(case, arena_row_bytes=4 * max(d_in, 1024), modules=MODULES)
    assert T.equal(r["scores"], r["logits"])
    assert tuple(r["dx"].shape) == (B, d_in) and tuple(r["logits"].shape) == (B, C)
    for i, p in enumerate(params):
        assert r[f"g{i}"].shape == p.shape
    # the workspace ends with the last layer's dz = 0.37 * dz of the forward
    assert T.equal(r["ws"][-B * C:].reshape(B, C), r["dz"] * up)


def test_undersized_workspace_is_refused_before_any_launch(T, gww):
    from gw_whisper_amd import GwwError, ops
    from gw_whisper_amd._lib import lib
    for layout, d_in, C, B in ((bh.ONE, 128, 1, 3), (bh.TWO, 256, 2, 5)):
        params, x, t = _case(T, layout, d_in, C, B, seed=43)
        *_, saved = ops.bin_head_forward(layout, x, params, t)
        need = lib().gww_bin_head_workspace_bytes(layout, B, C)
        assert need % 4 == 0
        with pytest.raises(GwwError, match="gww_bin_head_backward_f32"):
            ops.bin_head_backward(saved, ws=T.empty((need // 4 - 1,), device="cuda"))
        assert lib().gww_last_error().decode().count("workspace")
        ops.bin_head_backward(saved, ws=T.empty((need // 4,), device="cuda"))
    T.cuda.synchronize()
