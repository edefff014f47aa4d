"""Memory contract of the entry points of csrc/detect.hip (the pattern of
tests/test_gpu_memory_contract.py::test_head_step): every caller-visible buffer is allocated under tests/guard.py's
guard-band allocator, each case runs under the three fill bytes and unguarded, and must leave every band intact, write
every element its contract says it writes, and give the same bits whatever lies outside its buffers.  The wrappers
allocate the backward workspace at exactly ``gww_det_head_workspace_bytes`` and the selection workspace at exactly
``gww_score_thresholds_workspace_bytes``; an undersized workspace is refused before any launch."""

import numpy as np
import pytest

from tests.guard import FILLS, Guard, run_contract

from . import efficiency_helpers as eh

pytestmark = pytest.mark.gpu

MODULES = ("gw_whisper_amd.ops", "gw_whisper_amd.efficiency")


@pytest.fixture(scope="module")
def T():
    import torch
    assert torch.cuda.is_available()
    return torch


def _case(T, d_in, C, B, seed):
    x, t = eh.case_inputs(d_in, C, B, seed)
    params = [T.from_numpy(p).cuda() for p in eh.case_params(seed % 7, d_in, C)]
    return T.from_numpy(x).cuda(), T.from_numpy(t).cuda(), params


@pytest.mark.parametrize("B,C,d_in", [(1, 2, 128), (7, 3, 384), (33, 64, 1280), (257, 2, 512)])
def test_det_head_step(T, gww, B, C, d_in):
    """Forward, backward with ws at gww_det_head_workspace_bytes (the wrapper), scores into a strided slice of a guarded
    buffer, and the evaluation accumulate into guarded int64 / fp64 state."""
    from gw_whisper_amd import efficiency, ops
    x, t, params = _case(T, d_in, C, B, 40 + B)
    up = T.tensor([0.37], device="cuda")

    def case(g):
        pp = [g.place(p) for p in params]
        xx, tt = g.place(x), g.place(t)
        loss, logits, probs, row_loss, saved = ops.det_head_forward(xx, pp, tt, 1e-6)
        dx, grads = ops.det_head_backward(saved, g.place(up))
        state = efficiency.EvalState("cuda")
        for lo, hi in ((0, B // 2), (B // 2, B)):
            if hi > lo:
                state.add(probs[lo:hi], tt[lo:hi], row_loss[lo:hi])
        out = {"loss": loss, "logits": logits, "probs": probs, "row_loss": row_loss, "dz": saved[3], "dx": dx,
               "correct": state.correct, "loss_sum": state.loss_sum, "n": state.n, "batches": state.batches}
        out.update({f"h{i}": h for i, h in enumerate(saved[2])})
        out.update({f"g{i}": gr for i, gr in enumerate(grads)})
        # one score per row into every third element of a zeroed buffer: the elements between stay zero
        for mode in ((ops.SCORE_PROB0, ops.SCORE_LOGIT_DIFF) if C == 2 else (ops.SCORE_PROB0,)):
            buf = g.zeros((3 * B + 2,), T.float32)
            ops.det_head_scores(xx, pp, buf[1:1 + 3 * B:3], mode)
            out[f"scores{mode}"] = buf
        return out
    r = run_contract(case, modules=MODULES)
    assert int(r["n"]) == B and int(r["batches"]) == (1 if B == 1 else 2)
    assert int(r["correct"]) == int((r["probs"].argmax(1) == t.argmax(1)).sum())
    assert T.equal(r[f"scores{ops.SCORE_PROB0}"][1::3][:B], r["probs"][:, 0])
    rest = T.ones(3 * B + 2, dtype=T.bool, device="cuda")
    rest[1:1 + 3 * B:3] = False
    assert not bool(r[f"scores{ops.SCORE_PROB0}"][rest].any())
    if C == 2:
        assert T.equal(r[f"scores{ops.SCORE_LOGIT_DIFF}"][1::3][:B], r["logits"][:, 0] - r["logits"][:, 1])


@pytest.mark.parametrize("N,F", [(1, 1), (257, 5), (70001, 8)])
def test_selection_and_counts(T, gww, N, F):
    """Thresholds (workspace from the wrapper, at exactly the documented size) and counts into one row of a guarded
    [3, F] table."""
    from gw_whisper_amd import ops
    rng = np.random.default_rng(N)
    a = rng.standard_normal(N).astype(np.float32)
    ranks = np.concatenate(([0, 1, N], rng.integers(0, N + 1, 5)))[:F].astype(np.int64)
    scores, ranks_d = T.from_numpy(a).cuda(), T.from_numpy(ranks).cuda()

    def case(g):
        s = g.place(scores)
        thr = ops.score_thresholds(s, g.place(ranks_d))
        table = g.zeros((3, F), T.int64)
        ops.detection_counts(s, thr, table[1])
        ops.detection_counts(s[:max(N // 2, 1)], thr, table[1])
        return {"thr": thr, "table": table}
    r = run_contract(case, modules=MODULES)
    srt = np.sort(a)
    ref = np.asarray([srt[N - k] if k > 0 else srt[0] for k in ranks], np.float32)
    assert np.array_equal(r["thr"].cpu().numpy(), ref)
    cnt = (a[:, None] > ref[None]).sum(0) + (a[:max(N // 2, 1), None] > ref[None]).sum(0)
    assert np.array_equal(r["table"].cpu().numpy(), np.stack([np.zeros(F, np.int64), cnt, np.zeros(F, np.int64)]))


def test_undersized_workspaces_are_refused_before_any_launch(T, gww):
    """One float short: GwwError, and neither the outputs nor the workspace are touched."""
    from gw_whisper_amd import ops
    x, t, params = _case(T, 128, 2, 5, 3)
    with Guard(FILLS[0], modules=MODULES) as g:
        _, _, _, _, saved = ops.det_head_forward(g.place(x), [g.place(p) for p in params], g.place(t))
        need = gww.lib().gww_det_head_workspace_bytes(5, 2)
        ws = g.empty((need // 4 - 1,), T.float32)
        n_before = len(g.records)
        with pytest.raises(gww.GwwError, match="workspace"):
            ops.det_head_backward(saved, None, ws=ws)
        T.cuda.synchronize()
        assert g.unwritten(ws) == ws.numel()
        for rec in g.records[n_before:]:                 # dx and the ten gradients the wrapper had allocated
            assert g.unwritten(g.interior(rec)) == g.interior(rec).numel(), rec.describe()
        sel = g.empty((gww.lib().gww_score_thresholds_workspace_bytes() // 8 - 1,), T.int64)
        n_before = len(g.records)
        with pytest.raises(gww.GwwError, match="workspace"):
            ops.score_thresholds(g.place(T.randn(100, device="cuda")), g.place(T.tensor([1, 5], device="cuda")), ws=sel)
        T.cuda.synchronize()
        assert g.unwritten(sel) == sel.numel()
        thr = [rec for rec in g.records[n_before:] if rec.shape == (2,) and rec.kind == "empty"]
        assert thr and all(g.unwritten(g.interior(rec)) == 2 for rec in thr)
        g.check()
