"""Memory contract of the entry points of csrc/roc.hip (the pattern of tests/test_gpu_efficiency_contract.py): every
caller-visible buffer is allocated under tests/guard.py's guard-band allocator, each case runs under the three fill bytes
and unguarded, and must leave every band intact, write every element its contract says it writes -- the TPR rows of
invalid replicates included --, and give the same bits whatever lies outside its buffers.  The wrappers allocate the three
workspaces at exactly the bytes their ``*_workspace_bytes`` functions advertise; an undersized workspace is refused before
any launch."""

import numpy as np
import pytest

from tests.guard import FILLS, Guard, run_contract

from . import roc_helpers as rh

pytestmark = pytest.mark.gpu

MODULES = ("gw_whisper_amd.ops", "gw_whisper_amd.roc")


@pytest.fixture(scope="module")
def T():
    import torch
    assert torch.cuda.is_available()
    return torch


def _inputs(T, n):
    scores, labels = rh.saturating_scores(n, 2.0, 900 + n)
    labels[0], labels[1] = 1.0, 0.0
    scores[0], scores[1] = 0.75, 0.25
    rng = np.random.default_rng(n)
    idx = np.stack([rng.integers(0, n, n), np.arange(n), np.zeros(n, np.int64)]).astype(np.int32)   # the last one: no negative
    return scores, labels, idx


@pytest.mark.parametrize("n", [2, 65, "T+1"])
def test_roc_entry_points(T, gww, n):
    from gw_whisper_amd import ops, roc
    if n == "T+1":
        n = ops.ROC_TILE + 1
    scores, labels, idx = _inputs(T, n)
    s_d, l_d, i_d = (T.from_numpy(a).cuda() for a in (scores, labels, idx))
    grid_d = T.from_numpy(rh.GRID).cuda()
    logits = T.from_numpy(np.linspace(-6, 6, n).astype(np.float32)).cuda()

    def case(g):
        s, l = g.place(s_d), g.place(l_d)
        order, rank, pos, gend, G, n_nan = ops.roc_sort(s, l)
        fps, tps, fpr, tpr, counts, auc = ops.roc_curve(pos, gend, G)
        rows, valid = ops.roc_bootstrap_tpr(rank, pos, gend, G, g.place(i_d), g.place(grid_d))
        mean, std, n_valid = ops.roc_band(rows, valid)
        ng = int(G.item())
        state = roc.BinaryEvalState(n, "cuda")
        half = n // 2
        state.add(g.place(logits[:half]), l[:half], l[:half])
        state.add(g.place(logits[half:]), l[half:], l[half:])
        # the NaN rows of invalid replicates are part of the contract: compared (and checked as written) by their bits
        return {"order": order, "rank": rank, "pos": pos, "gend": gend[:ng], "G": G, "n_nan": n_nan, "fps": fps[:ng + 1],
                "tps": tps[:ng + 1], "fpr": fpr[:ng + 1], "tpr": tpr[:ng + 1], "counts": counts, "auc": auc,
                "rows_bits": rows.view(T.int64), "valid": valid, "mean": mean, "std": std, "n_valid": n_valid,
                "scores": state.scores, "loss_sum": state.loss_sum, "batches": state.batches, "confusion": state.confusion}
    r = run_contract(case, modules=MODULES)
    _, rr, rp, rg = rh.sort_desc(scores, labels)
    assert np.array_equal(r["rank"].cpu().numpy(), rr) and np.array_equal(r["gend"].cpu().numpy(), rg)
    ref, ref_valid = rh.bootstrap_rows(rr, rp, rg, idx)
    assert ref_valid[1] == 1 and ref_valid[2] == 0
    assert np.array_equal(r["valid"].cpu().numpy(), ref_valid)
    assert np.array_equal(r["rows_bits"].view(T.float64).cpu().numpy(), ref, equal_nan=True)
    mean, std = rh.band(ref, ref_valid)
    assert np.array_equal(r["mean"].cpu().numpy(), mean) and np.array_equal(r["std"].cpu().numpy(), std)
    assert int(r["n_valid"]) == int(ref_valid.sum()) and int(r["batches"]) == 2 and int(r["confusion"].sum()) == n


def test_undersized_workspaces_are_refused_before_any_launch(T, gww):
    """One byte short: GwwError, and neither the outputs nor the workspace are touched."""
    from gw_whisper_amd import ops
    n = 65
    scores, labels, idx = _inputs(T, n)
    L = gww.lib()
    with Guard(FILLS[0], modules=MODULES) as g:
        s, l = g.place(T.from_numpy(scores).cuda()), g.place(T.from_numpy(labels).cuda())
        order, rank, pos, gend, G, n_nan = ops.roc_sort(s, l)
        T.cuda.synchronize()

        def refused(call, need):
            ws = g.empty((need - 1,), T.uint8)
            before = len(g.records)
            with pytest.raises(gww.GwwError, match="workspace"):
                call(ws)
            T.cuda.synchronize()
            assert g.unwritten(ws) == ws.numel()
            new = g.records[before:]
            assert new, "the wrapper allocated its outputs before the call"
            for rec in new:
                assert g.unwritten(g.interior(rec)) == g.interior(rec).numel(), rec.describe()
        refused(lambda ws: ops.roc_sort(s, l, ws=ws), L.gww_roc_sort_workspace_bytes(n))
        refused(lambda ws: ops.roc_curve(pos, gend, G, ws=ws), L.gww_roc_curve_workspace_bytes(n))
        i_g, grid_g = g.place(T.from_numpy(idx).cuda()), g.place(T.from_numpy(rh.GRID).cuda())
        refused(lambda ws: ops.roc_bootstrap_tpr(rank, pos, gend, G, i_g, grid_g, ws=ws), L.gww_roc_bootstrap_workspace_bytes(3, n))
        g.check()
