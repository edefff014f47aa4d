"""Memory contract of the entry points of csrc/score.hip (the pattern of tests/test_gpu_roc_contract.py): every
caller-visible buffer is allocated under tests/guard.py's guard-band allocator, each case runs under the three fill bytes
and unguarded, and must leave every band intact, write every element its contract says it writes -- the leading
``counts`` entries of the compacted buffers, the first F of a sort under a device count --, and give the same bits whatever
lies outside its buffers.  The wrappers allocate the workspaces at exactly the bytes their ``*_workspace_bytes``
functions advertise; an undersized workspace is refused before any launch."""

import numpy as np
import pytest

from tests.guard import FILLS, Guard, run_contract

from . import search_score_helpers as sh

pytestmark = pytest.mark.gpu

MODULES = ("gw_whisper_amd.ops", "gw_whisper_amd.search_score")


@pytest.fixture(scope="module")
def T():
    import torch
    assert torch.cuda.is_available()
    return torch


def _inputs(n):
    # at least two injections: with one, the reference's own chirp-weighted variance cancels to +-0 and may come out NaN
    fg, bg, inj, duration = sh.make_case(n, n, max(2, n // 3), 5200 + n)
    mc = (inj["mass1"] * inj["mass2"]) ** 0.6 / (inj["mass1"] + inj["mass2"]) ** 0.2
    return fg, bg, inj, duration, mc ** 2.5, mc ** 5


@pytest.mark.parametrize("n", [2, 65, 4097])
def test_score_entry_points(T, gww, n):
    from gw_whisper_amd import ops, search_score
    fg, bg, inj, duration, w1, w2 = _inputs(n)
    N = len(inj["tc"])
    fg_d, bg_d, tc_d, w1_d, w2_d = (T.from_numpy(np.ascontiguousarray(a)).cuda() for a in (fg, bg, inj["tc"], w1, w2))
    stats = []

    def case(g):
        ev, tc = g.place(fg_d), g.place(tc_d)
        order, times, nan_t = ops.score_sort(ev[0])
        m = ops.score_match(ev, order, tc)
        c = m["counts"]
        n_tp, n_fp, n_f, n_m, _ = (int(v) for v in c.cpu().numpy())
        fg_far = ops.score_far(n, duration, "cuda", n_dev=c[1:2])
        f_order, f_sorted, nan_f = ops.score_sort(m["found_stat"], n_dev=c[2:3])
        _, noise, nan_b = ops.score_sort(g.place(bg_d[1]))
        far = ops.score_far(n, duration, "cuda")
        cs1, cs2 = ops.score_suffix(g.place(w1_d), g.place(w2_d), m["found_inj"], f_order, c[2:3])
        nf, frac, vol, err = ops.score_volume(f_sorted, c[2:3], noise, float(N), 2.5, None, None)
        nf_c, frac_c, vol_c, err_c = ops.score_volume(f_sorted, c[2:3], noise, 1.25 * N, 2.5, cs1, cs2)
        idx, diff = ops.score_closest(tc, g.place(bg_d[0]))
        stats.append(search_score.get_stats(g.place(fg_d), g.place(bg_d), inj, duration, chirp_distance=True))
        out = {"order": order, "times": times, "nan_t": nan_t, "fg_sorted": m["fg_sorted"], "found_idx": m["found_idx"],
               "tp_idx": m["tp_idx"][:n_tp], "tp_diff": m["tp_diff"][:n_tp], "tp_events": m["tp_events"][:, :n_tp],
               "found_inj": m["found_inj"][:n_f], "found_stat": m["found_stat"][:n_f], "counts": c, "f_order": f_order[:n_f],
               "f_sorted": f_sorted[:n_f], "nan_f": nan_f, "noise": noise, "nan_b": nan_b, "far": far, "cs1": cs1[:n_f + 1],
               "cs2": cs2[:n_f + 1], "nfound": nf, "frac": frac, "vol": vol, "err": err, "nfound_c": nf_c, "frac_c": frac_c,
               "vol_c": vol_c, "err_c": err_c, "idx": idx, "diff": diff}
        if n_fp:
            out.update({"fp_idx": m["fp_idx"][:n_fp], "fp_diff": m["fp_diff"][:n_fp], "fp_events": m["fp_events"][:, :n_fp],
                        "fg_far": fg_far[:n_fp]})
        if n_m:
            out["missed"] = m["missed"][:n_m]
        return out
    r = run_contract(case, modules=MODULES)
    ref = sh.restate(fg, bg, inj, duration)
    assert np.array_equal(r["order"].cpu().numpy(), ref["sorting-indices"])
    assert np.array_equal(r["found_idx"].cpu().numpy(), ref["found-indices"])
    assert np.array_equal(r["tp_idx"].cpu().numpy(), ref["true-positive-event-indices"])
    assert np.array_equal(r["nfound"].cpu().numpy(), np.round(ref["sensitive-fraction"] * N))
    assert int(r["counts"][2]) == ref["_F"]
    assert len(stats) == len(FILLS) + 1
    chirp = sh.restate(fg, bg, inj, duration, True)
    for s in stats:
        sh.compare(s, chirp, True, "guarded get_stats vs restatement")
        assert all(np.array_equal(s[k], stats[-1][k]) for k in s), "get_stats depends on bytes outside its buffers"


def test_undersized_workspaces_are_refused_before_any_launch(T, gww):
    """One byte short: GwwError, and neither the outputs nor the workspace are touched."""
    from gw_whisper_amd import ops
    n = 65
    fg, bg, inj, duration, w1, w2 = _inputs(n)
    L = gww.lib()
    with Guard(FILLS[0], modules=MODULES) as g:
        ev, tc = g.place(T.from_numpy(fg).cuda()), g.place(T.from_numpy(inj["tc"]).cuda())
        order, _, _ = ops.score_sort(ev[0])
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
        refused(lambda ws: ops.score_sort(ev[0], ws=ws), L.gww_score_sort_workspace_bytes(n))
        refused(lambda ws: ops.score_match(ev, order, tc, ws=ws), L.gww_score_match_workspace_bytes(n, len(inj["tc"])))
        g.check()
