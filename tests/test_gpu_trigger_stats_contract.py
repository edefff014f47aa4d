"""Memory contract of the entry points of csrc/trigger_stats.hip and of the two-column head (the pattern of
tests/test_gpu_search_score_contract.py): every caller-visible buffer is allocated under tests/guard.py's guard-band
allocator, each case runs under the three fill bytes and unguarded, and must leave every band intact, write every element
its contract says it writes -- the leading ``counts`` entries of the capacity-sized buffers --, and give the same bits
whatever lies outside its buffers or behind the device's count.  The wrappers allocate the workspaces at exactly the bytes
their ``*_workspace_bytes`` functions advertise; an undersized workspace is refused before any launch."""

import numpy as np
import pytest

from tests.guard import FILLS, Guard, run_contract

from . import trigger_stats_helpers as th

pytestmark = pytest.mark.gpu

MODULES = ("gw_whisper_amd.ops", "gw_whisper_amd.trigger_stats")


@pytest.fixture(scope="module")
def T():
    import torch
    assert torch.cuda.is_available()
    return torch


@pytest.mark.parametrize("n,dtype", [(1, "float64"), (257, "float32"), (4097, "float64"), (12305, "float64")])
def test_trigger_entry_points(T, gww, n, dtype):
    from gw_whisper_amd import ops
    from gw_whisper_amd import trigger_stats as ts
    c = th.make_case(n, max(1, n // 20), 5000 if n > 10000 else 0, 5300 + n, 1238166018.75)
    c["series"] = c["series"].astype(dtype)
    thr = 0.1
    duration = n * c["delta_t"]
    ref = th.restate(c, thr)
    series_d = T.from_numpy(c["series"]).cuda()
    inj_d = T.from_numpy(np.sort(c["inj"])).cuda()
    prefactor = (4. / 3.) * np.pi * c["dist"].max() ** 3. / float(len(c["dist"]))
    whole = []

    def case(g):
        series, inj = g.place(series_d), g.place(inj_d)
        t, v, c_trig = ops.trig_triggers(series, c["delta_t"], c["epoch"], thr)
        et, ev, c_ev = ops.trig_events(t, v, th.CLUSTER_TOL, n_dev=c_trig[0:1])
        _, diff = ops.score_closest(inj, et)
        tp, fp, c_sp = ops.trig_split(ev, diff, th.EVENT_TOL, n_dev=c_ev[0:1])
        _, tp_s, _ = ops.score_sort(tp, n_dev=c_sp[0:1])
        _, fp_s, _ = ops.score_sort(fp, n_dev=c_sp[1:2])
        *outs, n_steps = ops.trig_steps(fp_s, c_sp[1:2], tp_s, c_sp[0:1], duration, prefactor, float(len(c["dist"])))
        n_trig, n_ev = int(c_trig[0]), int(c_ev[0])
        n_tp, n_fp, S = int(c_sp[0]), int(c_sp[1]), int(n_steps)
        whole.append(ts.evaluate(g.place(series_d), c["delta_t"], c["epoch"], c["inj"], c["dist"], thr, th.CLUSTER_TOL,
                                 th.EVENT_TOL))
        out = {"c_trig": c_trig, "c_ev": c_ev, "c_sp": c_sp, "n_steps": n_steps, "times": t[:n_trig], "values": v[:n_trig],
               "ev_times": et[:n_ev], "ev_values": ev[:n_ev], "tp": tp[:n_tp]}
        if n_fp:
            out.update({"fp": fp[:n_fp], **{k: o[:S] for k, o in zip(("ranking", "far", "frac", "vol", "err"), outs)}})
        return out
    # err: where a case has more true positives than injections the reference's own variance is negative and its error NaN
    r = run_contract(case, modules=MODULES, may_hold_fill=("err",))
    assert np.array_equal(r["times"].cpu().numpy(), ref["trig_times"]) and np.array_equal(r["values"].cpu().numpy(), ref["trig_values"])
    assert np.array_equal(r["ev_times"].cpu().numpy(), ref["ev_times"]) and np.array_equal(r["ev_values"].cpu().numpy(), ref["ev_values"])
    assert r["c_trig"].tolist() == [len(ref["trig_times"]), 0] and r["c_ev"].tolist() == [len(ref["ev_times"]), 0]
    if "ranking" in r:
        for k, name in (("ranking", "ranking"), ("far", "far"), ("frac", "sens-frac"), ("vol", "sens-vol"), ("err", "sens-vol-err")):
            assert np.array_equal(r[k].cpu().numpy(), ref[name], equal_nan=True), name
    assert len(whole) == len(FILLS) + 1
    for w in whole:
        flat = {"trig_times": w["triggers"][0], "trig_values": w["triggers"][1], "ev_times": w["events"][0],
                "ev_values": w["events"][1], **w["statistics"]}
        th.compare(flat, ref, "guarded evaluate vs restatement")


def test_two_column_head(T, gww):
    """Both modes into rows of a wider buffer: the columns behind C stay untouched."""
    from gw_whisper_amd import ops
    T.manual_seed(5)
    B, d = 37, 128
    dims = (d, 512, 256, 128, 64, 2)
    params = [t for i in range(5) for t in (T.randn(dims[i + 1], dims[i], device="cuda") / dims[i] ** 0.5,
                                            0.1 * T.randn(dims[i + 1], device="cuda"))]
    x = T.randn(B, d, device="cuda")

    def case(g):
        xs, ps = g.place(x), [g.place(p) for p in params]
        soft = ops.det_head_scores2(xs, ps)
        lin = ops.det_head_scores2(xs, ps, remove_softmax=True)
        wide = g.empty((B, 5), T.float32)
        wide.zero_()
        ops.det_head_scores2(xs, ps, out=wide[:, :2])
        return {"soft": soft, "lin": lin, "wide": wide}
    r = run_contract(case, modules=MODULES)
    assert T.equal(r["wide"][:, :2], r["soft"]) and bool((r["wide"][:, 2:] == 0).all())
    assert T.equal(r["lin"][:, 1], -r["lin"][:, 0])
    assert T.equal(r["soft"][:, 0], ops.det_head_scores(x, params, T.empty(B, device="cuda"), ops.SCORE_PROB0))
    assert T.equal(r["lin"][:, 0], ops.det_head_scores(x, params, T.empty(B, device="cuda"), ops.SCORE_LOGIT_DIFF))


def test_undersized_workspaces_are_refused_before_any_launch(T, gww):
    """One byte short: GwwError, and neither the outputs nor the workspace are touched."""
    from gw_whisper_amd import ops
    n = 5000
    c = th.make_case(n, 20, 0, 5400, 0.75)
    L = gww.lib()
    with Guard(FILLS[0], modules=MODULES) as g:
        series = g.place(T.from_numpy(c["series"]).cuda())
        t, v, c_trig = ops.trig_triggers(series, 0.1, 0.75, 0.1)
        one = g.place(T.ones(1, dtype=T.int32, device="cuda"))
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
        refused(lambda ws: ops.trig_triggers(series, 0.1, 0.75, 0.1, ws=ws), L.gww_trig_triggers_workspace_bytes(n))
        refused(lambda ws: ops.trig_events(t, v, 0.2, ws=ws), L.gww_trig_events_workspace_bytes(n))
        refused(lambda ws: ops.trig_split(v, t, 0.3, ws=ws), L.gww_trig_split_workspace_bytes(n))
        refused(lambda ws: ops.trig_steps(v, one, t, one, 10.0, 1.0, 3.0, ws=ws), L.gww_trig_steps_workspace_bytes(n))
        g.check()
