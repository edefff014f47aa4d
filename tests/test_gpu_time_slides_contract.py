"""Memory contract of the entry points of csrc/timeslide.hip (the pattern of tests/test_gpu_search_score_contract.py):
every caller-visible buffer -- the partials, the scores, the event buffers and the counts -- is allocated under
tests/guard.py's guard-band allocator, each case runs under the three fill bytes and unguarded, and must leave every band
intact, write every element its contract says it writes (all of ``scores``, all of ``out_count``, the first ``count``
entries of a slide's event row) and give the same bits whatever lies outside its buffers."""

import numpy as np
import pytest

from tests.guard import run_contract

from . import time_slides_helpers as th

pytestmark = pytest.mark.gpu

MODULES = ("gw_whisper_amd.ops", "gw_whisper_amd.time_slides")


@pytest.fixture(scope="module")
def T():
    import torch
    assert torch.cuda.is_available()
    return torch


@pytest.mark.parametrize("N,D", [(5, 2), (37, 3), (300, 2)])
def test_time_slide_entry_points(T, gww, N, D):
    from gw_whisper_amd import ops
    from gw_whisper_amd import time_slides as ts
    d, C = 128, 2
    tokens, head = th.make_case(N, D, d, C, 900 + N)
    head = head.cuda()
    offs = th.offsets_for(N)
    S = len(offs)
    tok_d, t_d = T.from_numpy(tokens).cuda(), T.from_numpy(th.stamps(N)).cuda()
    params = ts._tail_params(ts.head_layers(head)[0])
    thr = float(np.float32(np.percentile(ts.slide_scores(tok_d, head, offs).cpu().numpy(), 70.0)))

    def case(g):
        partials = ts.head_partials(g.place(tok_d), head)
        scores = ops.slide_scores(partials, [g.place(p) for p in params], offs, ops.SLIDE_LOGIT0)
        probs = ops.slide_scores(partials, [g.place(p) for p in params], offs, ops.SLIDE_PROB0)
        out_t, out_v, cnt = ops.cluster_slides(g.place(t_d), scores, thr, 0.35)
        tight_t, tight_v, tight_cnt = ops.cluster_slides(g.place(t_d), scores, thr, 0.35, cap=1)
        out = {"partials": partials, "scores": scores, "probs": probs, "cnt": cnt, "tight_cnt": tight_cnt}
        for s, c in enumerate(cnt.cpu().numpy()):
            if c:
                out[f"t{s}"], out[f"v{s}"] = out_t[s, :c], out_v[s, :c]
                out[f"tight_t{s}"], out[f"tight_v{s}"] = tight_t[s, :1], tight_v[s, :1]
        return out
    r = run_contract(case, modules=MODULES)
    assert tuple(r["scores"].shape) == (S, N) and tuple(r["probs"].shape) == (S, N) and tuple(r["cnt"].shape) == (S,)
    assert T.equal(r["cnt"], r["tight_cnt"]) and int(r["cnt"].sum()) >= 1
    # ... and what came out under the guard is what the tests of the values check
    sc = r["scores"].cpu().numpy()
    times = th.stamps(N)
    for s in range(S):
        t_ref, v_ref, _ = th.host_clusters(times, sc[s], thr, 0.35)
        assert int(r["cnt"][s]) == len(t_ref)
        if len(t_ref):
            assert np.array_equal(r[f"t{s}"].cpu().numpy(), t_ref) and np.array_equal(r[f"tight_t{s}"].cpu().numpy(), t_ref[:1])
