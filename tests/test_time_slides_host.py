"""Host side of the time slides (gw_whisper_amd/time_slides.py): the slide plan, the fp64 oracle the GPU tests compare
against, and the argument checks of the new entry points, which come before any HIP call.  No GPU."""

import numpy as np
import pytest
import torch

from gw_whisper_amd import GwwError, ops
from gw_whisper_amd import time_slides as ts

from . import time_slides_helpers as th


def test_plan_offsets_and_live_times():
    p = ts.slide_plan(292, 0.1, 2.0, 3, 1.0)
    assert p.k == 20 and p.slides == (1, 2, 3) and p.offsets == (20, 40, 60)
    assert np.array_equal(p.livetime, np.full(3, 292 * 0.1))
    # live time counts the seconds a step really covers when the slicer's step is not the nominal one
    q = ts.slide_plan(292, 0.1, 2.0, 3, 1.0, time_step_size=204 / 2048)
    assert q.offsets == p.offsets and np.array_equal(q.livetime, np.full(3, 292 * (204 / 2048)))
    # 0.1 + 0.2 style ratios are whole numbers within 1e-9
    assert ts.slide_plan(100, 0.1, 0.1 * 3, 1, 0.25).k == 3


def test_plan_keeps_only_the_slides_that_fit():
    """k <= o_s <= N - k: a slide that would wrap back towards zero lag is skipped, not wrapped."""
    p = ts.slide_plan(100, 0.1, 2.0, 6, 1.0)             # k = 20: offsets 20, 40, 60, 80 fit, 100 and 120 do not
    assert p.slides == (1, 2, 3, 4) and p.offsets == (20, 40, 60, 80)
    assert np.array_equal(p.livetime, np.array([10.0, 10.0, 10.0, 10.0, 0.0, 0.0]))
    edge = ts.slide_plan(40, 0.1, 2.0, 3, 1.0)           # N = 2 k: exactly one slide, o = k = N - k
    assert edge.offsets == (20,) and edge.livetime.tolist() == [4.0, 0.0, 0.0]
    short = ts.slide_plan(39, 0.1, 2.0, 3, 1.0)          # N < 2 k: no slide at all
    assert short.slides == () and short.offsets == () and not short.livetime.any()
    # several segments: a slide's live time is the sum over the segments it exists for
    total = sum(ts.slide_plan(n, 0.1, 2.0, 3, 1.0).livetime for n in (100, 50, 39))
    assert np.allclose(total, [15.0, 10.0, 10.0]) and total.sum() == pytest.approx(35.0)


def test_plan_validation():
    with pytest.raises(GwwError, match="whole number"):
        ts.slide_plan(100, 0.1, 2.05, 3, 1.0)
    with pytest.raises(GwwError, match="whole number"):
        ts.slide_plan(100, 0.1, 2.0 + 1e-6, 3, 1.0)
    with pytest.raises(GwwError, match="window length"):
        ts.slide_plan(100, 0.1, 1.0, 3, 1.0)             # equal is not greater
    with pytest.raises(GwwError, match="n_slides"):
        ts.slide_plan(100, 0.1, 2.0, 0, 1.0)


@pytest.mark.parametrize("D,C,softmax", [(2, 2, False), (2, 2, True), (3, 1, False)])
def test_oracle_equals_the_per_pair_loop(D, C, softmax):
    tokens, head = th.make_case(7, D, 128, C, 11)
    w = th.head_weights(head)
    for o in (0, 1, 3, 6):
        a = th.oracle(th.gathered(tokens, o), w, softmax)
        b = th.oracle_pair_loop(tokens, w, o, softmax)
        assert a.shape == (7,) and np.allclose(a, b, rtol=1e-12, atol=1e-14)
    # an offset moves detector 1 only: detector 0's columns of the gathered rows stay where they are
    g = th.gathered(tokens, 3)
    assert np.array_equal(g[:, :128], tokens[:, 0]) and np.array_equal(g[2, 128:256], tokens[5, 1])
    assert np.array_equal(g[5, 128:256], tokens[1, 1])     # (5 + 3) mod 7
    if D == 3:
        assert np.array_equal(g[5, 256:], tokens[(5 + 6) % 7, 2])


def test_helper_offsets_cover_the_wrap():
    assert th.offsets_for(37) == [0, 1, 21, 32, 36]        # wrap at i = 16 (a tile edge) and at i = 5 (inside a tile)
    assert th.offsets_for(5) == [0, 1, 3, 4]
    assert 48 in th.offsets_for(64) and 17 in th.offsets_for(33)


def test_argument_errors_without_gpu():
    """Shape and mode checks come before any HIP call."""
    from gw_whisper_amd import lib
    L = lib()
    a = 1 << 12                                            # non-NULL, 16-byte aligned stand-in: nothing is dereferenced
    p = [a] * 10

    def scores(N=37, D=2, S=3, C=2, mode=0, ptrs=p, out=a):
        return L.gww_slide_scores_f32(*ptrs, N, D, S, C, mode, out, None)
    assert scores(D=1) == -1 and b"D=1" in L.gww_last_error()
    assert scores(D=5) == -1 and b"D=5" in L.gww_last_error()
    assert scores(N=0) == -1 and b"N=" in L.gww_last_error()
    assert scores(S=0) == -1 and b"S=" in L.gww_last_error()
    assert scores(C=0) == -1 and b"C=" in L.gww_last_error()
    assert scores(C=65) == -1 and b"C=" in L.gww_last_error()
    assert scores(mode=2) == -1 and b"mode" in L.gww_last_error()
    assert scores(C=1, mode=1) == -1 and b"softmax" in L.gww_last_error()
    assert scores(out=None) == -1 and b"NULL" in L.gww_last_error()
    assert scores(ptrs=[a + 4] + p[1:]) == -1 and b"aligned" in L.gww_last_error()
    assert scores(ptrs=p[:9] + [None]) == -1 and b"NULL" in L.gww_last_error()

    def cluster(N=37, S=3, cap=4, times=a, cnt=a):
        return L.gww_cluster_slides_f64(times, a, N, S, 0.5, 0.35, a, a, cnt, cap, None)
    assert cluster(N=0) == -1 and b"N=" in L.gww_last_error()
    assert cluster(S=0) == -1 and b"S=" in L.gww_last_error()
    assert cluster(cap=-1) == -1 and b"max_clusters" in L.gww_last_error()
    assert cluster(times=None) == -1 and b"NULL" in L.gww_last_error()
    assert cluster(cnt=None) == -1 and b"NULL" in L.gww_last_error()


def test_python_layer_refuses_what_it_cannot_run():
    tokens, head = th.make_case(7, 2, 128, 2, 3)
    tok = torch.from_numpy(tokens)
    with pytest.raises(GwwError, match="GPU"):
        ts.slide_scores(tok, head, [1])
    with pytest.raises(GwwError, match="GPU"):
        ops.slide_scores(torch.zeros(2, 7, 512), [torch.zeros(1)] * 8, [1])
    with pytest.raises(GwwError, match="GPU"):
        ops.cluster_slides(torch.zeros(7, dtype=torch.float64), torch.zeros(1, 7), 0.5, 0.35)
    with pytest.raises(GwwError, match="D=1"):
        ts.head_partials(torch.from_numpy(tokens[:, :1]), th.make_head(1, 128, 2, 3))
    with pytest.raises(GwwError, match="D \\* d"):
        ts.head_partials(tok, th.make_head(2, 256, 2, 3))
    with pytest.raises(GwwError, match="softmax"):
        ts.slide_scores(tok, th.make_head(2, 128, 1, 3), [1], softmax=True)
    nn = torch.nn
    for bad in (nn.Linear(256, 2), nn.Sequential(nn.Linear(256, 2)),
                nn.Sequential(nn.Linear(256, 512), nn.ReLU(), nn.Linear(512, 256), nn.ReLU(), nn.Linear(256, 128), nn.ReLU(),
                              nn.Linear(128, 32), nn.ReLU(), nn.Linear(32, 2)),
                nn.Sequential(nn.Linear(256, 512), nn.GELU(), nn.Linear(512, 256), nn.ReLU(), nn.Linear(256, 128), nn.ReLU(),
                              nn.Linear(128, 64), nn.ReLU(), nn.Linear(64, 2))):
        with pytest.raises(GwwError, match="five Linear|nn.Sequential"):
            ts.head_layers(bad)
    lin, softmax = ts.head_layers(head)
    assert len(lin) == 5 and softmax
    assert ts.head_layers(th.make_head(2, 128, 2, 3, softmax=False))[1] is False


def test_cluster_capacity_bounds_the_clusters():
    t = th.stamps(300)
    assert ts.cluster_capacity(t, 0.35) == 1 + int((t[-1] - t[0]) / 0.35) < 300
    assert ts.cluster_capacity(t[:1], 0.35) == 1 and ts.cluster_capacity(t, 0.0) == 300
    # the densest case: every fourth window a trigger (0.398 s apart) -- each is a cluster of its own
    sc = np.zeros(300, np.float32)
    sc[::4] = 1.0
    got, _, _ = th.host_clusters(t, sc, 0.5, 0.35)
    assert len(got) == 75 <= ts.cluster_capacity(t, 0.35)


def test_time_slides_refuse_more_than_one_rank(tmp_path, monkeypatch):
    """run_inference.py --time-slides under WORLD_SIZE > 1: a clear message before any GPU work (there is no GPU here)."""
    import importlib.util
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("run_inference", os.path.join(root, "harness", "run_inference.py"))
    ri = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ri)
    argv = ["none", str(tmp_path / "o.npz"), "--synthetic", "30", "--white", "--time-slides", "3"]
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(SystemExit, match="one rank"):
        ri.main(argv + ["--slides-output", str(tmp_path / "s.npz")])
    monkeypatch.setenv("WORLD_SIZE", "1")
    with pytest.raises(SystemExit, match="slides-output"):
        ri.main(argv)
    a = ri.parse_args(["in", "out"])
    assert a.time_slides == 0 and a.slide_shift == 2.0 and a.slides_output is None
