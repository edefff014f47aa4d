"""Time slides on the GPU (gw_whisper_amd/time_slides.py, csrc/timeslide.hip): every slid score against the fp64 oracle of
the head on the gathered rows, determinism and isolation of a slide's row, the clustering of many slides against the host
``get_clusters``, the pipeline end to end and the background duration of ``get_stats``.  Needs an MI355X.

Measured on an MI355X (the per-pair test prints them; the table is in profiles/time_slides.md): e_ref 2.0e-8 .. 5.3e-8, the
slide kernel 1.5e-8 .. 3.5e-8 off the oracle, 0.4 .. 1.35 of e_ref, against a tolerance of 1.0e-7 .. 2.8e-7."""

import importlib.util
import os

import numpy as np
import pytest

from gw_whisper_amd import synth

from . import search_score_helpers as sh
from . import time_slides_helpers as th

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def T():
    import torch
    assert torch.cuda.is_available()
    return torch


def _harness(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "harness", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# ---------------------------------------------------------------------------------------------- 1. per pair
@pytest.mark.parametrize("N,D,d,C", th.SHAPES)
def test_every_slid_score_against_the_fp64_oracle(T, gww, N, D, d, C):
    """Tolerance 4 e_ref + 2^-23 max|score| with e_ref the largest error of the torch fp32 head (the head the zero-lag
    search runs) against the same oracle on the same gathered rows: the split first layer adds one rounding to a
    five-layer chain, and 4x covers the spread of a maximum over a few hundred values."""
    from gw_whisper_amd import time_slides as ts
    tokens, head = th.make_case(N, D, d, C, 100 + N)
    w = th.head_weights(head)
    offs = th.offsets_for(N)
    rows = [th.gathered(tokens, o) for o in offs]
    tok_d = T.from_numpy(tokens).cuda()
    head_d = th.make_head(D, d, C, 100 + N).cuda()
    for softmax in ((False, True) if C >= 2 else (False,)):
        ref = np.stack([th.oracle(r, w, softmax) for r in rows])
        with T.no_grad():
            z = T.stack([head_d[:-1](T.from_numpy(r).cuda()) for r in rows])                 # [S, N, C] logits
            yard = (T.softmax(z, dim=2) if softmax else z)[:, :, 0].cpu().numpy().astype(np.float64)
        got = ts.slide_scores(tok_d, head_d, offs, softmax=softmax).cpu().numpy().astype(np.float64)
        assert got.shape == (len(offs), N)
        e_ref = float(np.abs(yard - ref).max())
        tol = 4.0 * e_ref + 2.0 ** -23 * float(np.abs(ref).max())
        err = np.abs(got - ref).max(axis=1)
        d0 = float(np.abs(got[0] - yard[0]).max())
        print(f"slide scores N={N} D={D} d={d} C={C} softmax={softmax}: e_ref {e_ref:.3e}, tol {tol:.3e}, kernel error per "
              f"offset {dict(zip(offs, [float(f'{e:.3e}') for e in err]))}, offset 0 vs the torch head {d0:.3e}")
        assert e_ref > 0.0
        assert float(err.max()) <= tol, f"slid scores are {err.max():.3e} off the fp64 oracle, tolerance {tol:.3e}"
        # offset 0 is the zero-lag pairing: what model(x)[:, 0]'s head gives
        assert offs[0] == 0 and d0 <= tol, f"offset 0 is {d0:.3e} off the torch head, tolerance {tol:.3e}"
        # a pair off by one window would be orders of magnitude outside the tolerance
        assert float(np.abs(ref[1] - ref[0]).max()) > 100.0 * tol


# ---------------------------------------------------------------------------------------------- 2. determinism, isolation
def test_identical_calls_identical_bits_and_a_row_does_not_depend_on_its_launch(T, gww):
    from gw_whisper_amd import ops
    from gw_whisper_amd import time_slides as ts
    N, D, d, C = 37, 2, 384, 2
    tokens, _ = th.make_case(N, D, d, C, 7)
    tok = T.from_numpy(tokens).cuda()
    head = th.make_head(D, d, C, 7).cuda()
    offs = [21, 1, 32, 36, 5]
    for softmax in (False, True):
        a = ts.slide_scores(tok, head, offs, softmax=softmax)
        b = ts.slide_scores(tok, head, offs, softmax=softmax)
        assert T.equal(a, b)
        for r, o in enumerate(offs):
            assert T.equal(ts.slide_scores(tok, head, [o], softmax=softmax)[0], a[r]), f"offset {o} alone differs"
        # chunking: two launches of 2 + 3 slides are the one launch of 5
        assert T.equal(T.cat([ts.slide_scores(tok, head, offs[:2], softmax=softmax),
                              ts.slide_scores(tok, head, offs[2:], softmax=softmax)]), a)
    # the head with or without its Softmax module is the same head: the mode is the caller's
    assert T.equal(ts.slide_scores(tok, T.nn.Sequential(*list(head.children())[:-1]), offs), ts.slide_scores(tok, head, offs))
    # offsets are checked on the host, before upload
    P = ts.head_partials(tok, head)
    for bad in ([N], [-1], []):
        with pytest.raises(gww.GwwError, match="offset"):
            ops.slide_scores(P, ts._tail_params(ts.head_layers(head)[0]), bad)


# ---------------------------------------------------------------------------------------------- 3. clustering
@pytest.mark.parametrize("S", [1, 5])
@pytest.mark.parametrize("N", [1, 63, 64, 65, 300])
def test_slides_cluster_as_get_clusters_does(T, gww, N, S):
    from gw_whisper_amd import ops
    sc, thr = th.score_rows(S, N, 40 + N + S)
    times = th.stamps(N)
    sc_d, t_d = T.from_numpy(sc).cuda(), T.from_numpy(times).cuda()
    out_t, out_v, cnt = ops.cluster_slides(t_d, sc_d, thr, 0.35)
    out_t, out_v, cnt = out_t.cpu().numpy(), out_v.cpu().numpy(), cnt.cpu().numpy()
    dev_rows = sc_d.cpu().numpy()
    most = 0
    for s in range(S):
        t_ref, v_ref, _ = th.host_clusters(times, dev_rows[s], thr, 0.35)
        assert cnt[s] == len(t_ref), f"slide {s}: {cnt[s]} clusters, get_clusters finds {len(t_ref)}"
        assert np.array_equal(out_t[s, :cnt[s]], t_ref) and np.array_equal(out_v[s, :cnt[s]].astype(np.float64), v_ref)
        most = max(most, int(cnt[s]))
    if S == 5:
        assert cnt[1] == 0 and cnt[2] == 1 and cnt[3] == 1 and cnt[4] == 1
        assert out_t[3, 0] == times[0] and out_t[4, 0] == times[N - 1]
    # fewer slots than clusters: the count tells, the stored prefix is unchanged
    if most >= 2:
        ct, cv, cc = ops.cluster_slides(t_d, sc_d, thr, 0.35, cap=1)
        assert np.array_equal(cc.cpu().numpy(), cnt)
        assert np.array_equal(ct.cpu().numpy()[cnt > 0, 0], out_t[cnt > 0, 0])
        assert np.array_equal(cv.cpu().numpy()[cnt > 0, 0], out_v[cnt > 0, 0])


def test_slide_background_reports_a_cap_overflow(T, gww, monkeypatch):
    """``slide_background`` sizes its event buffers by ``cluster_capacity``; were that ever too small it raises instead of
    returning a cut list."""
    from gw_whisper_amd import inference as inf
    from gw_whisper_amd import time_slides as ts
    N = 300
    rng = np.random.default_rng(5)
    sl = inf.DeviceSegmentSlicer(rng.standard_normal((2, 2048 + 204 * (N - 1))).astype(np.float32), start_time=10.0)
    assert len(sl) == N
    tokens, _ = th.make_case(N, 2, 128, 2, 5)
    head = th.make_head(2, 128, 2, 5, softmax=False).cuda()
    plan = ts.slide_plan(N, 0.1, 2.0, 2, 1.0)
    tok = T.from_numpy(tokens).cuda()
    thr = float(np.percentile(ts.slide_scores(tok, head, plan.offsets).cpu().numpy(), 80.0))
    t, v, var, slide = ts.slide_background(sl, tok, head, plan, thr, 0.35)
    assert len(t) > 4 and set(slide.tolist()) == {1, 2}
    monkeypatch.setattr(ts, "cluster_capacity", lambda times, c: 2)
    with pytest.raises(gww.GwwError, match="more than the 2 slots"):
        ts.slide_background(sl, tok, head, plan, thr, 0.35)


# ---------------------------------------------------------------------------------------------- 4. end to end
@pytest.fixture(scope="module")
def search_case(T):
    """30 s of seeded noise through the d = 128 bf16 model of test_gpu_inference.py, once: the slicer, the model, the
    zero-lag results with and without tokens."""
    from gw_whisper_amd import inference as inf
    from gw_whisper_amd.encoder import WhisperConfig, WhisperEncoder
    rng = np.random.default_rng(30)
    strain = rng.standard_normal((2, 30 * 2048)).astype(np.float32)
    sd = synth.encoder_state_dict(128, 2, 2, 512, seed=3)
    enc = WhisperEncoder.from_numpy_state_dict(sd, WhisperConfig(128, 2, 2, 512), precision="bf16").cuda()
    model = inf.GWWhisperClassifier(enc).cuda().eval()
    sl = inf.DeviceSegmentSlicer(strain, start_time=1.0e9)
    plain = inf.evaluate_slices(sl, model, trigger_threshold=0.5, cluster_threshold=0.35)
    with_tokens = inf.evaluate_slices(sl, model, trigger_threshold=0.5, cluster_threshold=0.35, return_tokens=True)
    return sl, model, plain, with_tokens


def test_return_tokens_changes_nothing_else(T, gww, search_case):
    sl, model, plain, with_tokens = search_case
    N = len(sl)
    assert N == 1 + (30 * 2048 - 2048) // 204 and len(with_tokens) == len(plain) + 1
    tokens = with_tokens[-1]
    assert tokens.is_cuda and tokens.dtype == T.float32 and tuple(tokens.shape) == (N, 2, 128)
    assert plain[0] == with_tokens[0]
    assert all(np.array_equal(a, b) for a, b in zip(plain[1], with_tokens[1]))
    assert all(np.array_equal(a, b) for a, b in zip(plain[2], with_tokens[2]))
    with T.no_grad():                                     # the tokens are the ones the scores were computed from
        first = model.classifier(tokens[:256].reshape(256, 256))[:, 0].cpu().numpy()
    assert np.array_equal(first, with_tokens[1][0])
    with pytest.raises(gww.GwwError, match="embed"):
        from gw_whisper_amd import inference as inf
        inf.evaluate_slices(sl, model.classifier, return_tokens=True)


def test_slide_background_is_the_head_on_shifted_pairs(T, gww, search_case):
    """S = 3, shift 2.0 s: ``slide_background`` == thresholding and clustering, on the host, each slide's device scores;
    and those scores are the model's own classifier on the gathered tokens."""
    from gw_whisper_amd import time_slides as ts
    sl, model, _, with_tokens = search_case
    tokens, N = with_tokens[-1], len(sl)
    plan = ts.slide_plan(N, sl.step_size, 2.0, 3, sl.slice_length * sl.delta_t, sl.time_step_size)
    assert plan.offsets == (20, 40, 60) and np.array_equal(plan.livetime, np.full(3, N * sl.time_step_size))
    times = sl.times_host(0, N)
    per_slide = [ts.slide_scores(tokens, model.classifier, [o], softmax=True)[0].cpu().numpy() for o in plan.offsets]
    thr = float(np.float32(np.percentile(np.stack(per_slide), 70.0)))
    t, v, var, slide = ts.slide_background(sl, tokens, model.classifier, plan, thr, 0.35)
    ref = [th.host_clusters(times, row, thr, 0.35) for row in per_slide]
    assert np.array_equal(t, np.concatenate([r[0] for r in ref])) and np.array_equal(v, np.concatenate([r[1] for r in ref]))
    assert np.array_equal(slide, np.concatenate([np.full(len(r[0]), s, np.int32) for s, r in zip(plan.slides, ref)]))
    assert slide.dtype == np.int32 and (var == 0.2).all() and len(t) >= 3
    # the byte budget only chunks: one slide per launch gives the same events
    t1, v1, _, s1 = ts.slide_background(sl, tokens, model.classifier, plan, thr, 0.35, byte_budget=1)
    assert np.array_equal(t1, t) and np.array_equal(v1, v) and np.array_equal(s1, slide)
    # the scores are the model's own head on the gathered tokens (the torch fp32 head, to its own rounding)
    tok_h = tokens.cpu().numpy()
    with T.no_grad():
        own = model.classifier(T.from_numpy(th.gathered(tok_h, 40)).cuda())[:, 0].cpu().numpy()
    assert np.abs(own - per_slide[1]).max() < 1e-5
    # a segment too short for any slide contributes nothing
    short = ts.slide_plan(N, sl.step_size, 20.0, 3, 1.0, sl.time_step_size)
    assert short.offsets == () and all(len(a) == 0 for a in ts.slide_background(sl, tokens, model.classifier, short, thr, 0.35))


def test_run_inference_with_time_slides(T, gww, tmp_path):
    """harness/run_inference.py --time-slides 3: the zero-lag datasets are bit for bit those of the same command without
    the flag, the slides file carries the plan's live time, and run_search_evaluate.py counts `far` per that live time."""
    from gw_whisper_amd import time_slides as ts
    ri, rse = _harness("run_inference"), _harness("run_search_evaluate")
    probe, base, slid, slides = (str(tmp_path / n) for n in ("probe.npz", "base.npz", "slid.npz", "slides.npz"))
    common = ["none", "--synthetic", "30", "--white"]
    assert ri.main(common[:1] + [probe] + common[1:] + ["--trigger-threshold=-1e30"]) == 0
    thr = float(np.percentile(np.load(probe)["all_vals"], 70.0))
    assert ri.main(common[:1] + [base] + common[1:] + [f"--trigger-threshold={thr!r}"]) == 0
    argv = common[:1] + [slid] + common[1:] + [f"--trigger-threshold={thr!r}", "--time-slides", "3", "--slides-output", slides]
    assert ri.main(argv) == 0
    a, b, s = np.load(base), np.load(slid), np.load(slides)
    assert sorted(a.files) == sorted(b.files) == ["all_vals", "stat", "time", "var"]
    for k in a.files:
        assert a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k]), f"zero-lag dataset {k} changed under --time-slides"
    N = len(a["all_vals"])
    plan = ts.slide_plan(N, 0.1, 2.0, 3, 1.0, 204 / 2048)
    assert np.array_equal(s["slide_livetime"], plan.livetime) and float(s["livetime"]) == plan.livetime.sum()
    assert s["slide"].dtype == np.int32 and len(s["time"]) == len(s["stat"]) == len(s["var"]) == len(s["slide"]) >= 3
    assert set(s["slide"].tolist()) <= {1, 2, 3} and (np.diff(s["slide"]) >= 0).all()
    with pytest.raises(RuntimeError, match="Slides file exists"):
        ri.main(common[:1] + [str(tmp_path / "other.npz")] + argv[2:])
    with pytest.raises(SystemExit, match="slides-output"):
        ri.main(common[:1] + [str(tmp_path / "other.npz")] + common[1:] + ["--time-slides", "3"])

    # run_search_evaluate on a foreground of its own, the slides file as its background
    fg, _, inj, _ = sh.make_case(12, 4, 5, 77)
    t0, t1 = float(np.floor(inj["tc"][0] - 40.0)), float(np.ceil(inj["tc"][-1] + 40.0))
    files = {n: str(tmp_path / f"{n}.npz") for n in ("inj", "fgev", "fgfile", "out_auto", "out_flag", "out_plain", "bg_plain")}
    np.savez(files["inj"], **inj)
    np.savez(files["fgev"], time=fg[0], stat=fg[1], var=fg[2])
    np.savez(files["fgfile"], **{"H1/seg": np.zeros(int(t1 - t0), np.float32), "seg/start_time": t0, "seg/delta_t": 1.0})
    np.savez(files["bg_plain"], time=s["time"], stat=s["stat"], var=s["var"])
    head = ["--injection-file", files["inj"], "--foreground-events", files["fgev"], "--foreground-files", files["fgfile"]]
    assert rse.main(head + ["--background-events", slides, "--output-file", files["out_auto"]]) == 0
    assert rse.main(head + ["--background-events", files["bg_plain"], "--background-duration", repr(float(s["livetime"])),
                            "--output-file", files["out_flag"]]) == 0
    assert rse.main(head + ["--background-events", files["bg_plain"], "--output-file", files["out_plain"]]) == 0
    auto, flag, plain = (dict(np.load(files[k])) for k in ("out_auto", "out_flag", "out_plain"))
    B = len(s["time"])
    assert np.array_equal(auto["far"], np.arange(B - 1, -1, -1) / float(s["livetime"]))
    assert np.array_equal(plain["far"], np.arange(B - 1, -1, -1) / (t1 - t0))
    for k in plain:
        assert np.array_equal(auto[k], flag[k]), k
        if k != "far":
            assert np.array_equal(auto[k], plain[k]), f"{k} depends on the background duration"


# ---------------------------------------------------------------------------------------------- 5. background duration
def test_get_stats_background_duration(T, gww):
    from gw_whisper_amd import search_score
    fg, bg, inj, duration = sh.make_case(40, 90, 9, 4242)
    today = search_score.get_stats(fg, bg, inj, duration=duration, chirp_distance=True)
    x = 31.0 * duration + 0.125
    got = search_score.get_stats(fg, bg, inj, duration=duration, chirp_distance=True, background_duration=x)
    assert set(got) == set(today) == set(search_score.KEYS)
    B = bg.shape[1]
    assert np.array_equal(got["far"], np.arange(B - 1, -1, -1) / x)
    np.testing.assert_allclose(got["far"], today["far"] * duration / x, rtol=4 * 2.0 ** -52, atol=0.0)
    for k in today:
        if k != "far":
            assert np.array_equal(got[k], today[k]), f"{k} depends on the background duration"
    with pytest.raises(gww.GwwError, match="background_duration"):
        search_score.get_stats(fg, bg, inj, duration=duration, background_duration=0.0)
