"""The coincidence kernels (csrc/coinc.hip) and the single-detector search on top of them (gw_whisper_amd/coinc.py) on the
MI355X, against the host oracle ``coinc.coinc_host`` (itself held to a brute-force double loop by
tests/test_coinc_host.py).  Every quantity is an index, a copy or a single fp64 operation: all comparisons are ``==``."""

import dataclasses

import numpy as np
import pytest

from gw_whisper_amd import coinc, synth

from . import coinc_helpers as ch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def T():
    import torch
    assert torch.cuda.is_available()
    return torch


def _np(r):
    return {k: v.cpu().numpy() for k, v in r.items()}


def _run(T, t0, v0, t1, v1, shifts, window, n0=None, n1=None, cap_total=None):
    from gw_whisper_amd import ops
    d = lambda a, dt: T.from_numpy(np.array(a, dtype=dt)).cuda()  # noqa: E731
    return ops.coinc_slides(d(t0, np.float64), d(v0, np.float32), len(t0) if n0 is None else n0, d(t1, np.float64),
                            d(v1, np.float32), len(t1) if n1 is None else n1, d(shifts, np.float64), window, cap_total)


@pytest.mark.parametrize("step", ch.STEPS)
@pytest.mark.parametrize("N,q", ch.CASES)
def test_coinc_slides_equals_the_oracle(T, gww, N, q, step):
    """The three generator cases x two steps x two windows.  (5000, S = 249) has 360 detector-0 events -- two workgroups
    per slide -- and 500 (slide, workgroup) entries, two trips of the offsets scan."""
    c = ch.make_case(N, q, step)
    if N == 5000:
        assert len(c["t0"]) > 256 and 2 * len(c["shifts"]) > 256
    for window in (ch.WINDOW, step):
        ref = coinc.coinc_host(c["t0"], c["v0"], c["t1"], c["v1"], c["shifts"], window)
        assert ref["offsets"][1] >= 1
        got = _np(_run(T, c["t0"], c["v0"], c["t1"], c["v1"], c["shifts"], window))
        ch.check_equal(got, ref)


def test_edge_cases(T, gww):
    e, f = np.zeros((0,)), np.zeros((0,), np.float32)
    one_t, one_v = np.array([1000.6]), np.array([1.5], np.float32)
    shifts = np.array([0.0, 2.0])
    for (t0, v0), (t1, v1) in (((one_t, one_v), (e, f)), ((e, f), (one_t, one_v)), ((e, f), (e, f))):
        got = _np(_run(T, t0, v0, t1, v1, shifts, 0.15))
        assert got["offsets"].tolist() == [0, 0, 0] and all(len(got[k]) == 0 for k in ("time", "stat", "dt", "idx0", "idx1"))
    # one event each: coincident at zero lag (exactly on the boundary), not under the slide -- and the other way round
    for t1, hits in ((np.array([1000.75]), [0, 1, 1]), (np.array([998.5]), [0, 0, 1]), (np.array([1003.0]), [0, 0, 0])):
        window = 0.15 if hits != [0, 1, 1] else float(np.fabs(t1[0] - one_t[0]))
        got = _np(_run(T, one_t, one_v, t1, np.array([2.0], np.float32), shifts, window))
        ref = coinc.coinc_host(one_t, one_v, t1, np.array([2.0], np.float32), shifts, window)
        assert ref["offsets"].tolist() == hits
        ch.check_equal(got, ref)
        if hits == [0, 1, 1]:
            assert abs(got["dt"][0]) == window and got["stat"][0] == 3.5
            cut = _np(_run(T, one_t, one_v, t1, np.array([2.0], np.float32), shifts, float(np.nextafter(window, 0.0))))
            assert cut["offsets"].tolist() == [0, 0, 0]


def test_counts_on_the_device(T, gww):
    """n0, n1 as int32 tensors smaller than the capacity: the entries behind them hold times that would match and values
    that would win, and must be ignored."""
    c = ch.make_case(600, 85.0, 0.1)
    n0, n1 = len(c["t0"]) - 7, len(c["t1"]) - 5
    ref = coinc.coinc_host(c["t0"][:n0], c["v0"][:n0], c["t1"][:n1], c["v1"][:n1], c["shifts"], ch.WINDOW)
    t0, v0, t1, v1 = (np.array(c[k]) for k in ("t0", "v0", "t1", "v1"))
    t0[n0:] = c["t1"][3:10]                              # detector-0 ghosts on top of real detector-1 events
    t1[n1:] = c["t0"][2:7] + 0.01                        # detector-1 ghosts next to real detector-0 events, out of order
    v1[n1:] = 100.0
    dev = lambda n: T.tensor([n], dtype=T.int32).cuda()  # noqa: E731
    got = _np(_run(T, t0, v0, t1, v1, c["shifts"], ch.WINDOW, dev(n0), dev(n1)))
    ch.check_equal(got, ref)
    # a count beyond the capacity is clamped to it, a negative one to zero
    full = coinc.coinc_host(c["t0"], c["v0"], c["t1"], c["v1"], c["shifts"], ch.WINDOW)
    ch.check_equal(_np(_run(T, c["t0"], c["v0"], c["t1"], c["v1"], c["shifts"], ch.WINDOW, dev(10 ** 6), dev(len(c["t1"])))), full)
    none = _np(_run(T, c["t0"], c["v0"], c["t1"], c["v1"], c["shifts"], ch.WINDOW, dev(-1), dev(len(c["t1"])), cap_total=4))
    assert not none["offsets"].any()


@pytest.mark.parametrize("N,q", [(600, 85.0), (5000, 90.0)])
def test_cut_list(T, gww, N, q, monkeypatch):
    """cap_total below the total: offsets unchanged, the written prefix is the oracle's, nothing at or beyond cap_total is
    written -- the buffers come prefilled (torch.empty of ops replaced by a filling one) and two further entries behind
    cap_total are checked through a larger allocation."""
    from gw_whisper_amd import ops
    c = ch.make_case(N, q, 0.1)
    ref = coinc.coinc_host(c["t0"], c["v0"], c["t1"], c["v1"], c["shifts"], ch.WINDOW)
    total = int(ref["offsets"][-1])
    cap = total // 2 + 1
    assert 0 < cap < total
    PAD = 64
    real_empty = T.empty

    class Filling:
        def __getattr__(self, name):
            return getattr(T, name)

        @staticmethod
        def empty(shape, dtype=None, device=None):
            if tuple(shape) != (cap,):
                return real_empty(shape, dtype=dtype, device=device)
            big = real_empty((cap + PAD,), dtype=dtype, device=device)
            big.view(T.uint8).fill_(0x5A)
            Filling.big.append(big)
            return big[:cap]
    Filling.big = []
    monkeypatch.setattr(ops, "torch", Filling())
    got = _run(T, c["t0"], c["v0"], c["t1"], c["v1"], c["shifts"], ch.WINDOW, cap_total=cap)
    monkeypatch.undo()
    assert len(Filling.big) == 5
    for big in Filling.big:
        assert bool((big[cap:].view(T.uint8) == 0x5A).all()), "an entry at or beyond cap_total was written"
    got = _np(got)
    assert np.array_equal(got["offsets"], ref["offsets"])
    for k in ("time", "stat", "dt", "idx0", "idx1"):
        assert got[k].shape == (cap,) and np.array_equal(got[k], ref[k][:cap]), k
    # cap_total above the total: the entries behind the total keep their fill
    Filling.big = []
    cap = total + 3
    monkeypatch.setattr(ops, "torch", Filling())
    got = _run(T, c["t0"], c["v0"], c["t1"], c["v1"], c["shifts"], ch.WINDOW, cap_total=cap)
    monkeypatch.undo()
    for big in Filling.big:
        assert bool((big[total:].view(T.uint8) == 0x5A).all())
    assert np.array_equal(got["idx1"][:total].cpu().numpy(), ref["idx1"])


def test_rule_breaking_lists(T, gww):
    t0, v0, t1, v1 = ch.rule_breaking()
    shifts = np.array([0.0, 0.125, 0.3, 1.0])
    twice = False
    for window in (0.0625, 0.15, 0.1875, 0.5):
        ref = coinc.coinc_host(t0, v0, t1, v1, shifts, window)
        got = _np(_run(T, t0, v0, t1, v1, shifts, window))
        ch.check_equal(got, ref)
        j = got["idx1"][:got["offsets"][1]]
        twice |= len(np.unique(j)) < len(j)
    assert twice                                         # a detector-1 event is not consumed by being chosen


def test_argument_errors(T, gww):
    from gw_whisper_amd import GwwError, ops
    t, v = T.zeros(4, dtype=T.float64).cuda(), T.zeros(4).cuda()
    sh = T.zeros(1, dtype=T.float64).cuda()
    with pytest.raises(GwwError, match="n0"):
        ops.coinc_slides(t, v, 5, t, v, 4, sh, 0.15)
    with pytest.raises(GwwError, match="window"):
        ops.coinc_slides(t, v, 4, t, v, 4, sh, -1.0)
    with pytest.raises(GwwError, match="shifts"):
        ops.coinc_slides(t, v, 4, t, v, 4, sh[:0], 0.15)
    with pytest.raises(GwwError, match="GPU"):
        ops.coinc_slides(t.cpu(), v, 4, t, v, 4, sh, 0.15)
    with pytest.raises(GwwError, match="v1"):
        ops.coinc_slides(t, v, 4, t, v.double(), 4, sh, 0.15)
    lib = gww.lib()
    assert lib.gww_coinc_count_f64(t.data_ptr(), None, 4, t.data_ptr(), v.data_ptr(), None, 4, sh.data_ptr(), 0, 0.15, None, None,
                                   None) == -1
    assert b"slides" in lib.gww_last_error()
    assert lib.gww_coinc_count_f64(t.data_ptr(), None, (1 << 27) + 1, t.data_ptr(), v.data_ptr(), None, 4, sh.data_ptr(), 1, 0.15,
                                   None, None, None) == -1
    assert b"2^27" in lib.gww_last_error()
    assert lib.gww_coinc_offsets(None, 4, 1, None, None) == -1 and b"NULL" in lib.gww_last_error()
    assert lib.gww_coinc_emit_f64(t.data_ptr(), v.data_ptr(), None, 4, t.data_ptr(), v.data_ptr(), None, 4, sh.data_ptr(), 70000,
                                  None, None, 0, None, None, None, None, None, None) == -1


# ---------------------------------------------------------------------------------------------- detector_scores
def _encoder(T, seed, context=None):
    from gw_whisper_amd.encoder import WhisperConfig, WhisperEncoder
    d, L, H, F = synth.ENCODER_SIZES["micro"]
    sd = synth.encoder_state_dict(d, L, H, F, seed=seed)
    cfg = WhisperConfig.named("micro")
    if context is not None:
        sd["embed_positions.weight"] = sd["embed_positions.weight"][:context].copy()
        cfg = dataclasses.replace(cfg, max_source_positions=context)
    return WhisperEncoder.from_numpy_state_dict(sd, cfg, precision="bf16").cuda()


def _model(T, seed, context=None):
    """A seeded single-detector model on the micro encoder; the first layer of its head scaled so that the logit moves with
    the strain (tests/test_gpu_real_events.py)."""
    from gw_whisper_amd import models
    T.manual_seed(seed)
    m = models.one_channel_ligo_binary_classifier(_encoder(T, seed, context), num_classes=1).cuda().eval()
    with T.no_grad():
        m.classifier[0].weight.mul_(200.0)
    return m


def _segment(n_windows, seed, L=2048, step=204):
    return np.random.default_rng(seed).standard_normal((2, L + (n_windows - 1) * step + 5)).astype(np.float32)


def _direct(T, models, windows, features):
    """The models applied to cut windows [b, 2, L]: the feature path on the cut windows, the detectors stacked in one batch
    for one shared model, one pass per model otherwise -- the same batch boundaries ``detector_scores`` has."""
    from gw_whisper_amd import binary
    b = windows.shape[0]
    mel = features(windows.permute(1, 0, 2).reshape(2 * b, -1).contiguous())
    with T.no_grad():
        if len(models) == 1:
            return binary.head_logits(models[0].classifier, models[0].pooled(mel))[:, 0].reshape(2, b)
        return T.stack([binary.head_logits(m.classifier, m.pooled(mel[g * b:(g + 1) * b]))[:, 0] for g, m in enumerate(models)])


@pytest.mark.parametrize("shared", [True, False])
def test_detector_scores_resampled(T, gww, shared):
    """micro encoder, two detectors, N = 37 windows in batches of 16 (16 + 16 + 5): row g, window i is the model applied
    to the cut window, bit for bit; the head's one HIP launch agrees with the module's own forward to fp32 rounding."""
    from gw_whisper_amd import ops
    from gw_whisper_amd.inference import DeviceSegmentSlicer, resample
    slicer = DeviceSegmentSlicer(_segment(37, 3))
    assert len(slicer) == 37 and slicer.index_step_size == 204
    ms = [_model(T, 5)] if shared else [_model(T, 5), _model(T, 6)]
    got = coinc.detector_scores(slicer, ms[0] if shared else ms, batch_size=16)
    assert got.shape == (2, 37) and got.dtype == T.float32
    feats = lambda rows: ops.logmel(resample(rows, 16000))  # noqa: E731
    ref = T.cat([_direct(T, ms, slicer.windows(i, min(i + 16, 37)), feats) for i in range(0, 37, 16)], dim=1)
    assert T.equal(got, ref)
    assert float(got.std()) > 1e-3                          # the logits move with the strain
    if not shared:
        assert not T.equal(got[1], coinc.detector_scores(slicer, ms[0], batch_size=16)[1])
    # the module's forward (torch's Linear layers) on detector 0's first batch: the same logits up to fp32 summation order;
    # five layers of at most 512 terms, |logit| of order 1..10: 1e-3 absolute is hundreds of roundings away from either
    with T.no_grad():
        mel = feats(slicer.windows(0, 16)[:, 0].contiguous())
        fwd = ms[0](mel)[:, 0].float()
    assert float((fwd - got[0, :16]).abs().max()) <= 1e-3 * max(1.0, float(fwd.abs().max()))


@pytest.mark.parametrize("shared", [True, False])
def test_detector_scores_native_front_end(T, gww, shared):
    """The same with a native ``FrontendConfig`` (2048 samples, n_fft 128, hop 16; a 64-position encoder): the features come
    from ``ops.logmel_windows`` on the series and equal ``ops.logmel`` on the cut windows bit for bit."""
    from gw_whisper_amd import ops
    from gw_whisper_amd.inference import DeviceSegmentSlicer
    fe = ops.FrontendConfig(80, 2048, 128, 16, 2048, 0.0, 1024.0)
    slicer = DeviceSegmentSlicer(_segment(37, 4))
    ms = [_model(T, 7, 64)] if shared else [_model(T, 7, 64), _model(T, 8, 64)]
    got = coinc.detector_scores(slicer, ms[0] if shared else ms, batch_size=16, frontend=fe)
    feats = lambda rows: ops.logmel(rows, config=fe)  # noqa: E731
    ref = T.cat([_direct(T, ms, slicer.windows(i, min(i + 16, 37)), feats) for i in range(0, 37, 16)], dim=1)
    assert T.equal(got, ref) and float(got.std()) > 1e-3
    with pytest.raises(coinc.GwwError, match="n_samples"):
        coinc.detector_scores(slicer, ms[0], frontend=ops.FrontendConfig(80, 2048, 128, 16, 1024, 0.0, 1024.0))
    with pytest.raises(coinc.GwwError, match="models"):
        coinc.detector_scores(slicer, [ms[0]] * 3)


# ---------------------------------------------------------------------------------------------- end to end
PLANTED = (12.0, 31.5, 47.3)           # seconds into the segment at which a burst starts
BURST = 64                             # samples (31 ms)
FRAMES = (71, 84)                      # the log-mel frames around 0.6 s into a window: frame f is centred on sample 16 f


def _strain():
    """~60 s of white noise in two detectors, three loud common bursts (150 Hz, 31 ms) up to 4 ms apart."""
    x = np.random.default_rng(11).standard_normal((2, 60 * 2048)).astype(np.float32)
    burst = (40.0 * np.sin(2 * np.pi * 150.0 * np.arange(BURST) / 2048.0) * np.hanning(BURST)).astype(np.float32)
    for k, sec in enumerate(PLANTED):
        i = int(sec * 2048)
        x[0, i:i + BURST] += burst
        x[1, i + 8 * (k - 1):i + 8 * (k - 1) + BURST] += burst
    return x


class _EnergyEncoder:
    """Stands where the encoder stands in ``one_channel_ligo_binary_classifier`` and localises by construction: the token is
    the mean log-mel energy per mel bin over the frames around 0.6 s into the window (80 values, zero-padded to 128).  With
    the head below the logit of a window is its mean log-mel energy there: largest for the window that holds a burst where
    a trained model expects the merger, so that the window's stamp is the burst's time to within half a step."""

    class config:
        d_model = 128

    def last_token(self, mel):
        e = mel[:, :, FRAMES[0]:FRAMES[1]].mean(dim=2)
        import torch
        return torch.cat((e, e.new_zeros((e.shape[0], 128 - e.shape[1]))), dim=1).contiguous()


def _energy_model(T):
    from gw_whisper_amd import models
    m = models.one_channel_ligo_binary_classifier(_EnergyEncoder(), num_classes=1)
    with T.no_grad():
        for p in m.classifier.parameters():
            p.zero_()
        m.classifier[0].weight[0, :80] = 1.0 / 80.0          # unit 0: the mean over the mel bins ...
        for i in (2, 4, 6, 8):
            m.classifier[i].weight[0, 0] = 1.0               # ... handed on through the ReLUs (it is positive) to the logit
    return m.cuda().eval()


def _search_and_check(slicer, model, fe, S=12):
    """``search_segment`` against ``coinc_host`` on the scores read back from the device and on the host's clusters; the
    threshold at the 90th percentile of the scores, so that the slides are not empty either."""
    N, window, cthr = len(slicer), ch.WINDOW, ch.CLUSTER_THRESHOLD
    scores = coinc.detector_scores(slicer, model, batch_size=128, frontend=fe)
    sc = scores.cpu().numpy()
    thr = float(np.float32(np.percentile(sc, 90.0)))
    times = slicer.times_host(0, N)
    plan = coinc.slide_shifts(N, 0.1, 2.0, S, slicer.slice_length * slicer.delta_t, slicer.time_step_size, window=window)
    assert plan.slides == tuple(range(1, S + 1))
    fg, bg = coinc.search_segment(slicer, model, thr, cthr, window, plan, batch_size=128, frontend=fe)
    (t0, v0), (t1, v1) = (ch.clusters(times, sc[g], thr, cthr) for g in range(2))
    assert len(t0) >= 3 and len(t1) >= 3
    ref = coinc.coinc_host(t0, v0, t1, v1, [0.0] + list(plan.shifts), window)
    o = ref["offsets"]
    print(f"events {len(t0)} / {len(t1)}, zero-lag coincidences {o[1]}, slid {o[-1] - o[1]} in {S} slides")
    assert np.array_equal(fg[0], ref["time"][:o[1]]) and np.array_equal(fg[1], ref["stat"][:o[1]])
    assert np.array_equal(fg[2], np.full((o[1],), 0.2))
    assert np.array_equal(bg[0], ref["time"][o[1]:]) and np.array_equal(bg[1], ref["stat"][o[1]:])
    assert np.array_equal(bg[2], np.full((o[-1] - o[1],), 0.2))
    assert bg[3].dtype == np.int32 and np.array_equal(bg[3], np.repeat(np.arange(1, S + 1), np.diff(o)[1:]))
    # the scores given instead of a second pass, and the slides in chunks of three: the same arrays
    fg2, bg2 = coinc.search_segment(slicer, None, thr, cthr, window, plan, scores=scores,
                                    byte_budget=3 * (4 * len(t0) + 8 + 32 * min(len(t0), len(t1))))
    assert all(np.array_equal(a, b) for a, b in zip(fg + bg, fg2 + bg2))
    fg3, bg3 = coinc.search_segment(slicer, None, thr, cthr, window, None, scores=scores)
    assert all(np.array_equal(a, b) for a, b in zip(fg, fg3)) and all(len(b) == 0 for b in bg3) and bg3[3].dtype == np.int32
    # live time: the overlap of the segment with its shifted copy, summed over the slides
    step = slicer.time_step_size
    assert plan.livetime.sum() == sum(N * step - s_ * 20 * step for s_ in range(1, S + 1))
    return dict(slicer=slicer, scores=scores, thr=thr, times=times, fg=fg, bg=bg)


@pytest.fixture(scope="module")
def searched(T):
    """The search with a seeded 64-position micro model on the native front end (a short encoder keeps the pass over 593
    windows x 2 detectors well under a second)."""
    from gw_whisper_amd import ops
    from gw_whisper_amd.inference import DeviceSegmentSlicer
    fe = ops.FrontendConfig(80, 2048, 128, 16, 2048, 0.0, 1024.0)
    return _search_and_check(DeviceSegmentSlicer(_strain(), start_time=1000.0), _model(T, 9, 64), fe)


def test_search_segment_end_to_end(T, gww, searched):
    assert len(searched["slicer"]) == 593


def test_search_segment_finds_the_planted_transients(T, gww):
    """The same search with a model that localises by construction (``_EnergyEncoder``): every planted burst comes out as a
    foreground coincidence within one step of its time.  A burst that starts p seconds in is centred at p + 0.016 s.  The
    12 frames that overlap it fit the 13 of ``FRAMES`` when it is centred 0.598 .. 0.605 s into the window; the windows start
    every 204 samples, so the best window holds it there up to half a step and its stamp, start + 0.6 s, is the burst's time
    to 0.055 s -- inside one step, 204 / 2048 s."""
    from gw_whisper_amd import ops
    from gw_whisper_amd.inference import DeviceSegmentSlicer
    fe = ops.FrontendConfig(80, 2048, 128, 16, 2048, 0.0, 1024.0)
    slicer = DeviceSegmentSlicer(_strain(), start_time=1000.0)
    r = _search_and_check(slicer, _energy_model(T), fe)
    planted = 1000.0 + np.array(PLANTED) + 0.5 * BURST / 2048.0
    away = np.abs(r["fg"][0][None, :] - planted[:, None]).min(axis=1)
    print("foreground times", r["fg"][0].tolist(), "nearest to the planted times by", away.tolist())
    assert (away <= slicer.time_step_size).all()
    assert len(r["bg"][0]) >= 1


def test_search_segment_one_detector_and_refusals(T, gww, searched):
    from gw_whisper_amd.inference import DeviceSegmentSlicer
    s = searched
    one = DeviceSegmentSlicer(s["slicer"].dss[1:2], start_time=1000.0)
    fg, bg = coinc.search_segment(one, None, s["thr"], ch.CLUSTER_THRESHOLD, ch.WINDOW, None, scores=s["scores"][1:2].contiguous())
    t1, v1 = ch.clusters(s["times"], s["scores"][1].cpu().numpy(), s["thr"], ch.CLUSTER_THRESHOLD)
    assert np.array_equal(fg[0], t1) and np.array_equal(fg[1], v1.astype(np.float64)) and np.array_equal(fg[2], np.full(t1.shape, 0.2))
    assert all(len(b) == 0 for b in bg)
    plan = coinc.slide_shifts(len(one), 0.1, 2.0, 3, 1.0, one.time_step_size, window=ch.WINDOW)
    with pytest.raises(coinc.GwwError, match="one detector"):
        coinc.search_segment(one, None, s["thr"], ch.CLUSTER_THRESHOLD, ch.WINDOW, plan, scores=s["scores"][1:2].contiguous())
    with pytest.raises(coinc.GwwError, match="cluster_threshold"):
        coinc.search_segment(s["slicer"], None, s["thr"], 0.35, 0.175, None, scores=s["scores"])
