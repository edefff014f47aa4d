"""The glitch scan on the GPU (csrc/glitch_scan.hip, gw_whisper_amd/glitch_scan.py): ``ops.head_scan`` against
``ops.head_forward(train=False)``, ``ops.glitch_events`` against ``build_events_host`` bit for bit, the memory contract of
both, and ``GlitchScanner.scan`` against the same windows cut out and passed through the pieces one by one.

The bound on the probabilities.  The reference is the fp64 softmax of the fp32 logits ``head_forward`` returns, which are
the bits ``head_scan`` computes its probabilities from (asserted through ``cls`` and, in the scan test, by construction).
With u = 2^-24, d_j = z_j - z_max <= 0 and p_k the true probabilities, the tail of ``k_head_scan`` does, per row:

    d_j   = fl(z_j - z_max)             one rounding: d_j (1 + a), |a| <= u; through the exponential a relative |d_j| u
    e_j   = expf(d_j)                   HIP's expf: 1 ulp, at most 2 u relative         -> e_j carries (|d_j| + 2) u
                                        (csrc/glitch_scan.hip is built without fma contraction, csrc/Makefile: a
                                        contracted expf counts a rounding remainder twice, |d_j| u more)
    se    = sum of <= 64 e_k            all positive: the e_k's errors enter weighted by p_k, sum_k p_k (|d_k| + 2) u, and
                                        the 6 levels of the shuffle tree add 6 u
    p_j   = e_j / se                    one rounding, u

so  |p_j - p_j(fp64)| <= p_j u (|d_j| + sum_k p_k |d_k| + 11) to first order; the second-order terms are below 1e-12
relative and an exponential below the normal range adds at most 2^-125 absolutely.  ``prob`` is the j = argmax element:
d = 0, e = 1 exactly, the same sum and one division.  sum_k p_k |d_k| is at most ln 64 = 4.2 (it is the entropy minus
ln sum e), so the predicted class's bound is below 15.2 u = 9.1e-7 for every input, and an element's stays below 1e-5
as long as the exponential is normal (|d_j| <= 87): both are asserted on the bound itself before it is used.
"""

import numpy as np
import pytest

from gw_whisper_amd import synth
from tests import glitch_scan_cases as gc
from tests import guard

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
MODULES = guard.PACKAGE_MODULES + ("gw_whisper_amd.glitch_scan",)
PARAM_KEYS = ("0.weight", "0.bias", "3.weight", "3.bias", "6.weight", "6.bias", "9.weight", "9.bias")


@pytest.fixture(scope="module")
def T():
    import torch
    assert torch.cuda.is_available()
    return torch


def head_params(T, d_in, C, seed, gain=8.0):
    """Seeded head tensors on the GPU; the last layer is scaled so that the logits of a row spread over several units."""
    sd = synth.head_state_dict([d_in, 512, 256, 128, C], seed=seed, sequential_stride=3)
    ps = [T.from_numpy(sd[k]).cuda() for k in PARAM_KEYS]
    ps[6] = ps[6] * gain
    return ps


def softmax64(logits):
    z = logits.astype(np.float64)
    d = z - z.max(axis=1, keepdims=True)
    e = np.exp(d)
    return e / e.sum(axis=1, keepdims=True), d


def prob_bounds(logits):
    """(bound per element [B, C], bound of the predicted class [B]) from the header's derivation."""
    p, d = softmax64(logits)
    spread = (p * np.abs(d)).sum(axis=1, keepdims=True)
    assert float(spread.max()) <= np.log(64.0) + 1e-9
    rel = U * (np.abs(d) + spread + 11.0) + 1e-12
    assert float(rel[np.abs(d) <= 87.0].max()) < 1e-5 and float((U * (spread + 11.0)).max()) < 2e-6
    return p * rel + 2.0 ** -125, p.max(axis=1) * (U * (spread[:, 0] + 11.0) + 1e-12)


def check_against_head_forward(T, x, ps, cls, prob, probs):
    from gw_whisper_amd import ops
    B = x.shape[0]
    _, logits, _, pred, _ = ops.head_forward(x, ps, T.zeros(B, dtype=T.int64, device="cuda"), train=False)
    logits = logits.cpu().numpy()
    assert np.array_equal(cls.cpu().numpy(), pred.cpu().numpy().astype(np.int32))
    p64, _ = softmax64(logits)
    b_all, b_top = prob_bounds(logits)
    top = p64[np.arange(B), cls.cpu().numpy()]
    err_top = np.abs(prob.cpu().numpy().astype(np.float64) - top)
    print(f"B={B} C={logits.shape[1]}: max |prob - fp64| / bound = {float((err_top / b_top).max()):.3f}, "
          f"relative {float((err_top / top).max()):.2e}")
    assert np.all(err_top <= b_top)
    if probs is not None:
        got = probs.cpu().numpy()
        err = np.abs(got.astype(np.float64) - p64)
        print(f"    max |probs - fp64| / bound = {float((err / b_all).max()):.3f}")
        assert np.all(err <= b_all)
        assert np.array_equal(prob.cpu().numpy(), got[np.arange(B), cls.cpu().numpy()])      # prob IS probs[cls]
    return logits


# ---------------------------------------------------------------------------------------------- ops.head_scan
@pytest.mark.parametrize("d_in", [384, 512])
@pytest.mark.parametrize("C", [1, 2, 22, 64])
@pytest.mark.parametrize("B", [1, 16, 17, 33])
def test_head_scan_is_the_eval_head(T, gww, B, C, d_in):
    from gw_whisper_amd import ops
    ps = head_params(T, d_in, C, seed=100 + C)
    x = T.from_numpy(np.random.default_rng(B * 1000 + C + d_in).standard_normal((B, d_in)).astype(np.float32)).cuda()
    cls, prob, probs = ops.head_scan(x, ps, want_probs=True)
    assert cls.dtype == T.int32 and tuple(cls.shape) == (B,) and tuple(prob.shape) == (B,) and tuple(probs.shape) == (B, C)
    check_against_head_forward(T, x, ps, cls, prob, probs)
    # without probs: the same class and probability
    cls2, prob2, none = ops.head_scan(x, ps)
    assert none is None and T.equal(cls, cls2) and T.equal(prob, prob2)


def test_head_scan_tie_takes_the_lower_index(T, gww):
    """Two identical last-layer rows and biases give two identical logits; lifted above the rest they tie for the maximum."""
    from gw_whisper_amd import ops
    C, d_in, B = 22, 384, 17
    ps = head_params(T, d_in, C, seed=7)
    ps[6][13] = ps[6][5]
    ps[7][5] = ps[7][13] = 50.0
    x = T.from_numpy(np.random.default_rng(3).standard_normal((B, d_in)).astype(np.float32)).cuda()
    cls, prob, probs = ops.head_scan(x, ps, want_probs=True)
    logits = check_against_head_forward(T, x, ps, cls, prob, probs)
    assert np.array_equal(logits[:, 5], logits[:, 13]) and np.all(logits.argmax(axis=1) == 5)
    assert np.all(cls.cpu().numpy() == 5) and np.array_equal(probs[:, 5].cpu().numpy(), probs[:, 13].cpu().numpy())
    assert float(prob.max()) <= 0.5


def test_head_scan_row_offset_and_repeat(T, gww):
    """A batch written at a row offset touches its rows only, and gives there what it gives alone; two calls, same bits."""
    from gw_whisper_amd import GwwError, ops
    C, d_in, B, N, off = 22, 512, 17, 40, 9
    ps = head_params(T, d_in, C, seed=11)
    x = T.from_numpy(np.random.default_rng(5).standard_normal((B, d_in)).astype(np.float32)).cuda()
    alone = ops.head_scan(x, ps, want_probs=True)
    cls = T.full((N,), -7, dtype=T.int32, device="cuda")
    prob = T.full((N,), -1.0, dtype=T.float32, device="cuda")
    probs = T.full((N, C), -2.0, dtype=T.float32, device="cuda")
    out = ops.head_scan(x, ps, cls, prob, probs, row_offset=off)
    assert out[0] is cls and out[1] is prob and out[2] is probs
    for got, want, fill in zip((cls, prob, probs), alone, (-7, -1.0, -2.0)):
        assert T.equal(got[off:off + B], want)
        assert bool((got[:off] == fill).all()) and bool((got[off + B:] == fill).all())
    again = ops.head_scan(x, ps, want_probs=True)
    assert all(T.equal(a, b) for a, b in zip(alone, again))
    # the first batch of a scan allocates series-long arrays
    c3, p3, _ = ops.head_scan(x, ps, n_rows=N)
    assert tuple(c3.shape) == (N,) and T.equal(c3[:B], alone[0]) and T.equal(p3[:B], alone[1])
    with pytest.raises(GwwError, match="do not fit"):
        ops.head_scan(x, ps, cls, prob, row_offset=N - B + 1)
    with pytest.raises(GwwError, match="B=1025"):
        ops.head_scan(T.zeros(1025, d_in, device="cuda"), ps)


# ---------------------------------------------------------------------------------------------- ops.glitch_events
def device_events(T, times, cls, prob, cap=None, **kw):
    """``ops.glitch_events`` -> (the first min(count, cap) entries as numpy arrays, count, the raw device dict)."""
    from gw_whisper_amd import ops
    from gw_whisper_amd.glitch_scan import EVENT_KEYS, ignore_mask
    kw = dict(kw)
    if "ignore" in kw:
        kw["ignore"] = ignore_mask(kw["ignore"])
    ev = ops.glitch_events(T.from_numpy(times).cuda(), T.from_numpy(cls).cuda(), T.from_numpy(prob).cuda(), cap=cap, **kw)
    k = int(ev["count"].item())
    kept = k if cap is None else min(k, cap)
    return {key: ev[key][:kept].cpu().numpy() for key in EVENT_KEYS}, k, ev


@pytest.mark.parametrize("case", gc.HAND_CASES, ids=[c["name"] for c in gc.HAND_CASES])
def test_glitch_events_hand_written(T, gww, case):
    from gw_whisper_amd.glitch_scan import build_events_host
    got, k, _ = device_events(T, case["times"], case["cls"], case["prob"], **case["kw"])
    assert k == len(case["expect"])
    gc.same_bits(got, gc.expected_events(case))
    gc.same_bits(got, build_events_host(case["times"], case["cls"], case["prob"], **case["kw"]))


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257])
def test_glitch_events_small_sizes(T, gww, n):
    from gw_whisper_amd.glitch_scan import build_events_host
    times, cls, prob = gc.random_case(n, 5, seed=40 + n)
    for thr in (0.3, 0.0):
        want = build_events_host(times, cls, prob, prob_threshold=thr)
        got, k, _ = device_events(T, times, cls, prob, prob_threshold=thr)
        assert k == len(want["cls"])
        gc.same_bits(got, want)


def test_glitch_events_random_merges_and_splits(T, gww):
    """n = 5000, 22 classes: a common class whose events run on for many windows and rare ones whose events are single
    windows -- both a trigger that joins and one that splits occur, in the same series."""
    from gw_whisper_amd.glitch_scan import build_events_host
    times, cls, prob = gc.random_case(5000, 22, seed=77, p_class0=0.5)
    for kw in (dict(prob_threshold=0.5), dict(prob_threshold=0.2, gap=0.25, ignore=[3, 21]), dict(prob_threshold=0.9, gap=1.0)):
        want = build_events_host(times, cls, prob, **kw)
        got, k, ev = device_events(T, times, cls, prob, **kw)
        triggers = int(want["n"].sum())
        assert bool((want["n"] > 1).any()), "no trigger joined an event"
        assert len(want["cls"]) > 22 and triggers > len(want["cls"]), "no event was split off / nothing merged"
        assert k == len(want["cls"])
        gc.same_bits(got, want)
        again, k2, _ = device_events(T, times, cls, prob, **kw)                 # identical calls, identical bits
        assert k2 == k
        gc.same_bits(again, got)


def test_glitch_events_spanning_event(T, gww):
    """n = 70 000: one event of class 0 over the whole series (23 334 windows, its peak in the middle) under many short
    ones -- across every 64-window step, every 4096-window trip of the compaction and the 16-bit boundary."""
    from gw_whisper_amd.glitch_scan import build_events_host
    n = 70000
    times, cls, prob = gc.spanning_case(n, 22, seed=5)
    want = build_events_host(times, cls, prob)
    assert want["cls"][0] == 0 and want["first"][0] == 0 and want["n"][0] == (n + 2) // 3
    assert want["t_end"][0] == times[(n - 1) // 3 * 3] and want["t_peak"][0] == times[(n // 2) // 3 * 3]
    assert int((want["cls"] == 0).sum()) == 1 and len(want["cls"]) > 5000 and int(want["first"].max()) > 65536
    got, k, _ = device_events(T, times, cls, prob)
    assert k == len(want["cls"])
    gc.same_bits(got, want)


def test_glitch_events_cap_below_the_count(T, gww):
    from gw_whisper_amd.glitch_scan import EVENT_KEYS, build_events_host
    times, cls, prob = gc.random_case(5000, 22, seed=78)
    want = build_events_host(times, cls, prob)
    total = len(want["cls"])
    assert total > 100
    for cap in (0, 1, 100):
        got, k, ev = device_events(T, times, cls, prob, cap=cap)
        assert k == total and all(tuple(ev[key].shape) == (cap,) for key in EVENT_KEYS)
        gc.same_bits(got, {key: v[:cap] for key, v in want.items()})


# ---------------------------------------------------------------------------------------------- memory contract
@pytest.mark.parametrize("B,C,d_in", [(1, 1, 384), (17, 22, 384), (33, 64, 512)])
def test_head_scan_contract(T, gww, B, C, d_in):
    from gw_whisper_amd import ops
    ps = head_params(T, d_in, C, seed=21)
    x = T.from_numpy(np.random.default_rng(B).standard_normal((B, d_in)).astype(np.float32)).cuda()

    def case(g):
        cls, prob, probs = ops.head_scan(g.place(x), [g.place(p) for p in ps], want_probs=True)
        # a second batch behind the first in series-long arrays: rows in front of the offset are the first call's
        c2, p2, _ = ops.head_scan(g.place(x), [g.place(p) for p in ps], n_rows=2 * B)
        ops.head_scan(g.place(x), [g.place(p) for p in ps], c2, p2, row_offset=B)
        return {"cls": cls, "prob": prob, "probs": probs, "cls2": c2, "prob2": p2}
    r = guard.run_contract(case, modules=MODULES)
    assert T.equal(r["cls2"][:B], r["cls"]) and T.equal(r["cls2"][B:], r["cls"])
    assert T.equal(r["prob2"][:B], r["prob"]) and T.equal(r["prob2"][B:], r["prob"])
    check_against_head_forward(T, x, ps, r["cls"], r["prob"], r["probs"])


@pytest.mark.parametrize("n,cap", [(1, None), (65, None), (5000, None), (5000, 7)])
def test_glitch_events_contract(T, gww, n, cap):
    """No write outside any output (a cap below the count included), every element of [0, min(count, cap)) written, the
    same bits whatever the workspace and the memory around the buffers hold."""
    from gw_whisper_amd import ops
    from gw_whisper_amd.glitch_scan import EVENT_KEYS, build_events_host
    times, cls, prob = gc.random_case(n, 22, seed=90 + n)
    prob[0] = np.float32(0.9)
    cls[0] = 2                                                                    # at least one event
    want = build_events_host(times, cls, prob)
    kept = len(want["cls"]) if cap is None else min(len(want["cls"]), cap)
    t_d, c_d, p_d = T.from_numpy(times).cuda(), T.from_numpy(cls).cuda(), T.from_numpy(prob).cuda()

    def case(g):
        ev = ops.glitch_events(g.place(t_d), g.place(c_d), g.place(p_d), cap=cap)
        out = {"count": ev["count"]}
        out.update({key: ev[key][:kept] for key in EVENT_KEYS})
        return out
    r = guard.run_contract(case, modules=MODULES)
    assert int(r["count"]) == len(want["cls"])
    gc.same_bits({key: r[key].cpu().numpy() for key in EVENT_KEYS}, {key: v[:kept] for key, v in want.items()})


# ---------------------------------------------------------------------------------------------- the scan
@pytest.fixture(scope="module")
def tiny(T):
    """A seeded whisper-tiny DoRA glitch model of 11 classes, 6 s of strain with one burst per second, and its scan."""
    from gw_whisper_amd import glitch
    from gw_whisper_amd.glitch_scan import GlitchScanner
    from gw_whisper_amd import ops
    from gw_whisper_amd.inference import DeviceSegmentSlicer, resample
    from gw_whisper_amd.models import _pooled
    T.manual_seed(3)
    model = glitch.build_model("tiny", 11, "DoRA", seed=2).eval()
    wave, _cls, _snr = synth.glitch_segments(6, 11, seed=9, n_samples=2048)
    strain = np.ascontiguousarray(wave.reshape(-1), np.float32)
    # A seeded encoder's pooled token moves by a small fraction of itself from window to window, and a seeded head then puts
    # every window into one class.  The head's first layer is re-centred and re-scaled on this strain's own tokens (mean 0,
    # spread 1 on average) and its last layer widened, so that classes and probabilities change along the series.
    slicer = DeviceSegmentSlicer(strain[None], step_size=0.1)
    with T.no_grad():
        tok = T.cat([_pooled(model.encoder, ops.logmel(resample(slicer.windows(i, min(i + 32, len(slicer)))[:, 0].contiguous())))
                     .to(T.float32) for i in range(0, len(slicer), 32)])
        first_layer = model.classifier[0]
        first_layer.weight.mul_(1.0 / float(tok.std(dim=0).mean()))
        first_layer.bias.sub_(first_layer.weight @ tok.mean(dim=0))
        model.classifier[9].weight.mul_(8.0)
    scanner = GlitchScanner(model, synth.glitch_class_names(11))
    first = scanner.scan(strain, start_time=100.0, batch_size=32, return_windows=True)
    return model, scanner, strain, first


def test_scan_windows_are_the_pieces_one_by_one(T, gww, tiny):
    """51 windows in batches of 32 + 19: the same windows cut out, resampled, through ``ops.logmel``, the pooled encoder
    pass and ``head_forward``, in the same batches."""
    from gw_whisper_amd import ops
    from gw_whisper_amd.inference import DeviceSegmentSlicer, resample
    from gw_whisper_amd.models import _pooled
    model, scanner, strain, r = tiny
    slicer = DeviceSegmentSlicer(strain[None], start_time=100.0, step_size=0.1, peak_offset=0.8)
    n = len(slicer)
    assert n == 51 and r["window_class"].shape == (1, n) and r["window_class"].dtype == np.int32
    assert np.array_equal(r["window_time"][0], slicer.times_host(0, n)) and r["window_time"][0][0] == 100.8
    ps = [p.detach() for p in scanner.params]
    with T.no_grad():
        for i0 in range(0, n, 32):
            i1 = min(n, i0 + 32)
            mel = ops.logmel(resample(slicer.windows(i0, i1)[:, 0].contiguous()))
            tok = _pooled(model.encoder, mel).to(T.float32)
            cls = T.from_numpy(r["window_class"][0, i0:i1]).cuda()
            prob = T.from_numpy(r["window_prob"][0, i0:i1]).cuda()
            check_against_head_forward(T, tok, ps, cls, prob, None)
    assert len(set(r["window_class"][0].tolist())) > 1, "every window fell into one class: the check sees one logit order"


def test_scan_events_are_the_host_events_of_its_windows(T, gww, tiny):
    from gw_whisper_amd.glitch_scan import build_events_host
    model, scanner, strain, first = tiny
    wp = np.sort(first["window_prob"][0])
    assert wp[20] < wp[30], "no spread in the window probabilities"
    thr = float(np.float32(0.5) * (wp[24] + wp[25]))
    for kw in (dict(prob_threshold=thr), dict(prob_threshold=thr, gap=0.15, ignore=[int(first["window_class"][0, 0])])):
        r = scanner.scan(strain, start_time=100.0, batch_size=32, return_windows=True, **kw)
        for k in ("window_class", "window_prob", "window_time"):
            assert np.array_equal(r[k], first[k])
        want = build_events_host(r["window_time"][0], r["window_class"][0], r["window_prob"][0], **kw)
        assert len(want["cls"]) >= 2
        gc.same_bits({"cls": r["class"], "n": r["n_windows"], "t_start": r["time_start"], "t_end": r["time_end"],
                      "t_peak": r["time_peak"], "p_peak": r["prob"]},
                     {k: v for k, v in want.items() if k != "first"})
        assert np.array_equal(r["detector"], np.zeros(len(want["cls"]), np.int32))
    # ignoring by name is ignoring by index
    name = scanner.classes[int(first["window_class"][0, 0])]
    by_name = scanner.scan(strain, start_time=100.0, batch_size=32, prob_threshold=thr, gap=0.15, ignore=[name])
    for k in by_name:
        assert np.array_equal(by_name[k], r[k])


def test_scan_two_detectors_are_two_scans(T, gww, tiny):
    model, scanner, strain, first = tiny
    other = np.ascontiguousarray(synth.glitch_segments(6, 11, seed=10, n_samples=2048)[0].reshape(-1), np.float32)
    thr = float(np.median(first["window_prob"][0]))
    both = scanner.scan(np.stack([strain, other]), start_time=100.0, batch_size=32, prob_threshold=thr, return_windows=True)
    one = [scanner.scan(s, start_time=100.0, batch_size=32, prob_threshold=thr, return_windows=True) for s in (strain, other)]
    assert both["window_class"].shape == (2, 51)
    for k in ("window_class", "window_prob", "window_time"):
        assert np.array_equal(both[k], np.concatenate([o[k] for o in one]))
    assert np.array_equal(one[0]["window_class"], first["window_class"])
    n0 = len(one[0]["class"])
    assert n0 >= 1 and len(one[1]["class"]) >= 1
    assert np.array_equal(both["detector"], np.r_[np.zeros(n0, np.int32), np.ones(len(one[1]["class"]), np.int32)])
    for k in ("class", "time_start", "time_end", "time_peak", "prob", "n_windows"):
        assert np.array_equal(both[k], np.concatenate([o[k] for o in one]))
    # a GPU tensor is scanned where it is; a CPU tensor is refused
    import gw_whisper_amd
    dev = scanner.scan(T.from_numpy(strain).cuda(), start_time=100.0, batch_size=32, prob_threshold=thr)
    assert all(np.array_equal(dev[k], one[0][k]) for k in dev)
    with pytest.raises(gw_whisper_amd.GwwError, match="GPU"):
        scanner.scan(T.from_numpy(strain))


def test_scan_native_front_end_short_context(T, gww):
    """A front end at the strain's own rate (16-point frames every 4 samples, windows of 128 every 8) under a short-context
    encoder (T = 16, d = 128): the sliding path against ``ops.logmel(config=...)`` on the cut windows."""
    from gw_whisper_amd import models, ops
    from gw_whisper_amd.encoder import WhisperConfig, WhisperEncoder
    from gw_whisper_amd.glitch_scan import GlitchScanner, build_events_host
    from gw_whisper_amd.models import _pooled
    cfg = ops.FrontendConfig(80, 2048, 16, 4, 128, 0.0, 1024.0)
    sd = synth.encoder_state_dict(128, 1, 2, 512, seed=11)
    sd["embed_positions.weight"] = sd["embed_positions.weight"][:16].copy()
    enc = WhisperEncoder.from_numpy_state_dict(sd, WhisperConfig(128, 1, 2, 512, max_source_positions=16), precision="bf16")
    T.manual_seed(4)
    model = models.glitch_classifier(enc, num_classes=5).cuda().eval()
    with T.no_grad():
        model.classifier[9].weight.mul_(8.0)
    n_win, step = 11, 8
    x = np.random.default_rng(3).standard_normal(128 + (n_win - 1) * step + 3).astype(np.float32)
    x[140:150] += np.float32(30.0)
    scanner = GlitchScanner(model, [f"c{i}" for i in range(5)], frontend=cfg)
    r = scanner.scan(x, start_time=5.0, step_size=step / 2048.0, peak_offset=0.03, batch_size=4, prob_threshold=0.0,
                     return_windows=True)
    assert ops.last_logmel_windows_route() == "shared" and r["window_class"].shape == (1, n_win)
    dev = T.from_numpy(x).cuda()
    ps = [p.detach() for p in scanner.params]
    with T.no_grad():
        for i0 in range(0, n_win, 4):
            i1 = min(n_win, i0 + 4)
            cut = T.stack([dev[i * step:i * step + 128] for i in range(i0, i1)])
            tok = _pooled(model.encoder, ops.logmel(cut, config=cfg)).to(T.float32)
            check_against_head_forward(T, tok, ps, T.from_numpy(r["window_class"][0, i0:i1]).cuda(),
                                       T.from_numpy(r["window_prob"][0, i0:i1]).cuda(), None)
    want = build_events_host(r["window_time"][0], r["window_class"][0], r["window_prob"][0], prob_threshold=0.0)
    assert len(want["cls"]) >= 1 and int(want["n"].sum()) == n_win                 # every window triggers at threshold 0
    gc.same_bits({"cls": r["class"], "n": r["n_windows"], "t_start": r["time_start"], "t_end": r["time_end"],
                  "t_peak": r["time_peak"], "p_peak": r["prob"]}, {k: v for k, v in want.items() if k != "first"})
    # an extractor of Whisper's published configuration is the default path, not a native one
    from gw_whisper_amd import GwwError
    from gw_whisper_amd.feature_extraction import WhisperFeatureExtractor
    with pytest.raises(GwwError, match="published"):
        GlitchScanner(model, [f"c{i}" for i in range(5)], frontend=WhisperFeatureExtractor())
