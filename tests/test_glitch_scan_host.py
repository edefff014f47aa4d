"""Host side of the glitch scan (gw_whisper_amd/glitch_scan.py, harness/run_glitch_scan.py): the event semantics as the
sequential program, on hand-written cases with hand-written expectations (tests/glitch_scan_cases.py); the high-pass taps
against scipy; the harness' argument surface, its ``.npz`` round trip and its refusal to overwrite; and the whitening
filter's response form for a filter that is too long for the time-domain kernel from the start."""

import importlib.util
import os

import numpy as np
import pytest

from tests import glitch_scan_cases as gc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("case", gc.HAND_CASES, ids=[c["name"] for c in gc.HAND_CASES])
def test_build_events_host_hand_written(case):
    from gw_whisper_amd.glitch_scan import build_events_host
    got = build_events_host(case["times"], case["cls"], case["prob"], **case["kw"])
    gc.same_bits(got, gc.expected_events(case))


def test_the_stamp_differences_the_cases_rest_on():
    """3 steps of 204 samples are 0.2988 s (below the 0.35 s gap), 4 steps 0.3984 s (above it); 2 steps 0.1992 s."""
    t = gc.stamps(8)
    assert t[0] == 0.8 and gc.STEP == 0.099609375
    assert abs((t[3] - t[0]) - 0.298828125) < 1e-15 and (t[3] - t[0]) < 0.35
    assert abs((t[7] - t[3]) - 0.3984375) < 1e-15 and (t[7] - t[3]) > 0.35
    assert abs((t[2] - t[0]) - 0.19921875) < 1e-15
    # ... and they are the slicer's stamps
    from gw_whisper_amd.inference import DeviceSegmentSlicer
    s = DeviceSegmentSlicer(np.zeros((1, 2048 + 7 * 204), np.float32), start_time=0.0, peak_offset=0.8, device="cpu")
    assert len(s) == 8 and s.index_step_size == 204
    assert np.array_equal(s.times_host(0, 8), np.add.accumulate(np.r_[0.0, np.full(7, gc.STEP)]) + 0.8)


def test_build_events_host_arguments():
    from gw_whisper_amd.glitch_scan import build_events_host, ignore_mask
    e = build_events_host(np.zeros(0), np.zeros(0, np.int32), np.zeros(0, np.float32))
    assert set(e) == set(("cls", "first", "n", "t_start", "t_end", "t_peak", "p_peak")) and all(len(v) == 0 for v in e.values())
    assert e["t_start"].dtype == np.float64 and e["p_peak"].dtype == np.float32 and e["first"].dtype == np.int32
    assert ignore_mask([0, 63]) == (1 << 63) | 1 and ignore_mask(5) == 5 and ignore_mask(()) == 0
    with pytest.raises(ValueError):
        ignore_mask([64])
    with pytest.raises(ValueError):
        build_events_host(np.zeros(3), np.zeros(2, np.int32), np.zeros(3, np.float32))
    # a mask and a list of classes are the same thing
    c = gc.HAND_CASES[7]
    gc.same_bits(build_events_host(c["times"], c["cls"], c["prob"], ignore=1 << 6),
                 build_events_host(c["times"], c["cls"], c["prob"], ignore=[6]))


def test_highpass_taps_are_firwin():
    signal = pytest.importorskip("scipy.signal")
    from gw_whisper_amd.glitch_scan import highpass_taps
    for freq, order, dt, beta in ((30.0, 512, 1.0 / 2048, 5.0), (20.0, 64, 1.0 / 4096, 5.0), (100.0, 7, 1.0 / 2048, 8.6)):
        h = highpass_taps(freq, order, dt, beta)
        ref = signal.firwin(2 * order + 1, freq / (int(1.0 / dt) / 2), window=("kaiser", beta), pass_zero=False)
        assert h.shape == ref.shape and h.dtype == np.float64
        assert np.abs(h - ref).max() <= 1e-15, np.abs(h - ref).max()
        assert np.array_equal(h, h[::-1])                                       # linear phase: the filter is centred
        m = np.arange(2 * order + 1) - order
        assert abs(np.sum(h * np.cos(np.pi * m)) - 1.0) < 1e-12                 # unit gain at the Nyquist frequency
    with pytest.raises(ValueError):
        highpass_taps(2000.0, 8, 1.0 / 2048)


def test_design_filter_too_long_from_the_start_is_the_response_form():
    """4 s of filter at 2048 Hz starts at K = 4096, one past ``K_MAX``: 8 193 taps pad to 8 196 and ``gww_fir_f64`` takes
    8 192.  The design returns ``(None, |fft(q)|)`` for it -- on CPU tensors too -- and still the taps for a short filter."""
    import torch
    from gw_whisper_amd import whiten as wh
    dt, seg = 1.0 / 2048, 4.0
    bins = int(seg / dt) // 2 + 1
    f = torch.arange(bins, dtype=torch.float64) / seg
    psd = (1.0 + 1.0e4 / (1.0 + (f / 20.0) ** 4))[None]                          # a gentle low-frequency rise
    n = 16 * 2048
    mfl = int(4.0 / dt)
    assert max(mfl // 2, 64) == wh.K_MAX + 1
    g, wf = wh.design_filter(psd, 1.0 / seg, n, dt, mfl)
    assert g is None and tuple(wf.shape) == (1, n // 2 + 1) and wf.dtype == torch.float64
    assert bool(torch.isfinite(wf).all()) and float(wf.max()) > 0.0
    g, K = wh.design_filter(psd, 1.0 / seg, n, dt, int(0.25 / dt))
    assert g is not None and isinstance(K, int) and K <= wh.K_MAX and g.shape[1] % 4 == 0 and g.shape[1] >= 2 * K + 1


# ---------------------------------------------------------------------------------------------- the program
def _harness():
    spec = importlib.util.spec_from_file_location("run_glitch_scan", os.path.join(ROOT, "harness", "run_glitch_scan.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_run_glitch_scan_parser():
    gs = _harness()
    a = gs.parse_args(["in.hdf", "out.hdf"])
    assert (a.inputfile, a.outputfile, a.white, a.force) == ("in.hdf", "out.hdf", False, False)
    assert (a.prob_threshold, a.gap, a.step_size, a.batch_size) == (0.5, 0.35, 0.1, 256)
    assert (a.encoder, a.method, a.lora_rank, a.lora_alpha, a.precision) == ("tiny", "DoRA", 8, 32, "bf16")
    assert a.ignore_class == [] and a.window_output is None and a.synthetic is None and a.classes is None
    a = gs.parse_args(["i", "o", "--white", "--force", "--encoder", "base", "--method", "LoRA", "--lora_weights_path", "L",
                       "--dense_weights_path", "D", "--lora_rank", "4", "--lora_alpha", "16", "--precision", "fp32",
                       "--encoder-weights", "E", "--lora-targets", "layers.*.fc1", "--classes", "c.json", "--ignore-class",
                       "No Glitch", "Blip", "--prob-threshold", "0.7", "--gap", "0.5", "--step-size", "0.05", "--batch-size",
                       "64", "--window-output", "w.npz", "--synthetic", "12.5"])
    assert a.white and a.force and (a.encoder, a.method, a.lora_weights_path, a.dense_weights_path) == ("base", "LoRA", "L", "D")
    assert (a.lora_rank, a.lora_alpha, a.precision, a.encoder_weights, a.lora_targets) == (4, 16, "fp32", "E", ["layers.*.fc1"])
    assert a.classes == "c.json" and a.ignore_class == ["No Glitch", "Blip"] and a.window_output == "w.npz"
    assert (a.prob_threshold, a.gap, a.step_size, a.batch_size, a.synthetic) == (0.7, 0.5, 0.05, 64, 12.5)


def test_run_glitch_scan_npz_round_trip_and_refusals(tmp_path, monkeypatch):
    gs = _harness()
    classes = ["Blip", "GW", "Koi Fish"]
    ev = lambda k: {"detector": np.zeros(k, np.int32), "class": np.arange(k, dtype=np.int32) % 3,        # noqa: E731
                    "n_windows": np.full(k, 2, np.int32), "time_start": 10.0 + np.arange(k), "time_end": 10.5 + np.arange(k),
                    "time_peak": 10.25 + np.arange(k), "prob": np.full(k, 0.75, np.float32)}
    packed = gs.pack_events({"200": ev(2), "100": ev(0), "300": ev(3)}, ["300", "200", "100"], classes)
    out = str(tmp_path / "events.npz")
    gs.write_result(out, packed)
    z = np.load(out)
    assert sorted(z.files) == sorted(["segment", *gs.EVENT_FIELDS, "class_names", "segment_keys"])
    assert z["segment"].tolist() == [0, 0, 0, 1, 1] and z["segment"].dtype == np.int32
    assert [s.decode() for s in z["class_names"]] == classes and [s.decode() for s in z["segment_keys"]] == ["300", "200", "100"]
    assert z["class"].tolist() == [0, 1, 2, 0, 1] and z["class"].dtype == np.int32 and z["prob"].dtype == np.float32
    assert z["time_peak"].tolist() == [10.25, 11.25, 12.25, 10.25, 11.25] and z["time_peak"].dtype == np.float64
    empty = gs.pack_events({}, [], classes)
    assert all(len(empty[f]) == 0 for f in ("segment", *gs.EVENT_FIELDS))
    # refusals that need no device: an existing output without --force, an unknown --ignore-class, more than one rank
    with pytest.raises(RuntimeError, match="--force"):
        gs.main(["in.npz", out])
    win = str(tmp_path / "w.npz")
    np.savez(win, a=np.zeros(1))
    with pytest.raises(RuntimeError, match="Window file"):
        gs.main(["in.npz", str(tmp_path / "new.npz"), "--window-output", win])
    cj = tmp_path / "m_classes.json"
    cj.write_text('["Blip", "GW"]')
    with pytest.raises(SystemExit, match="ignore-class"):
        gs.main(["in.npz", str(tmp_path / "new.npz"), "--classes", str(cj), "--ignore-class", "Whistle"])
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(SystemExit, match="one rank"):
        gs.main(["in.npz", str(tmp_path / "new.npz")])
    monkeypatch.delenv("WORLD_SIZE")
    import torch
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)              # the refusal is checked on GPU machines too
    with pytest.raises(SystemExit, match="no GPU"):
        gs.main(["in.npz", str(tmp_path / "new.npz"), "--force"])


def test_scan_refuses_cpu_tensors():
    import torch
    from gw_whisper_amd import GwwError, glitch_scan, ops
    with pytest.raises(GwwError, match="GPU"):
        ops.head_scan(torch.zeros(2, 384), [torch.zeros(1)] * 8)
    with pytest.raises(GwwError, match="GPU"):
        ops.glitch_events(torch.zeros(3, dtype=torch.float64), torch.zeros(3, dtype=torch.int32), torch.zeros(3))
    with pytest.raises(GwwError, match="GPU"):
        glitch_scan.condition(torch.zeros(4096), 1.0 / 2048, device="cpu")
