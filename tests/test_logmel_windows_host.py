"""``gww_logmel_windows_plan`` (plain C++ in csrc/logmel_host.cpp, no GPU): its frame counts against a brute-force count,
the route rule, the refusals; and ``harness/run_real_events.py``'s pick-up of a saved front end (argument handling only)."""

import dataclasses
import json
import os
import sys

import pytest

import gw_whisper_amd
from gw_whisper_amd import ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def config(n_fft, hop, L, n_mels=80):
    return ops.FrontendConfig(n_mels, 2048, n_fft, hop, L, 0.0, 1024.0)


def brute_force(n_fft, hop, L, step, n):
    """Loop over windows and frames: a frame is an edge when t hop < n_fft / 2 or t hop + n_fft / 2 > L; the centres (in
    samples of the series) of the interior ones go into a set."""
    H, F = n_fft // 2, L // hop
    lo = hi = 0
    centres = set()
    for w in range(n):
        for t in range(F):
            if t * hop < H:
                lo += 1
            elif t * hop + H > L:
                hi += 1
            else:
                centres.add(w * step + t * hop)
    assert lo % n == 0 and hi % n == 0
    return {"edge_lo": lo // n, "edge_hi": hi // n, "interior": F - lo // n - hi // n, "stream_frames": len(centres),
            "dft_frames_shared": len(centres) + lo + hi, "dft_frames_per_window": n * F}


CASES = [
    (16, 4, 128, 8),
    (18, 6, 132, 12),        # n_fft / 2 is no multiple of the hop
    (16, 16, 256, 32),       # hop = n_fft: no edge frame at the end
    (128, 12, 2048, 204),
    (16, 4, 128, 4),         # step = hop
    (16, 4, 128, 128),       # step = L
    (400, 160, 16000, 1600),
    (64, 8, 2048, 200),
]


@pytest.mark.parametrize("n_fft,hop,L,step", CASES)
@pytest.mark.parametrize("n", [1, 2, 7, 256])
def test_plan_counts_against_brute_force(n_fft, hop, L, step, n):
    plan = ops.logmel_windows_plan(config(n_fft, hop, L), step, n)
    want = brute_force(n_fft, hop, L, step, n)
    assert {k: plan[k] for k in want} == want
    shared = step % hop == 0 and want["dft_frames_shared"] < want["dft_frames_per_window"]
    assert plan["route"] == ("shared" if shared else "per_window")
    if shared:
        floats = 80 * (want["stream_frames"] + n * (want["edge_lo"] + want["edge_hi"]))
    else:
        floats = n
    assert plan["workspace_bytes"] == -(-4 * floats // 16) * 16


def test_the_workload_s_counts():
    """n_fft 128, hop 12, windows of 2048 every 204: 6 + 160 + 4 frames, 17 (n - 1) + 160 stream frames."""
    for n in (1, 2, 256, 1000):
        plan = ops.logmel_windows_plan(config(128, 12, 2048), 204, n)
        assert (plan["edge_lo"], plan["interior"], plan["edge_hi"]) == (6, 160, 4)
        assert plan["stream_frames"] == 17 * (n - 1) + 160
        assert plan["dft_frames_shared"] == 17 * (n - 1) + 160 + 10 * n and plan["dft_frames_per_window"] == 170 * n
        assert plan["route"] == ("shared" if n > 1 else "per_window")       # one window shares nothing
    plan = ops.logmel_windows_plan(config(128, 12, 2048), 204, 256)
    assert (plan["dft_frames_per_window"], plan["dft_frames_shared"]) == (43520, 7055)      # 6.17 x fewer DFTs
    assert ops.logmel_windows_plan(config(16, 16, 256), 32, 4)["edge_hi"] == 0
    assert ops.logmel_windows_plan(config(128, 12, 2048, n_mels=128), 204, 2)["workspace_bytes"] == 4 * 128 * (177 + 20)


def test_routes():
    assert ops.logmel_windows_plan(config(16, 4, 128), 8, 5)["route"] == "shared"
    # a step that is no multiple of the hop: no frame of one window is a frame of another
    p = ops.logmel_windows_plan(config(16, 4, 128), 10, 5)
    assert p["route"] == "per_window" and p["stream_frames"] == 5 * p["interior"]
    # windows 4 L apart share nothing
    p = ops.logmel_windows_plan(config(16, 4, 128), 4 * 128, 5)
    assert p["route"] == "per_window" and p["dft_frames_shared"] == p["dft_frames_per_window"]
    # n_fft 64 on windows of 40 samples: every frame is an edge
    p = ops.logmel_windows_plan(config(64, 8, 40), 8, 5)
    assert (p["route"], p["interior"], p["stream_frames"]) == ("per_window", 0, 0) and p["edge_lo"] + p["edge_hi"] == 5
    assert p == {**p, **brute_force(64, 8, 40, 8, 5)}


def test_every_refusal_names_its_argument():
    import torch
    c = config(16, 4, 128)
    for kw, name in ((dict(step=0, n_windows=4), "step=0"), (dict(step=-8, n_windows=4), "step=-8"),
                     (dict(step=8, n_windows=0), "n_windows=0"), (dict(step=8, n_windows=-1), "n_windows=-1")):
        with pytest.raises(gw_whisper_amd.GwwError, match=name):
            ops.logmel_windows_plan(c, **kw)
    with pytest.raises(gw_whisper_amd.GwwError, match="n_fft=17"):
        ops.logmel_windows_plan(dataclasses.replace(c, n_fft=17), 8, 4)
    with pytest.raises(gw_whisper_amd.GwwError, match="hop_length=0"):
        ops.logmel_windows_plan(dataclasses.replace(c, hop_length=0), 8, 4)
    # ops.logmel_windows checks what needs no device before it looks at the tensor: a series too short for the last window
    x = torch.zeros(2, 128 + 3 * 8)                       # four windows fit
    with pytest.raises(gw_whisper_amd.GwwError, match=r"n_windows=5: a series of 152 samples holds 4 window"):
        ops.logmel_windows(x, c, 8, n_windows=5)
    with pytest.raises(gw_whisper_amd.GwwError, match=r"n_windows=3: .* holds 2 window"):
        ops.logmel_windows(x, c, 8, w0=2, n_windows=3)
    with pytest.raises(gw_whisper_amd.GwwError, match="w0=-1"):
        ops.logmel_windows(x, c, 8, w0=-1)
    with pytest.raises(gw_whisper_amd.GwwError, match="step=0"):
        ops.logmel_windows(x, c, 0)
    with pytest.raises(gw_whisper_amd.GwwError, match="route='shared' is refused"):
        ops.logmel_windows(x, c, 10, route="shared")
    with pytest.raises(gw_whisper_amd.GwwError, match="GPU"):          # and there is no CPU path behind the checks
        ops.logmel_windows(x, c, 8)
    # the C entry refuses a NULL handle before any HIP call
    assert gw_whisper_amd.lib().gww_logmel_windows_f32(None, None, 1, 152, 152, 8, 0, 4, None, 0, None, 0, -1, None) == -1
    assert b"NULL" in gw_whisper_amd.lib().gww_last_error()
    assert ops.last_logmel_windows_route() is None or ops.last_logmel_windows_route() in ("shared", "per_window")


def test_native_adapter_refuses_another_window_length():
    import torch
    from gw_whisper_amd.inference import NativeMelAdapter
    a = NativeMelAdapter(config(16, 4, 128))
    with pytest.raises(gw_whisper_amd.GwwError, match=r"windows of 2048 samples but config.n_samples is 128"):
        a(torch.zeros(1, 2, 2048))
    with pytest.raises(gw_whisper_amd.GwwError, match=r"windows of 2048 samples but config.n_samples is 128"):
        a.from_series(torch.zeros(2, 4096), 204, 0, 2, window=2048)


def test_run_real_events_picks_up_a_saved_front_end(tmp_path):
    """``front_end(args)``: a directory with preprocessor_config.json + config.json gives that configuration and context,
    flags override it, and without the files (and flags) the default run is what it was: no configuration at all."""
    from gw_whisper_amd.encoder import WhisperConfig, WhisperEncoder
    from gw_whisper_amd.feature_extraction import WhisperFeatureExtractor
    sys.path.insert(0, os.path.join(ROOT, "harness"))
    import run_real_events
    parse = run_real_events.build_parser().parse_args
    base = ["--timeseries_data_test", "x.npz", "--encoder", "micro"]

    plain = tmp_path / "plain"
    plain.mkdir()
    args = parse(base + ["--lora_weights_file", str(plain)])
    config, fe, window = run_real_events.front_end(args)
    assert fe is None and window == 2048 and config == WhisperConfig.named("micro") and args.step_samples == 204

    saved = tmp_path / "saved"
    saved.mkdir()
    short = WhisperEncoder(dataclasses.replace(WhisperConfig.named("micro"), max_source_positions=85))
    with open(saved / "config.json", "w") as f:
        json.dump(short.config_dict(), f)
    WhisperFeatureExtractor(sampling_rate=2048, n_fft=128, hop_length=12, chunk_length=1, max_frequency=1024.0).save_pretrained(str(saved))
    config, fe, window = run_real_events.front_end(parse(base + ["--lora_weights_file", str(saved)]))
    assert fe == ops.FrontendConfig(80, 2048, 128, 12, 2048, 0.0, 1024.0) and window == 2048
    assert config.max_source_positions == 85
    # flags override what was saved (and work without saved files)
    config, fe, window = run_real_events.front_end(parse(base + ["--lora_weights_file", str(saved), "--mel-fmax", "512"]))
    assert fe == ops.FrontendConfig(80, 2048, 128, 12, 2048, 0.0, 512.0)
    config, fe, window = run_real_events.front_end(parse(base + ["--lora_weights_file", str(plain), "--sampling-rate", "2048",
                                                                 "--n-fft", "128", "--hop-length", "16", "--mel-fmax", "1024"]))
    assert fe == ops.FrontendConfig(80, 2048, 128, 16, 2048, 0.0, 1024.0) and window == 2048
    assert config.max_source_positions == 64                  # 128 frames: conv2 halves them
    with pytest.raises(SystemExit, match="config.json is missing"):
        (tmp_path / "lost").mkdir()
        WhisperFeatureExtractor(sampling_rate=2048, n_fft=128, hop_length=12, chunk_length=1).save_pretrained(str(tmp_path / "lost"))
        run_real_events.front_end(parse(base + ["--lora_weights_file", str(tmp_path / "lost")]))
