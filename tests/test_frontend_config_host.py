"""The configurable front end on the CPU: the ``WhisperFeatureExtractor`` shim for any supported configuration, its
filterbank and its host twin (``gww_logmel_host_cfg_f32``) against HuggingFace's own numbers (tests/golden/
frontend_configs.npz, tools/make_golden_frontend.py), the refusals, the ``preprocessor_config.json`` round trip through
HF itself, and the GAMMA table of tests/frontend_any.py the GPU limits are multiples of.  Nothing here touches a GPU."""

import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import gw_whisper_amd
from gw_whisper_amd import _lib, ops
from gw_whisper_amd.feature_extraction import WhisperFeatureExtractor
from tests import frontend_any as fa

TOL = 1e-5   # the bound tests/test_logmel_host.py holds the default configuration to
IDS = list(range(len(fa.CONFIGS)))


def extractor(i, **kw):
    return WhisperFeatureExtractor(**fa.cfg(i).extractor_kwargs(), **kw)


@pytest.mark.parametrize("i", IDS)
def test_golden_configurations_are_the_helper_s(golden, i):
    g = golden("frontend_configs.npz")
    assert tuple(int(v) for v in g[f"cfg{i}"]) == fa.CONFIGS[i]
    assert int(g[f"near{i}"]) == 0 and int(fa.case(i).near.sum()) == 0     # no element within NEAR of the floor


@pytest.mark.parametrize("i", IDS)
def test_extractor_accepts_and_keeps_hf_names(i):
    c, fe = fa.cfg(i), extractor(i)
    assert (fe.feature_size, fe.sampling_rate, fe.hop_length, fe.chunk_length, fe.n_fft) == \
        (c.n_mels, c.rate, c.hop, c.chunk, c.n_fft)
    assert fe.n_samples == c.n_samples and fe.nb_max_frames == c.n_frames
    assert fe.mel_filters.shape == (c.n_freq, c.n_mels) and fe.mel_filters.dtype == np.float32


BAD = [
    ("n_mels", dict(feature_size=64)),
    ("n_fft", dict(n_fft=127)),
    ("n_fft", dict(n_fft=14)),
    ("n_fft", dict(n_fft=1026)),
    ("hop_length", dict(hop_length=0)),
    ("hop_length", dict(hop_length=129)),
    ("n_samples", dict(sampling_rate=32, chunk_length=2, hop_length=1)),      # 64 samples <= n_fft / 2
    ("n_frames", dict(chunk_length=24)),                                      # 49152 / 16 = 3072 frames
    ("min_frequency", dict(min_frequency=-1.0)),
    ("max_frequency", dict(min_frequency=500.0, max_frequency=500.0)),
    ("chunk_length", dict(chunk_length=0)),
    ("hop_length", dict(hop_length=16.5)),
]


@pytest.mark.parametrize("field,change", BAD, ids=[f"{f}-{i}" for i, (f, _) in enumerate(BAD)])
def test_extractor_refuses_by_field_name(field, change):
    kw = dict(fa.cfg(1).extractor_kwargs(), **change)
    with pytest.raises(ValueError, match=field):
        WhisperFeatureExtractor(**kw)


def test_library_refuses_by_field_name():
    lib = gw_whisper_amd.lib()
    z = np.zeros(4096, np.float32)
    for field, bad in (("n_mels", (64, 2048, 128, 16, 4096, 0, 1024)), ("n_fft", (80, 2048, 2048, 16, 4096, 0, 1024)),
                       ("hop_length", (80, 2048, 128, 200, 4096, 0, 1024)), ("n_samples", (80, 2048, 128, 16, 64, 0, 1024)),
                       ("n_frames", (80, 2048, 128, 1, 4096, 0, 1024)), ("max_frequency", (80, 2048, 128, 16, 4096, 9, 9)),
                       ("min_frequency", (80, 2048, 128, 16, 4096, -1, 1024))):
        cfg = _lib.FrontendCfg(*bad)
        assert lib.gww_logmel_host_cfg_f32(C.byref(cfg), z.ctypes.data, 1, 4096, 4096, z.ctypes.data) == -1
        assert field.encode() in lib.gww_last_error(), (field, lib.gww_last_error())
        h = C.c_void_p()
        assert lib.gww_frontend_create_cfg(C.byref(cfg), C.byref(h)) == -1        # refused before any HIP call
        assert field.encode() in lib.gww_last_error()
        assert lib.gww_frontend_validate_cfg(C.byref(cfg)) == -1                  # the validator on its own, no data
        assert field.encode() in lib.gww_last_error()
    assert lib.gww_frontend_validate_cfg(None) == -1
    for i in IDS:
        c = fa.cfg(i)
        ok = _lib.FrontendCfg(c.n_mels, c.rate, c.n_fft, c.hop, c.n_samples, c.fmin, c.fmax)
        assert lib.gww_frontend_validate_cfg(C.byref(ok)) == 0, lib.gww_last_error()
    with pytest.raises(gw_whisper_amd.GwwError, match="GPU"):
        ops.logmel(torch.zeros(1, 2048), config=ops.FrontendConfig(80, 2048, 128, 16, 4096, 0.0, 1024.0))


@pytest.mark.parametrize("i", IDS)
def test_mel_filters_equal_hf(golden, i):
    """The library's filterbank is HF's float64 one rounded to fp32 (one ulp of slack for the last bit of the fp64 chain)."""
    fb = golden("frontend_configs.npz")[f"fb{i}"]
    got = extractor(i).mel_filters
    assert got.shape == fb.shape
    assert np.array_equal(got == 0, fb.astype(np.float32) == 0)                  # the same support, empty filters included
    np.testing.assert_allclose(got, fb, rtol=2.0 ** -23, atol=1e-12)
    np.testing.assert_array_equal(got, fa.cfg(i).filters())                      # ... and the helper's, bit for bit


@pytest.mark.parametrize("i", IDS)
def test_host_twin_matches_hf(golden, i):
    g, c = golden("frontend_configs.npz"), fa.cfg(i)
    out = extractor(i)(list(fa.waves(i)), sampling_rate=c.rate, return_tensors="np").input_features
    assert out.shape == (fa.N_SEG, c.n_mels, c.n_frames) and out.dtype == np.float32
    ref, live = g[f"hf{i}"], c.live()
    keep = ref.shape[2]
    assert keep == min(c.n_frames, live + 3)
    np.testing.assert_allclose(out[:, :, :keep], ref, atol=TOL, rtol=0)
    for s in range(fa.N_SEG):
        assert np.all(out[s, :, live:] == out[s, 0, c.n_frames - 1]) or live == c.n_frames
        assert abs(out[s, 0, c.n_frames - 1] - g[f"pad{i}"][s]) < TOL
    # ... and the fp64 restatement the GPU test measures against
    np.testing.assert_allclose(out, fa.case(i).out, atol=TOL, rtol=0)


def test_call_surface_of_a_configured_extractor():
    c, fe = fa.cfg(1), extractor(1)
    w = fa.waves(1)
    one = fe(w[0].tolist(), sampling_rate=c.rate, return_tensors="pt").input_features
    assert one.shape == (1, 80, 256) and one.dtype == torch.float32 and one.device.type == "cpu"
    both = fe([w[0], w[1]], sampling_rate=c.rate, return_tensors="pt").input_features
    assert torch.equal(both[0], one[0])
    long = fe(np.concatenate([w[0], w[1], w[0]]), return_tensors="pt").input_features       # truncated at 2 s
    assert torch.equal(long, fe(np.concatenate([w[0], w[1]]), return_tensors="pt").input_features)
    with pytest.raises(ValueError, match="sampling rate of 2048"):
        fe(w[0], sampling_rate=16000)


@pytest.mark.parametrize("i", [1, 4])
def test_save_load_round_trip_and_hf_reads_it(tmp_path, i):
    import transformers
    fe = extractor(i)
    fe.save_pretrained(str(tmp_path))
    back = WhisperFeatureExtractor.from_pretrained(str(tmp_path))
    keys = ("feature_size", "sampling_rate", "hop_length", "chunk_length", "n_fft", "n_samples", "nb_max_frames",
            "padding_value", "min_frequency", "max_frequency")
    assert all(getattr(back, k) == getattr(fe, k) for k in keys)
    np.testing.assert_array_equal(back.mel_filters, fe.mel_filters)
    assert WhisperFeatureExtractor.from_pretrained(str(tmp_path), hop_length=32).nb_max_frames == fe.n_samples // 32
    hf = transformers.WhisperFeatureExtractor.from_pretrained(str(tmp_path))
    assert all(getattr(hf, k) == getattr(fe, k) for k in keys[:8])
    with open(tmp_path / "preprocessor_config.json") as f:
        j = json.load(f)
    assert j["max_frequency"] == fe.max_frequency and j["feature_extractor_type"] == "WhisperFeatureExtractor"


def test_from_pretrained_reads_a_plain_hf_file(tmp_path):
    """A preprocessor_config.json as HF writes it (no frequency keys): every constructor field is read."""
    with open(tmp_path / "preprocessor_config.json", "w") as f:
        json.dump({"feature_size": 128, "sampling_rate": 4000, "hop_length": 25, "chunk_length": 1, "n_fft": 250,
                   "padding_value": 0.0, "n_samples": 4000, "nb_max_frames": 160, "processor_class": "WhisperProcessor"}, f)
    fe = WhisperFeatureExtractor.from_pretrained(str(tmp_path))
    assert (fe.feature_size, fe.sampling_rate, fe.hop_length, fe.chunk_length, fe.n_fft) == (128, 4000, 25, 1, 250)
    assert fe.max_frequency == 8000.0 and fe.nb_max_frames == 160
    assert WhisperFeatureExtractor.from_pretrained("openai/whisper-large-v3").feature_size == 128


@pytest.mark.parametrize("n_mels", [80, 128])
@pytest.mark.parametrize("n", [1, 12345, 16000])
def test_default_configuration_is_the_fixed_entry_point_bitwise(n_mels, n):
    w = fa.waves("default")[:, :n]
    a = ops.logmel_host(w, n_mels=n_mels, config=ops.FrontendConfig(n_mels=n_mels))
    b = ops.logmel_host(w, n_mels=n_mels)
    assert a.shape == (2, n_mels, 3000) and torch.equal(a, b)
    # ... and a default extractor goes on using it
    assert WhisperFeatureExtractor(feature_size=n_mels)._config is None


@pytest.mark.parametrize("i", IDS + ["default"])
def test_ideal_fp32_reproduces_gamma(i):
    g = fa.gamma(i)
    print(f"GAMMA[{i!r}] = {g:.3e} (table {fa.GAMMA[i]:.3e})")
    assert abs(g / fa.GAMMA[i] - 1) <= 0.1


def test_forked_workers_run_a_configured_extractor():
    """The host twin keeps no state and makes no HIP call: it runs inside forked DataLoader workers."""
    c, fe, w = fa.cfg(6), extractor(6), fa.waves(6)

    class DS(torch.utils.data.Dataset):
        def __len__(self):
            return 2

        def __getitem__(self, j):
            return fe(w[j], sampling_rate=c.rate, return_tensors="pt").input_features[0], j

    ref = fe(list(w), return_tensors="pt").input_features
    for x, idx in torch.utils.data.DataLoader(DS(), batch_size=1, num_workers=2, multiprocessing_context="fork"):
        assert torch.equal(x[0], ref[int(idx)])


# ---------------------------------------------------------------------------------------------------- short contexts
def test_with_context_slices_and_keeps_hf_keys(tmp_path):
    from gw_whisper_amd import synth
    from gw_whisper_amd.encoder import WhisperConfig, WhisperEncoder
    sd = synth.encoder_state_dict(128, 2, 2, 512, seed=3)
    enc = WhisperEncoder.from_numpy_state_dict(sd, WhisperConfig(128, 2, 2, 512))
    short = enc.with_context(100)
    assert short.config.max_source_positions == 100 and enc.config.max_source_positions == 1500
    assert set(short.state_dict()) == set(enc.state_dict()) == set(sd)
    for k, v in short.state_dict().items():
        ref = torch.from_numpy(sd[k])
        assert torch.equal(v, ref[:100] if k == "embed_positions.weight" else ref), k
    assert not any(p.requires_grad for p in short.parameters()) and short.precision == enc.precision
    with pytest.raises(ValueError, match="1500 rows"):
        enc.with_context(1501)
    with pytest.raises(ValueError, match="max_source_positions"):
        enc.with_context(8)
    # ... the same encoder by from_pretrained and by a state-dict load of the longer table
    enc.save_pretrained(str(tmp_path))
    a = WhisperEncoder.from_pretrained(str(tmp_path), max_source_positions=100)
    b = WhisperEncoder(WhisperConfig(128, 2, 2, 512, max_source_positions=100))
    b.load_state_dict(enc.state_dict())
    for other in (a, b):
        assert all(torch.equal(v, other.state_dict()[k]) for k, v in short.state_dict().items())
    assert WhisperEncoder.from_pretrained(str(tmp_path)).config.max_source_positions == 1500
    with pytest.raises(RuntimeError, match="size mismatch"):
        WhisperEncoder(WhisperConfig(128, 2, 2, 512)).load_state_dict(short.state_dict())      # a shorter table stays an error
    short.save_pretrained(str(tmp_path / "s"))
    with open(tmp_path / "s" / "config.json") as f:
        assert json.load(f)["max_source_positions"] == 100
    assert WhisperEncoder.from_pretrained(str(tmp_path / "s")).config.max_source_positions == 100


def _train_args(*flags):
    import importlib.util
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("run_train_for_test", os.path.join(root, "harness", "run_train.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod, mod.build_parser().parse_args(list(flags))


def test_run_train_front_end_flags():
    mod, args = _train_args()
    assert mod.frontend_plan(args) == (None, 1500)                              # the default run is untouched
    mod, args = _train_args("--sampling-rate", "2048", "--n-fft", "128", "--hop-length", "16", "--chunk-length", "2",
                            "--mel-fmax", "1024")
    kw, T = mod.frontend_plan(args)
    assert T == 128 and kw == dict(feature_size=80, sampling_rate=2048, hop_length=16, chunk_length=2, n_fft=128,
                                   min_frequency=0.0, max_frequency=1024.0)
    assert WhisperFeatureExtractor(**kw).nb_max_frames == 2 * T
    _, args = _train_args("--chunk-length", "1")
    assert mod.frontend_plan(args)[1] == 50
    _, args = _train_args("--sampling-rate", "2000", "--hop-length", "16", "--n-fft", "128", "--chunk-length", "1")
    with pytest.raises(ValueError, match="125 frames, an odd count"):
        mod.frontend_plan(args)
    _, args = _train_args("--n-fft", "2048")
    with pytest.raises(ValueError, match="n_fft"):
        WhisperFeatureExtractor(**mod.frontend_plan(args)[0])
    h1, l1, labels, snr = mod.synthetic_dataset(6, 1, rate=2048)
    assert h1.shape == l1.shape == (6, 2048) and labels.tolist() == [0, 1, 0, 1, 0, 1]
    a, b = mod.synthetic_dataset(4, 1), mod.synthetic_dataset(4, 1, 16000)
    assert all(np.array_equal(x, y) for x, y in zip(a, b)) and a[0].shape == (4, 16000)


def test_run_evaluation_reads_the_saved_front_end_or_refuses(tmp_path):
    """``saved_front_end``: both files give the saved context and extractor; neither gives Whisper's defaults; one without
    the other, or two that do not fit each other, is an error -- never a silent run on the defaults."""
    import importlib.util
    from gw_whisper_amd.encoder import WhisperConfig, WhisperEncoder
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("run_evaluation_for_test", os.path.join(root, "harness", "run_evaluation.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    import dataclasses
    short = WhisperEncoder(dataclasses.replace(WhisperConfig.named("micro"), max_source_positions=128))
    fe = WhisperFeatureExtractor(sampling_rate=2048, n_fft=128, hop_length=16, chunk_length=2, max_frequency=1024.0)

    def write(name, config=None, extractor=None):
        d = tmp_path / name
        d.mkdir()
        if config is not None:
            with open(d / "config.json", "w") as f:
                json.dump(config, f)
        if extractor is not None:
            extractor.save_pretrained(str(d))
        return str(d)

    config, fe_config, rate = mod.saved_front_end(write("both", short.config_dict(), fe), "micro")
    assert config.max_source_positions == 128 and rate == 2048
    assert fe_config == ops.FrontendConfig(80, 2048, 128, 16, 4096, 0.0, 1024.0) == fe.frontend_config
    config, fe_config, rate = mod.saved_front_end(write("neither"), "micro")
    assert (config, fe_config, rate) == (WhisperConfig.named("micro"), None, 16000)
    # a fully fine-tuned encoder of the default context: config.json alone
    config, fe_config, rate = mod.saved_front_end(write("full", WhisperEncoder(WhisperConfig.named("micro")).config_dict()), "micro")
    assert (config.max_source_positions, fe_config, rate) == (1500, None, 16000)
    with pytest.raises(SystemExit, match="config.json is missing"):
        mod.saved_front_end(write("lost_config", None, fe), "micro")
    with pytest.raises(SystemExit, match="preprocessor_config.json is missing"):
        mod.saved_front_end(write("lost_pre", short.config_dict()), "micro")
    with pytest.raises(SystemExit, match=r"\[80, 100\] features"):
        mod.saved_front_end(write("misfit", short.config_dict(), WhisperFeatureExtractor(chunk_length=1)), "micro")
    with pytest.raises(SystemExit, match="another encoder"):
        mod.saved_front_end(write("other", short.config_dict(), fe), "tiny")
    assert WhisperFeatureExtractor().frontend_config is None
