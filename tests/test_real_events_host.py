"""CPU-side checks of the catalogue-event scan (gw_whisper_amd/real_events.py, harness/run_real_events.py): the window
grid, event names, the ``.npz`` twin reader, event selection, and the refusals that need no GPU."""

import os
import sys

import numpy as np
import pytest
import torch

import gw_whisper_amd
from gw_whisper_amd import real_events

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "harness"))

KEYS = ["GW150914-v3", "GW170817-v2", "GW190521_074359-v1"]


def write_twin(path, keys=KEYS, n=2660, lengths=None, seed=0):
    rng = np.random.default_rng(seed)
    arrays = {}
    for i, k in enumerate(keys):
        m = lengths[i] if lengths else n
        arrays[f"{k}/h1_strain"] = rng.standard_normal(m)
        arrays[f"{k}/l1_strain"] = rng.standard_normal(m)
    np.savez(path, **arrays)
    return arrays


@pytest.mark.parametrize("n", [2047, 2048, 2251, 2252, 8192])
def test_window_starts_is_the_reference_range(n):
    assert list(real_events.window_starts(n)) == list(range(0, n - 2048 + 1, 204))
    assert len(real_events.window_starts(n)) == {2047: 0, 2048: 1, 2251: 1, 2252: 2, 8192: 31}[n]


def test_window_starts_other_sizes():
    assert list(real_events.window_starts(100, 10, 7)) == list(range(0, 91, 7))


def test_event_names():
    assert real_events.event_label("GW150914-v3") == "GW150914"
    assert real_events.event_label("GW190521_074359-v1-extra") == "GW190521_074359"
    assert real_events.event_label("GW170817") == "GW170817"
    assert real_events.event_label("some/dir/GW170817-v2") == "GW170817"       # the reference takes basename first


def test_twin_reader_selection_and_order(tmp_path):
    path = str(tmp_path / "events.npz")
    arrays = write_twin(path)
    assert real_events.event_keys(path) == KEYS
    keys, strain = real_events.read_events(path)
    assert keys == KEYS and strain.shape == (3, 2, 2660) and strain.dtype == np.float32
    for e, k in enumerate(KEYS):                                                 # H1 is detector 0, L1 detector 1
        np.testing.assert_array_equal(strain[e, 0], arrays[f"{k}/h1_strain"].astype(np.float32))
        np.testing.assert_array_equal(strain[e, 1], arrays[f"{k}/l1_strain"].astype(np.float32))
    keys, strain = real_events.read_events(path, [KEYS[2], KEYS[0]])
    assert keys == [KEYS[2], KEYS[0]] and strain.shape == (2, 2, 2660)
    np.testing.assert_array_equal(strain[0, 1], arrays[f"{KEYS[2]}/l1_strain"].astype(np.float32))
    with pytest.raises(gw_whisper_amd.GwwError, match="GW000000"):
        real_events.read_events(path, ["GW000000-v1"])
    # the twin is also found beside an .hdf name when h5py is missing
    if not real_events._have_h5py():
        hdf = str(tmp_path / "events.hdf")
        os.replace(path, hdf + ".npz")
        assert real_events.read_events(hdf)[0] == KEYS
        with pytest.raises(IOError, match="h5py"):
            real_events.read_events(str(tmp_path / "absent.hdf"))


def test_unequal_lengths_are_refused(tmp_path):
    path = str(tmp_path / "ragged.npz")
    write_twin(path, lengths=[2660, 2661, 2660])
    with pytest.raises(gw_whisper_amd.GwwError, match="GW170817-v2"):
        real_events.read_events(path)
    with pytest.raises(gw_whisper_amd.GwwError, match="unequal"):
        real_events.scan_events(None, [np.zeros((2, 2660)), np.zeros((2, 2661))])
    with pytest.raises(gw_whisper_amd.GwwError, match="no window"):
        real_events.scan_events(None, np.zeros((1, 2, 2047)), device="cpu")
    with pytest.raises(gw_whisper_amd.GwwError, match="events, 2, samples"):
        real_events.scan_events(None, np.zeros((2, 2660)))


def test_head_file_mismatch_is_a_clear_error(tmp_path):
    import run_real_events
    from gw_whisper_amd import models
    from tests.test_cnn_head_host import _Enc
    cnn = models.TwoChannelLIGOBinaryClassifierCNN(_Enc()).classifier.state_dict()
    mlp = models.two_channel_ligo_binary_classifier(_Enc()).classifier.state_dict()
    run_real_events.check_head_file(cnn, "cnn", "f.pth")
    run_real_events.check_head_file(mlp, "mlp", "f.pth")
    with pytest.raises(gw_whisper_amd.GwwError, match=r"--head mlp needs a rank-2"):
        run_real_events.check_head_file(cnn, "mlp", "f.pth")
    with pytest.raises(gw_whisper_amd.GwwError, match=r"--head cnn needs a rank-3"):
        run_real_events.check_head_file(mlp, "cnn", "f.pth")
    with pytest.raises(gw_whisper_amd.GwwError, match="0.weight"):
        run_real_events.check_head_file({"weight": torch.zeros(1)}, "cnn", "f.pth")


def test_parser_flags():
    import run_real_events
    p = run_real_events.build_parser()
    a = p.parse_args(["--timeseries_data_test", "x.hdf"])
    assert a.event_name is None and a.head == "mlp" and a.batch_size == 256 and not a.first_window_only
    assert a.encoder == "tiny" and a.output_path.endswith("results_2_detectors_real_events.hdf")
    a = p.parse_args(["--timeseries_data_test", "x.hdf", "--event_name", "A-v1", "B-v2", "--head", "cnn",
                      "--first-window-only", "--lora_weights_file", "l", "--dense_layers_file", "d.pth",
                      "--encoder-weights", "w.pth", "--batch-size", "64"])
    assert a.event_name == ["A-v1", "B-v2"] and a.head == "cnn" and a.first_window_only and a.batch_size == 64
