"""CPU-side checks of the MLGWSC-1 training program (harness/run_mlgwsc_train.py, gw_whisper_amd/mlgwsc_train.py): the
command line of the reference, the dataset reader, the batch planner against the reference's own draws
(tests/golden/mlgwsc_train.npz, tools/make_golden_mlgwsc.py), the refusals that come before any device is touched, and
the new C-ABI entries."""

import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HARNESS = os.path.join(ROOT, "harness", "run_mlgwsc_train.py")

# MLGWSC-1/train.py parse_args (:780-827): (option strings, default, required, nargs, action kind); the reference is not
# on the GPU machines, so the list is held here
REFERENCE_FLAGS = [
    (("--verbose",), False, False, 0, "store_true"),
    (("--debug",), False, False, 0, "store_true"),
    (("--force",), False, False, 0, "store_true"),
    (("--seed",), 42, False, None, "store"),
    (("--deterministic",), False, False, 0, "store_true"),
    (("-d", "--dataset-dir"), None, True, None, "store"),
    (("--n-detectors",), 2, False, None, "store"),
    (("--sample-rate",), 2048, False, None, "store"),
    (("--spectrogram-shape",), [128, 128], False, 2, "store"),
    (("--target-shape",), [80, 3000], False, 2, "store"),
    (("--q-range",), [4, 128], False, 2, "store"),
    (("--kernel-length",), 1.0, False, None, "store"),
    (("-o", "--output-training"), None, True, None, "store"),
    (("--snr",), (5.0, 15.0), False, 2, "store"),
    (("--learning-rate",), 1e-5, False, None, "store"),
    (("--epochs",), 50, False, None, "store"),
    (("--batch-size",), 128, False, None, "store"),
    (("--clip-norm",), 100.0, False, None, "store"),
    (("--num-workers",), 2, False, None, "store"),
    (("--pin-memory",), False, False, 0, "store_true"),
    (("--early-stop-patience",), 10, False, None, "store"),
    (("--num-classes",), 2, False, None, "store"),
    (("--resume",), None, False, "?", "store"),
    (("--train-device",), "cuda", False, None, "store"),
    (("--store-device",), "cpu", False, None, "store"),
    (("--pretrain-steps",), 60000, False, None, "store"),
    (("--pretrain-lr",), 1e-4, False, None, "store"),
    (("--pretrain-temp",), 0.1, False, None, "store"),
    (("--noise-only-prob",), 0.25, False, None, "store"),
    (("--lora-rank",), 8, False, None, "store"),
    (("--lora-alpha",), 32, False, None, "store"),
    (("--use-dora",), False, False, 0, "store_true"),
]
EXTRAS = {"--synthetic": 0, "--encoder": "tiny", "--encoder-weights": None}


def _harness():
    sys.path.insert(0, os.path.join(ROOT, "harness"))
    import run_mlgwsc_train
    return run_mlgwsc_train


def test_flags_and_defaults_are_the_references():
    p = _harness().build_parser()
    acts = {a.option_strings[-1]: a for a in p._actions if a.option_strings and a.dest != "help"}
    ref = {o[-1]: (o, d, req, na, kind) for o, d, req, na, kind in REFERENCE_FLAGS}
    assert set(acts) == set(ref) | set(EXTRAS), sorted(set(acts) ^ (set(ref) | set(EXTRAS)))
    for name, (opts, default, required, nargs, kind) in ref.items():
        a = acts[name]
        assert tuple(a.option_strings) == opts, name
        assert a.default == default and a.required == required, (name, a.default, a.required)
        if kind == "store_true":
            assert a.nargs == 0 and a.const is True, name
        else:
            assert a.nargs == nargs, (name, a.nargs)
    r = acts["--resume"]
    assert r.const == "latest" and list(r.choices) == ["latest", "best"]
    for name, default in EXTRAS.items():
        assert acts[name].default == default
    args = p.parse_args(["-d", "data", "-o", "out", "--resume"])
    assert args.resume == "latest" and args.snr == (5.0, 15.0) and args.q_range == [4, 128]


def test_help_runs_without_a_gpu():
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", CUDA_VISIBLE_DEVICES="")
    r = subprocess.run([sys.executable, HARNESS, "--help"], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stderr
    for flag in ("--pretrain-temp", "--noise-only-prob", "--use-dora", "--synthetic", "--encoder-weights"):
        assert flag in r.stdout


def test_npz_dataset_directory_is_read(tmp_path):
    h = _harness()
    rng = np.random.default_rng(0)
    arrays = {}
    for i, (n, m) in enumerate(((5, 2), (3, 1))):
        arrays[i] = {f"{g}/{k}": rng.standard_normal((c, 2, 16)).astype(np.float32)
                     for g, (a, b) in (("training", (n, m)), ("validation", (n - 1, m))) for k, c in (("noises", a), ("waveforms", b))}
        np.savez(tmp_path / f"part{i}.npz", **arrays[i])
    files = h.read_dataset_dir(str(tmp_path))
    assert [os.path.basename(p) for p, _ in files] == ["part0.npz", "part1.npz"]
    for i, (_, groups) in enumerate(files):
        for g in ("training", "validation"):
            np.testing.assert_array_equal(groups[g][0], arrays[i][f"{g}/noises"])
            np.testing.assert_array_equal(groups[g][1], arrays[i][f"{g}/waveforms"])
    # the reference's ConcatDataset layout: each file keeps its injections-first labelling
    from gw_whisper_amd.mlgwsc_train import BinaryGWDataset, ConcatGWData
    dses = [BinaryGWDataset(*groups["training"]) for _, groups in files]
    cat = ConcatGWData(dses, "cpu")
    assert len(cat) == 8
    idx_n, idx_w, snr = cat.plan(np.arange(8), np.random.default_rng(1))
    np.testing.assert_array_equal(idx_n, np.arange(8))
    np.testing.assert_array_equal(idx_w, [0, 1, -1, -1, -1, 2, -1, -1])
    assert ((snr[idx_w >= 0] >= 5) & (snr[idx_w >= 0] < 15)).all() and (snr[idx_w < 0] == 0).all()


def test_pretrain_planner_reproduces_the_reference_draws(golden):
    from gw_whisper_amd.mlgwsc_train import PretrainDataset
    z = golden("mlgwsc_train.npz")
    ds = PretrainDataset(torch.from_numpy(z["pre_noises"]), torch.from_numpy(z["pre_waves"]), snr_range=(5.0, 15.0),
                         noise_only_prob=float(z["pre_prob"]), device="cpu")
    assert len(ds) == len(z["pre_waves"])
    n1, n2, iw, snr = ds.plan(z["pre_idx"], np.random.default_rng(int(z["pre_seed"])))
    only = z["pre_noise_only"]
    np.testing.assert_array_equal(iw < 0, only)
    np.testing.assert_array_equal(n1, z["pre_n1"])
    np.testing.assert_array_equal(n2, z["pre_n2"])
    np.testing.assert_array_equal(iw[~only], z["pre_idx"][~only])
    np.testing.assert_array_equal(snr, z["pre_snr"].astype(np.float32))


def test_binary_planner_reproduces_the_reference_draws(golden):
    from gw_whisper_amd.mlgwsc_train import BinaryGWDataset
    z = golden("mlgwsc_train.npz")
    ds = BinaryGWDataset(z["bin_noises"], z["bin_waves"])
    assert len(ds) == len(z["bin_noises"])
    idx_n, idx_w, snr = ds.plan(z["bin_idx"], np.random.default_rng(int(z["bin_seed"])))
    inj = z["bin_idx"] < len(z["bin_waves"])
    np.testing.assert_array_equal(idx_n, z["bin_idx"])
    np.testing.assert_array_equal(idx_w, np.where(inj, z["bin_idx"], -1))
    np.testing.assert_array_equal(snr, z["bin_snr"].astype(np.float32))
    np.testing.assert_array_equal(z["bin_labels"], np.where(inj[:, None], [1.0, 0.0], [0.0, 1.0]))
    # the reference's own __getitem__ restated here gives the fixture's signals on the CPU
    ds.rng = np.random.default_rng(int(z["bin_seed"]))
    for k, i in enumerate(z["bin_idx"]):
        x, lab = ds[int(i)]
        np.testing.assert_array_equal(x.numpy(), z["bin_x"][k])
        np.testing.assert_array_equal(lab.numpy(), z["bin_labels"][k])


def test_reg_bce_loss_matches_the_reference(golden):
    from gw_whisper_amd.mlgwsc_train import RegBCELoss
    z = golden("mlgwsc_train.npz")
    p, y = torch.from_numpy(z["bce_p"]), torch.from_numpy(z["bce_y"])
    assert abs(RegBCELoss(dim=2)(p, y).item() - float(z["bce_loss"])) < 1e-6
    assert abs(RegBCELoss(dim=2, epsilon=1e-3)(p, y).item() - float(z["bce_loss_eps"])) < 1e-6


@pytest.fixture
def no_device(monkeypatch):
    def touched(*a, **k):
        raise AssertionError("a device was touched")
    for name in ("is_available", "set_device", "init", "device_count", "current_device"):
        monkeypatch.setattr(torch.cuda, name, touched)


def test_existing_losses_file_is_refused_before_any_device(tmp_path, no_device, monkeypatch):
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    (tmp_path / "losses.txt").write_text("0001\t1.000000\t1.000000\n")
    with pytest.raises(RuntimeError, match="Output file exists"):
        _harness().main(["-d", str(tmp_path), "-o", str(tmp_path), "--synthetic", "8"])


def test_world_size_above_one_is_refused_before_any_device(tmp_path, no_device, monkeypatch):
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(SystemExit, match="WORLD_SIZE=2"):
        _harness().main(["-d", str(tmp_path), "-o", str(tmp_path / "out"), "--synthetic", "8"])


def test_new_entries_are_bound_and_validate_without_gpu():
    import gw_whisper_amd
    from gw_whisper_amd import _lib
    lib = gw_whisper_amd.lib()
    names = ("gww_info_nce_forward_f32", "gww_info_nce_backward_f32", "gww_qadapter_tail_backward_f32",
             "gww_qadapter_tail_backward_workspace_bytes", "gww_assemble_batch_f32")
    header = open(os.path.join(ROOT, "include", "gww.h")).read()
    for n in names:
        assert n in _lib.SIGNATURES and hasattr(lib, n) and f"{n}(" in header
    p = 8   # any non-NULL value: the checks below fail before a pointer is read
    assert lib.gww_info_nce_forward_f32(None, p, 4, 256, 0.1, p, p, p, p, p, None) == -1
    assert b"NULL" in lib.gww_last_error()
    assert lib.gww_info_nce_forward_f32(p, p, 0, 256, 0.1, p, p, p, p, p, None) == -1          # B < 1
    assert lib.gww_info_nce_forward_f32(p, p, 4, 1025, 0.1, p, p, p, p, p, None) == -1         # P > 1024
    assert b"P" in lib.gww_last_error()
    assert lib.gww_info_nce_forward_f32(p, p, 4, 256, 0.0, p, p, p, p, p, None) == -1          # tau <= 0
    assert lib.gww_info_nce_backward_f32(p, p, p, p, 4, 0, 0.1, p, p, p, None) == -1           # P < 1
    assert lib.gww_info_nce_backward_f32(p, None, p, p, 4, 8, 0.1, p, p, p, None) == -1
    assert lib.gww_qadapter_tail_backward_workspace_bytes(32, 32) == 2 * 8 * 32 * 32
    assert lib.gww_qadapter_tail_backward_f32(p, 240000, p, 0, 32, 32, 80, 3000, p, p, p, p, p, 1 << 20,
                                              p, p, p, p, None) == -1                             # B < 1
    assert lib.gww_qadapter_tail_backward_f32(p, 240000, p, 2, 32, 32, 80, 3000, p, p, p, p, p, 8,
                                              p, p, p, p, None) == -3                             # GWW_ERR_WORKSPACE
    assert b"workspace" in lib.gww_last_error()
    assert lib.gww_assemble_batch_f32(p, 4, p, 2, 4096, None, p, p, 8, p, None) == -1
    assert lib.gww_assemble_batch_f32(p, 4, p, 2, 4096, p, p, p, 0, p, None) == -1              # R < 1
