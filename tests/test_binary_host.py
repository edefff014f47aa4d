"""CPU checks of the binary head step's host side: the fp64 restatement the GPU tests compare against equals the stored
values of the reference's own classifier classes (tests/golden/binary_head.npz, tools/make_golden_binary.py), the stored
cases keep every ReLU away from its kink, ``binary.head_layout`` recognises the two layouts and refuses every other
``nn.Sequential``, and harness/run_train.py's new flags default to today's behaviour and refuse the combinations that name
no model."""

import importlib.util
import os

import numpy as np
import pytest
import torch

from . import binary_helpers as bh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class _Enc:
    def __init__(self, d):
        self.config = type("Cfg", (), {"d_model": d})()


def _run_train():
    spec = importlib.util.spec_from_file_location("run_train_binary", os.path.join(ROOT, "harness", "run_train.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_fixture_holds_the_cases_of_the_helpers(golden):
    g = golden("binary_head.npz")
    assert [tuple(c) for c in g["cases"].tolist()] == list(bh.CASES)
    assert len(g["seeds"]) == len(bh.CASES)


@pytest.mark.parametrize("ci", range(len(bh.CASES)))
def test_fp64_head_equals_the_reference_classes(golden, ci):
    """logits, probs and loss of the helper's fp64 head against the reference's classes to 1e-12, and the margin condition:
    the smallest hidden pre-activation of every stored case is at least 2e-6 from zero."""
    g = golden("binary_head.npz")
    layout, d_in, C, B = bh.CASES[ci]
    x, t = bh.case_inputs(d_in, C, B, int(g["seeds"][ci]))
    params = [torch.from_numpy(p) for p in bh.case_params(ci, layout, d_in, C)]
    loss, z, p, rows, dx, grads, margin = bh.head64(torch.from_numpy(x), params, torch.from_numpy(t))
    assert margin >= bh.MARGIN and float(g[f"head{ci}_margin"]) >= bh.MARGIN
    assert abs(margin - float(g[f"head{ci}_margin"])) <= 1e-12
    assert z.shape == (B, C) and np.abs(z.numpy() - g[f"head{ci}_logits"]).max() <= 1e-12
    assert np.abs(p.numpy() - g[f"head{ci}_probs"]).max() <= 1e-12
    assert abs(float(loss) - float(g[f"head{ci}_loss"])) <= 1e-12
    assert abs(float(rows.sum()) / (B * C) - float(loss)) <= 1e-12
    assert dx.shape == (B, d_in) and [tuple(a.shape) for a in grads] == [tuple(a.shape) for a in params]


@pytest.mark.parametrize("ci", (1, 5))
def test_extreme_rows_move_two_rows_only(golden, ci):
    """The inputs of test_gpu_binary_head.py's +-120 case: two rows reach +-120, every other row keeps its bits, and the
    margin condition still holds."""
    layout, d_in, C, B = bh.CASES[ci]
    x, t = bh.case_inputs(d_in, C, B, int(golden("binary_head.npz")["seeds"][ci]))
    params = bh.case_params(ci, layout, d_in, C)
    x2, hi, lo = bh.with_extreme_rows(x, params, 120.0)
    tp = [torch.from_numpy(p) for p in params]
    z0 = bh.head64(torch.from_numpy(x), tp, torch.from_numpy(t))[1]
    *_, margin = r = bh.head64(torch.from_numpy(x2), tp, torch.from_numpy(t))
    z1 = r[1]
    assert hi != lo and abs(float(z1[hi, 0]) - 120.0) < 1e-2 and abs(float(z1[lo, 0]) + 120.0) < 1e-2
    keep = [i for i in range(B) if i not in (hi, lo)]
    assert np.array_equal(x2[keep], x[keep]) and float((z1[keep] - z0[keep]).abs().max()) <= 1e-12 and float(z0.abs().max()) < 1.0
    assert margin >= bh.MARGIN


def test_layout_recognition():
    from gw_whisper_amd import GwwError, binary, models, ops
    one = models.one_channel_ligo_binary_classifier(_Enc(384), num_classes=1).classifier
    two = models.two_channel_ligo_binary_classifier(_Enc(384), num_classes=3).classifier
    layout, params = binary.head_layout(one)
    assert layout == ops.BIN_HEAD_ONE and [tuple(p.shape) for p in params[0::2]] == [(512, 384), (256, 512), (128, 256),
                                                                                     (64, 128), (1, 64)]
    assert all(p is q for p, q in zip(params, [t for i in (0, 2, 4, 6, 8) for t in (one[i].weight, one[i].bias)]))
    layout, params = binary.head_layout(two)
    assert layout == ops.BIN_HEAD_TWO and [tuple(p.shape) for p in params[0::2]] == [(1024, 768), (512, 1024), (256, 512),
                                                                                     (3, 256)]
    assert list(one.state_dict()) == list(bh.param_keys(bh.ONE)) and list(two.state_dict()) == list(bh.param_keys(bh.TWO))
    foreign = (models.efficiency_classifier(_Enc(384)).classifier,                 # a trailing Softmax
               models.glitch_classifier(_Enc(384), 5).classifier,                  # Dropout slots
               models.TwoChannelLIGOBinaryClassifierCNN(_Enc(384), head="torch").classifier,
               torch.nn.Sequential(torch.nn.Linear(384, 512), torch.nn.ReLU(), torch.nn.Linear(512, 256), torch.nn.ReLU(),
                                   torch.nn.Linear(256, 128), torch.nn.ReLU(), torch.nn.Linear(128, 1)),   # other widths
               torch.nn.Sequential(torch.nn.Linear(384, 1024), torch.nn.Tanh(), torch.nn.Linear(1024, 512), torch.nn.ReLU(),
                                   torch.nn.Linear(512, 256), torch.nn.ReLU(), torch.nn.Linear(256, 1)),   # not a ReLU
               torch.nn.Linear(384, 1))
    for cls in foreign:
        with pytest.raises(GwwError, match="0 2 4 6 8.*0 2 4 6"):
            binary.head_layout(cls)


def test_cpu_tensors_are_refused():
    from gw_whisper_amd import GwwError, binary, models
    one = models.one_channel_ligo_binary_classifier(_Enc(128)).classifier
    with pytest.raises(GwwError, match="GPU"):
        binary.head_bce_with_logits(one, torch.zeros(2, 128), torch.zeros(2, 1))
    with pytest.raises(GwwError, match="GPU"):
        binary.head_logits(one, torch.zeros(2, 128))


def test_workspace_bytes_and_argument_errors_without_gpu():
    import gw_whisper_amd
    lib = gw_whisper_amd.lib()
    assert lib.gww_bin_head_workspace_bytes(1, 3, 1) == 3 * (512 + 256 + 128 + 64 + 1) * 4
    assert lib.gww_bin_head_workspace_bytes(2, 33, 64) == 33 * (1024 + 512 + 256 + 64) * 4
    assert lib.gww_bin_head_workspace_bytes(3, 33, 64) == 0 and lib.gww_bin_head_workspace_bytes(1, 0, 1) == 0
    from gw_whisper_amd import _lib
    nul = _lib.C.byref(_lib.MlpParams(5))         # five layers, every pointer NULL
    assert lib.gww_bin_head_scores_f32(3, None, nul, 1, 128, 1, None, None) == -1 and b"layout" in lib.gww_last_error()
    assert lib.gww_bin_head_scores_f32(2, None, nul, 1, 1408, 1, None, None) == -1 and b"256" in lib.gww_last_error()
    assert lib.gww_bin_head_scores_f32(1, None, nul, 1, 1408, 1, None, None) == -1 and b"128" in lib.gww_last_error()
    assert lib.gww_bin_head_scores_f32(1, None, nul, 1, 128, 65, None, None) == -1 and b"C=65" in lib.gww_last_error()
    assert lib.gww_bin_head_scores_f32(1, None, nul, 1, 128, 1, None, None) == -1 and b"NULL" in lib.gww_last_error()


def test_a_block_of_the_wrong_layer_count_is_refused_without_gpu():
    """The two-detector head has four layers: a five-layer block is refused, and the text names both counts."""
    import gw_whisper_amd
    from gw_whisper_amd import _lib
    lib = gw_whisper_amd.lib()
    p = 1 << 12                                   # non-NULL, 16-byte aligned stand-in: nothing is dereferenced before the checks
    five = (_lib.C.c_void_p * 5)(*([p] * 5))
    block = _lib.MlpParams(5, five, five)
    assert lib.gww_bin_head_scores_f32(2, p, _lib.C.byref(block), 1, 256, 1, p, None) == -1
    msg = lib.gww_last_error().decode()
    assert "gww_bin_head_scores_f32" in msg and "n_layers=5" in msg and "4 layers" in msg
    block.n_layers = 4
    assert lib.gww_bin_head_scores_f32(1, p, _lib.C.byref(block), 1, 128, 1, p, None) == -1
    msg = lib.gww_last_error().decode()
    assert "n_layers=4" in msg and "5 layers" in msg


def test_models_pooled_is_what_forward_feeds_the_classifier():
    from gw_whisper_amd import models

    class Enc(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.config = type("Cfg", (), {"d_model": 128})()

        def last_token(self, mel):
            return mel[:, :128, 0] * 2.0
    a, b = torch.randn(3, 128, 2, generator=torch.Generator().manual_seed(1)), torch.randn(3, 128, 2)
    one = models.one_channel_ligo_binary_classifier(Enc())
    two = models.two_channel_ligo_binary_classifier(Enc())
    assert one.pooled(a).shape == (3, 128) and two.pooled(a, b).shape == (3, 256)
    assert torch.equal(one(a), one.classifier(one.pooled(a)))
    assert torch.equal(two(a, b), two.classifier(two.pooled(a, b)))
    assert torch.equal(two.pooled(a, b), torch.cat((a[:, :, 0], b[:, :, 0]), dim=1) * 2.0)


def test_harness_defaults_are_unchanged_and_bad_combinations_raise():
    rt = _run_train()
    parser = rt.build_parser()
    a = parser.parse_args([])
    assert (a.detectors, a.head_step, a.head, a.method, a.precision) == (2, "torch", "mlp", "DoRA", "bf16")
    assert (a.batch_size, a.num_epochs, a.learning_rate, a.test_size, a.encoder, a.seed) == (32, 1, 1e-4, 0.2, "tiny", 42)
    assert (a.lora_rank, a.lora_alpha, a.synthetic) == (8, 32, 0) and a.lora_targets == list(rt.DEFAULT_LORA_TARGETS)
    assert a.models_path == "Detection/results/Two_detectors/models"
    rt.check_args(a)
    ok = parser.parse_args(["--detectors", "1", "--head-step", "hip", "--method", "full_finetune"])
    assert (ok.detectors, ok.head_step) == (1, "hip")
    rt.check_args(ok)
    rt.check_args(parser.parse_args(["--head", "cnn"]))
    with pytest.raises(ValueError, match="--detectors 1 --head cnn"):
        rt.check_args(parser.parse_args(["--detectors", "1", "--head", "cnn"]))
    with pytest.raises(ValueError, match="--head-step hip --head cnn"):
        rt.check_args(parser.parse_args(["--head-step", "hip", "--head", "cnn"]))
    with pytest.raises(SystemExit):
        parser.parse_args(["--detectors", "3"])
    with pytest.raises(SystemExit):
        parser.parse_args(["--head-step", "triton"])
