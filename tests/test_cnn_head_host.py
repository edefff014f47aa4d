"""CPU-side checks of the CNN decoder head: the classifier's layout and state_dict against the reference's class, the
argument errors of the launchers that need no GPU, the training harness' ``--head`` flag."""

import json
import os
import subprocess
import sys

import pytest
import torch
import torch.nn as nn

import gw_whisper_amd
from gw_whisper_amd import models, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "cnn_head_state_dict.json")


class _Cfg:
    d_model = 128


class _Enc(nn.Module):
    config = _Cfg()


def reference_sequential(num_classes=1):
    """The layout of the reference's decoder, slot for slot."""
    return nn.Sequential(nn.Conv1d(in_channels=2, out_channels=64, kernel_size=3, stride=1, padding=1), nn.ReLU(),
                         nn.Conv1d(in_channels=64, out_channels=128, kernel_size=3, stride=1, padding=1), nn.ReLU(),
                         nn.Conv1d(in_channels=128, out_channels=256, kernel_size=3, stride=1, padding=1), nn.ReLU(),
                         nn.AdaptiveAvgPool1d(1), nn.Flatten(), nn.Linear(256, num_classes))


def test_state_dict_keys_and_shapes_are_the_references():
    """tests/golden/cnn_head_state_dict.json: names and shapes of the reference class' classifier.state_dict()
    (num_classes = 1), in order."""
    want = [(k, tuple(s)) for k, s in json.load(open(GOLDEN))]
    m = models.TwoChannelLIGOBinaryClassifierCNN(_Enc(), num_classes=1)
    got = [(k, tuple(v.shape)) for k, v in m.classifier.state_dict().items()]
    assert got == want
    assert [k for k, _ in got] == ["0.weight", "0.bias", "2.weight", "2.bias", "4.weight", "4.bias", "8.weight", "8.bias"]
    kinds = [type(x) for x in m.classifier]
    assert kinds == [nn.Conv1d, nn.ReLU, nn.Conv1d, nn.ReLU, nn.Conv1d, nn.ReLU, nn.AdaptiveAvgPool1d, nn.Flatten, nn.Linear]
    for i in (0, 2, 4):
        assert m.classifier[i].kernel_size == (3,) and m.classifier[i].padding == (1,) and m.classifier[i].stride == (1,)
    m5 = models.TwoChannelLIGOBinaryClassifierCNN(_Enc(), num_classes=5)
    assert tuple(m5.classifier[8].weight.shape) == (5, 256)


def test_state_dict_round_trip_with_the_reference_layout(tmp_path):
    torch.manual_seed(0)
    ours = models.TwoChannelLIGOBinaryClassifierCNN(_Enc(), num_classes=1)
    path = str(tmp_path / "best_dense_layers_8_32.pth")
    torch.save(ours.classifier.state_dict(), path)
    ref = reference_sequential()
    ref.load_state_dict(torch.load(path))                      # strict: ours loads there
    x = torch.randn(2, 2, 128)
    assert torch.equal(ref(x), ours.classifier(x))
    torch.manual_seed(1)
    ref2 = reference_sequential()
    torch.save(ref2.state_dict(), path)
    ours.classifier.load_state_dict(torch.load(path))          # ... and the reference's loads here
    assert torch.equal(ref2(x), ours.classifier(x))
    # head="torch" is the plain nn.Sequential, also on the CPU
    tor = models.TwoChannelLIGOBinaryClassifierCNN(_Enc(), num_classes=1, head="torch")
    tor.classifier.load_state_dict(ref2.state_dict())
    assert torch.equal(tor.decode(x), ref2(x))
    with pytest.raises(gw_whisper_amd.GwwError, match="head="):
        models.TwoChannelLIGOBinaryClassifierCNN(_Enc(), head="mlp")


def test_cpu_input_raises():
    seq = reference_sequential()
    params = [t.detach() for i in (0, 2, 4, 8) for t in (seq[i].weight, seq[i].bias)]
    with pytest.raises(gw_whisper_amd.GwwError, match="GPU"):
        ops.cnn_head_forward(torch.zeros(1, 2, 128), params)
    with pytest.raises(gw_whisper_amd.GwwError, match="GPU"):
        models.TwoChannelLIGOBinaryClassifierCNN(_Enc()).decode(torch.zeros(1, 2, 128))
    with pytest.raises(gw_whisper_amd.GwwError, match="GPU"):
        ops.cnn_head_backward((torch.zeros(1, 2, 128), params, torch.zeros(1, 448, 128)), torch.zeros(1, 1))


def test_unsupported_geometry_is_an_argument_error_without_a_gpu():
    lib = gw_whisper_amd.lib()
    null = [None] * 9
    for B, d, Cn, word in ((1, 192, 1, b"d=192"), (1, 256, 1, b"d=256"), (1, 384, 0, b"C=0"), (1, 384, 65, b"C=65"),
                           (0, 384, 1, b"B=0")):
        assert lib.gww_cnn_head_forward_f32(*null, B, d, Cn, None, None, None) == -1
        assert word in lib.gww_last_error()
        assert lib.gww_cnn_head_backward_f32(*[None] * 7, B, d, Cn, *[None] * 10, 0, None) == -1
        assert word in lib.gww_last_error()
        assert lib.gww_cnn_head_workspace_bytes(B, d, Cn) == 0
    assert lib.gww_cnn_head_forward_f32(*null, 1, 384, 1, None, None, None) == -1      # supported geometry, NULL pointers
    assert b"NULL" in lib.gww_last_error()
    for d in (128, 384, 512, 768, 1024, 1280):
        assert lib.gww_cnn_head_workspace_bytes(2, d, 3) > 2 * 448 * d * 4
        assert lib.gww_cnn_head_saved_bytes(2, d) == 2 * 448 * d * 4
    assert lib.gww_cnn_head_saved_bytes(2, 100) == 0


def test_run_train_help_lists_head_with_default_mlp():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "harness", "run_train.py"), "--help"], capture_output=True,
                         text=True, check=True).stdout
    assert "--head {mlp,cnn}" in out
    src = open(os.path.join(ROOT, "harness", "run_train.py")).read()
    assert 'choices=("mlp", "cnn"), default="mlp"' in src
