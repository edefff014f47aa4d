"""CPU-side checks of the glitch-classification programs (gw_whisper_amd/glitch.py, harness/run_glitch_train.py,
harness/run_glitch_evaluate.py) against tests/golden/glitch_train.npz (tools/make_golden_glitch.py: the reference's head
class, its label transformation + sklearn's LabelEncoder, sklearn's classification_report)."""

import importlib.util
import json
import os

import numpy as np
import pytest
import torch

import gw_whisper_amd
from gw_whisper_amd import glitch, synth

from . import glitch_helpers as gh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _program(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "harness", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_label_transformation_and_class_order_equal_the_reference(golden):
    g = golden("glitch_train.npz")
    raw = [str(s) for s in g["labels_raw"]]
    assert [glitch.modify_label(s) for s in raw] == [str(s) for s in g["labels_modified"]]
    classes = glitch.fit_classes(raw)
    assert classes == [str(s) for s in g["labels_classes"]]
    assert classes.index("1080Lines") < classes.index("Blip") < classes.index("GW") < classes.index("Koi Fish")
    assert np.array_equal(glitch.encode_labels(raw, classes), g["labels_encoded"])
    with pytest.raises(ValueError, match="unseen"):
        glitch.encode_labels(["never_seen"], classes)


def test_classification_report_equals_sklearn_byte_for_byte(golden):
    g = golden("glitch_train.npz")
    y_true, y_pred, names = g["report_y_true"], g["report_y_pred"], [str(s) for s in g["report_names"]]
    cm = np.zeros((len(names), len(names)), np.int64)
    np.add.at(cm, (y_true, y_pred), 1)
    assert np.array_equal(cm, g["report_confusion"])
    assert cm[2].sum() == 0 and cm[:, 2].sum() > 0         # class 2: absent from the truth, predicted
    assert cm[:, 4].sum() == 0 and cm[4].sum() > 0         # class 4: in the truth, never predicted
    assert glitch.classification_report(cm, names) == str(g["report_text"])
    assert abs(glitch.macro_f1(cm) - float(g["report_macro_f1"])) <= 1e-12
    with pytest.raises(ValueError):
        glitch.classification_report(cm, names[:-1])


def test_float64_restatement_of_the_head_step_equals_the_reference_head(golden):
    """The restatement tests/test_gpu_glitch.py measures the HIP step against (glitch_helpers.head64) reproduces what the
    reference's own head class gave in fp64, eval mode and train mode under the recorded mask: logits, loss and the digest
    of every gradient tensor to 1e-11."""
    g = golden("glitch_train.npz")
    for ci, (d_in, C, B) in enumerate(g["head_cases"].tolist()):
        x, y, masks = gh.case_inputs(d_in, C, B, int(g["head_seeds"][ci]))
        params = [torch.from_numpy(p) for p in gh.case_params(ci, d_in, C)]
        for mode in ("eval", "train"):
            m = [torch.from_numpy(t) for t in masks] if mode == "train" else None
            loss, logits, dx, grads, margin = gh.head64(torch.from_numpy(x), params, torch.from_numpy(y), m)
            assert np.abs(logits.numpy() - g[f"head{ci}_{mode}_logits"]).max() <= 1e-11
            assert abs(float(loss) - float(g[f"head{ci}_{mode}_loss"])) <= 1e-11
            for key, t, name in [(0, dx, "dx")] + [(1 + k, grads[k], f"grad{k}") for k in range(8)]:
                want = g[f"head{ci}_{mode}_{name}"]
                assert np.abs(gh.digest(t.numpy(), key) - want).max() <= 1e-11 * max(1.0, np.abs(want).max()), (ci, mode, name)
            assert margin >= 2e-6
        assert g[f"head{ci}_margins"][0] >= 1e-4


def test_saved_adapter_state_dict_has_peft_runtime_keys_and_reloads(tmp_path):
    model = glitch.build_model("micro", 4, "DoRA", 8, 32, device="cpu")
    peft_keys = set(model.encoder.state_dict().keys())
    assert "base_model.model.layers.0.self_attn.q_proj.base_layer.weight" in peft_keys
    assert "base_model.model.layers.0.self_attn.q_proj.lora_A.default.weight" in peft_keys
    assert "base_model.model.layers.1.self_attn.v_proj.lora_magnitude_vector.default.weight" in peft_keys
    assert sum(k.endswith("lora_A.default.weight") for k in peft_keys) == 6      # q, k, v of two layers; o_proj matches nothing
    assert all(("lora" in n) == p.requires_grad for n, p in model.encoder.named_parameters())
    path = os.path.join(tmp_path, "m_best_lora_weights.pth")
    with torch.no_grad():
        for n, p in model.encoder.named_parameters():
            if "lora_B" in n:
                p.add_(0.25)
    torch.save(model.encoder.state_dict(), path)
    saved = torch.load(path, map_location="cpu")
    assert set(saved.keys()) == peft_keys
    fresh = glitch.build_model("micro", 4, "DoRA", 8, 32, device="cpu")
    fresh.encoder.load_state_dict(saved)           # strict
    for (n, a), (_, b) in zip(model.encoder.state_dict().items(), fresh.encoder.state_dict().items()):
        assert torch.equal(a, b), n
    lora = glitch.build_model("micro", 4, "LoRA", 4, 16, device="cpu")
    assert not any("magnitude" in k for k in lora.encoder.state_dict())
    full = glitch.build_model("micro", 4, "full_finetune", device="cpu")
    assert set(full.encoder.state_dict().keys()) == set(synth.named_encoder_state_dict("micro").keys())
    assert all(p.requires_grad for p in full.parameters())
    with pytest.raises(gw_whisper_amd.GwwError, match="bf16"):
        glitch.build_model("micro", 4, "full_finetune", precision="fp32", device="cpu")
    with pytest.raises(ValueError, match="method"):
        glitch.build_model("micro", 4, "QLoRA", device="cpu")


def test_head_state_dict_has_the_layout_of_the_shipped_heads(tmp_path):
    schema = json.load(open(os.path.join(ROOT, "tests", "golden", "adapter_schema.json")))["heads"]
    for key, C in (("Glitch_classification/results/generic/multi_class_model_best_dense_weights.pth", 11),
                   ("Glitch_classification/results/high_mass/multi_class_model_best_dense_weights.pth", 6)):
        model = glitch.build_model("tiny", C, "DoRA", device="cpu")
        path = os.path.join(tmp_path, f"head{C}.pth")
        torch.save(model.classifier.state_dict(), path)
        sd = torch.load(path, map_location="cpu")
        assert {k: list(v.shape) for k, v in sd.items()} == schema[key]
        params, p = glitch._head_parameters(model.classifier)
        assert p == 0.3 and [tuple(t.shape) for t in params] == [tuple(schema[key][k]) for k in gh.PARAM_KEYS]


def test_argument_parsers_accept_the_reference_command_lines():
    train = _program("run_glitch_train").build_parser()
    a = train.parse_args("--train_data_path data/train --test_data_path data/test --log_dir logs --results_path results "
                         "--encoder tiny --batch_size 32 --num_epochs 200 --learning_rate 8e-5 --num_workers 4 "
                         "--model_name multi_class_model --method DoRA --lora_rank 8 --lora_alpha 32".split())
    assert (a.method, a.lora_rank, a.lora_alpha, a.learning_rate, a.head, a.precision) == ("DoRA", 8, 32, 8e-5, "hip", "bf16")
    d = train.parse_args(["--train_data_path", "a", "--test_data_path", "b", "--method", "LoRA"])      # the reference's defaults
    assert (d.encoder, d.batch_size, d.num_epochs, d.learning_rate, d.num_workers, d.model_name, d.lora_rank, d.lora_alpha) \
        == ("tiny", 32, 200, 8e-5, 4, "multi_class_model", 8, 32)
    assert d.log_dir == "Glitch_classification/results/generic/logs" and d.results_path == "Glitch_classification/results/generic"
    f = train.parse_args("--method full_finetune --synthetic 64 --synthetic-classes 4 --seed 1 --head torch --precision fp32 "
                         "--lora-targets layers.*.fc1 layers.*.fc2 --encoder-weights w.pth".split())
    assert (f.method, f.synthetic, f.synthetic_classes, f.head, f.lora_targets) == \
        ("full_finetune", 64, 4, "torch", ["layers.*.fc1", "layers.*.fc2"])
    with pytest.raises(SystemExit):
        train.parse_args(["--train_data_path", "a", "--test_data_path", "b"])        # --method is required, as in the reference
    ev = _program("run_glitch_evaluate").build_parser()
    e = ev.parse_args("--test_data_path data/test --results_path results --encoder tiny --batch_size 32 --num_workers 4 "
                      "--model_name multi_class_model --method LoRA --lora_weights_path r/m_best_lora_weights.pth "
                      "--dense_weights_path r/m_best_dense_weights.pth --lora_rank 8 --lora_alpha 32".split())
    assert (e.method, e.lora_weights_path, e.dense_weights_path) == ("LoRA", "r/m_best_lora_weights.pth",
                                                                     "r/m_best_dense_weights.pth")


def test_synthetic_set_is_seeded_and_balanced():
    w1, c1, s1 = synth.glitch_segments(44, 4, seed=3)
    w2, c2, s2 = synth.glitch_segments(44, 4, seed=3)
    assert w1.dtype == np.float32 and w1.shape == (44, 16000) and c1.dtype == np.int64
    assert np.array_equal(w1, w2) and np.array_equal(c1, c2) and np.array_equal(s1, s2)
    assert np.array_equal(c1, np.arange(44) % 4) and np.bincount(c1).tolist() == [11, 11, 11, 11]
    w3, _, _ = synth.glitch_segments(44, 4, seed=4)
    assert not np.array_equal(w1, w3)
    assert np.isfinite(w1).all() and 0.9 < w1.std() < 1.6       # unit-variance noise plus one short burst
    wave, raw, _ = glitch.synthetic_split(64, 4, seed=0)
    test_wave, test_raw, _ = glitch.synthetic_split(64, 4, seed=0, test=True)
    assert len(raw) == 64 and len(test_raw) == 16 and not np.array_equal(wave[:16], test_wave)
    classes = glitch.fit_classes(raw + test_raw)
    assert classes == ["Burst Band 01", "Burst Band 02", "Burst Band 03", "GW"]
    assert np.bincount(glitch.encode_labels(test_raw, classes)).tolist() == [4, 4, 4, 4]
    with pytest.raises(ValueError):
        synth.glitch_segments(8, 65)


def test_cpu_tensors_and_bad_shapes_are_refused():
    from gw_whisper_amd import ops
    model = glitch.build_model("micro", 4, "DoRA", device="cpu")
    x, y = torch.zeros(2, 128), torch.zeros(2, dtype=torch.int64)
    with pytest.raises(gw_whisper_amd.GwwError, match="GPU|CPU"):
        glitch.head_cross_entropy(model.classifier, x, y)
    params, _ = glitch._head_parameters(model.classifier)
    with pytest.raises(gw_whisper_amd.GwwError, match="GPU"):
        ops.head_forward(x, params, y)
    with pytest.raises(gw_whisper_amd.GwwError, match="GPU"):
        ops.head_dropout_mask(0, 0, 0, 2, 512, device="cpu")
    with pytest.raises(gw_whisper_amd.GwwError, match="GPU"):
        ops.eval_accumulate(torch.zeros(2, 4), y, torch.zeros(2), torch.zeros(4, 4, dtype=torch.int64),
                            torch.zeros(1, dtype=torch.float64), torch.zeros(1, dtype=torch.int64))
    with pytest.raises(gw_whisper_amd.GwwError, match="nn.Sequential"):
        glitch._head_parameters(torch.nn.Sequential(torch.nn.Linear(4, 4)))
    # the C ABI validates shapes before any HIP call
    lib = gw_whisper_amd.lib()
    assert lib.gww_head_forward_f32(None, None, None, 4, 100, 4, 0.3, 0, 0, 0, *([None] * 6)) == -1
    assert b"d_in" in lib.gww_last_error()
    assert lib.gww_head_forward_f32(None, None, None, 4, 128, 65, 0.3, 0, 0, 0, *([None] * 6)) == -1
    assert lib.gww_head_forward_f32(None, None, None, 2000, 128, 4, 0.3, 0, 0, 0, *([None] * 6)) == -1
    assert lib.gww_head_backward_f32(*([None] * 5), 4, 128, 0, 0.3, 0, None, 0, None, None, None) == -1
    assert lib.gww_eval_accumulate(None, None, None, 4, 4, None, None, None, None) == -1
    assert lib.gww_head_workspace_bytes(32, 11) == 32 * (512 + 256 + 128 + 11) * 4


def test_dataset_directories_load_like_the_reference(tmp_path):
    """The reference's columns (``data``, ``labels``, ``SNR``: dataset.py:41-43); ``chunk*`` sub-directories are concatenated
    in sorted order (train.py:26-35), a directory without chunks is read as it is (evaluate.py:81)."""
    from datasets import Dataset
    rng = np.random.default_rng(0)
    data = rng.standard_normal((7, 64)).astype(np.float32)
    labels = ["Blip", "GW", "koi_fish", "Blip", "1080Lines", "GW", "whistle"]
    snr = np.arange(7, dtype=np.float32) + 7.5
    rows = {"data": data.tolist(), "labels": labels, "SNR": snr.tolist()}
    Dataset.from_dict(rows).save_to_disk(str(tmp_path / "whole"))
    for name, lo, hi in (("chunk_1", 3, 7), ("chunk_0", 0, 3)):          # written out of order: sorted on load
        Dataset.from_dict({k: v[lo:hi] for k, v in rows.items()}).save_to_disk(str(tmp_path / "chunked" / name))
    for path, concatenated in ((tmp_path / "whole", True), (tmp_path / "whole", False), (tmp_path / "chunked", True)):
        x, raw, s = glitch.load_split(str(path), concatenated=concatenated)
        assert x.dtype == np.float32 and np.array_equal(x, data) and raw == labels and np.array_equal(s, snr)
    classes = glitch.fit_classes(raw)
    assert classes == ["1080Lines", "Blip", "GW", "Koi Fish", "Whistle"]
    assert glitch.encode_labels(raw, classes).tolist() == [1, 2, 3, 1, 0, 2, 4]
