"""Host side of adapters on every linear layer: peft's "all-linear" target string, the target list the training
backward receives (fc1 / fc2 proj ids), the harness's --lora-targets default.  No GPU needed."""

import json
import os
import sys

from gw_whisper_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _micro():
    from gw_whisper_amd.encoder import WhisperConfig, WhisperEncoder
    d, L, H, F = synth.ENCODER_SIZES["micro"]
    sd = synth.encoder_state_dict(d, L, H, F, seed=1)
    return WhisperEncoder.from_numpy_state_dict(sd, WhisperConfig(d, L, H, F), precision="bf16"), L


def test_all_linear_wraps_every_projection_and_saves_the_names(tmp_path):
    from gw_whisper_amd.peft import DoraLinear, LoraConfig, PeftModel, get_peft_model
    enc, L = _micro()
    peft = get_peft_model(enc, LoraConfig(use_dora=True, r=4, lora_alpha=8, target_modules="all-linear"))
    wrapped = [n for n, m in peft.base_model.model.named_modules() if isinstance(m, DoraLinear)]
    assert len(wrapped) == 6 * L
    names = ["q_proj", "k_proj", "v_proj", "out_proj", "fc1", "fc2"]
    assert sorted(n.rsplit(".", 1)[-1] for n in wrapped) == sorted(names * L)
    peft.save_pretrained(str(tmp_path))
    cfg = json.load(open(tmp_path / "adapter_config.json"))
    assert sorted(cfg["target_modules"]) == sorted(names)
    enc2, _ = _micro()
    back = PeftModel.from_pretrained(enc2, str(tmp_path))
    assert sum(isinstance(m, DoraLinear) for m in back.base_model.model.modules()) == 6 * L


def test_dora_targets_include_fc1_and_fc2():
    from gw_whisper_amd.encoder import WhisperEncoder  # noqa: F401
    from gw_whisper_amd.peft import LoraConfig, get_peft_model
    from gw_whisper_amd.training import dora_targets
    enc, L = _micro()
    peft = get_peft_model(enc, LoraConfig(use_dora=False, r=16, lora_alpha=32, target_modules=["fc1", "fc2", "v_proj"]))
    for n, p in peft.named_parameters():
        p.requires_grad = "lora" in n
    got = [(li, pid) for li, pid, _ in dora_targets(peft.base_model.model)]
    assert got == [(li, pid) for li in range(L) for pid in (2, 4, 5)]
    assert peft.base_model.model._has_trainable_adapters()


def test_mlp_only_adapters_are_trainable():
    from gw_whisper_amd.peft import LoraConfig, get_peft_model
    enc, _ = _micro()
    peft = get_peft_model(enc, LoraConfig(use_dora=True, r=8, lora_alpha=32, target_modules=["fc1", "fc2"]))
    for n, p in peft.named_parameters():
        p.requires_grad = "lora" in n
    assert peft.base_model.model._has_trainable_adapters()


def test_lora_targets_default_is_the_reference_list():
    """--lora-targets defaults to the list the harness adapted before the flag existed, so default runs are unchanged."""
    import subprocess
    sys.path.insert(0, os.path.join(ROOT, "harness"))
    import run_train
    assert list(run_train.DEFAULT_LORA_TARGETS) == ["layers.*.self_attn.q_proj", "layers.*.self_attn.k_proj",
                                                    "layers.*.self_attn.v_proj", "layers.*.self_attn.o_proj"]
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", CUDA_VISIBLE_DEVICES="")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "harness", "run_train.py"), "--help"], capture_output=True,
                       text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stderr
    assert "--lora-targets" in r.stdout
