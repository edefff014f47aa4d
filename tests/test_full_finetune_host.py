"""CPU checks of the full fine-tuning surface: the save_pretrained layout (HF WhisperConfig fields, the HF encoder
state_dict keys and shapes) and the refusal to combine full fine-tuning with DoRA / LoRA adapters."""

import json

import pytest
import torch

from gw_whisper_amd import GwwError, synth
from gw_whisper_amd.encoder import WhisperConfig, WhisperEncoder
from gw_whisper_amd.peft import LoraConfig, get_peft_model


def _micro():
    d, L, H, F = synth.ENCODER_SIZES["micro"]
    sd = synth.encoder_state_dict(d, L, H, F, seed=9)
    return WhisperEncoder.from_numpy_state_dict(sd, WhisperConfig(d, L, H, F)), sd


def test_save_pretrained_layout(tmp_path):
    from safetensors.torch import load_file
    enc, sd = _micro()
    enc.save_pretrained(str(tmp_path / "enc"))
    cfg = json.load(open(tmp_path / "enc" / "config.json"))
    c = enc.config
    for k in ("d_model", "encoder_layers", "encoder_attention_heads", "encoder_ffn_dim", "num_mel_bins",
              "max_source_positions"):
        assert cfg[k] == getattr(c, k), k
    assert cfg["model_type"] == "whisper"
    saved = load_file(str(tmp_path / "enc" / "model.safetensors"))
    assert set(saved) == set(sd) == set(enc.state_dict())
    for k, v in sd.items():
        assert tuple(saved[k].shape) == v.shape and saved[k].dtype == torch.float32, k
        assert torch.equal(saved[k], torch.from_numpy(v)), k
    # reloads into a fresh encoder (the harness's --encoder-weights path)
    d, L, H, F = synth.ENCODER_SIZES["micro"]
    WhisperEncoder(WhisperConfig(d, L, H, F)).load_state_dict(saved)


def test_enable_full_finetune_returns_self_and_keeps_the_base_frozen():
    enc, _ = _micro()
    assert enc.enable_full_finetune() is enc and enc.full_finetune
    assert not any(p.requires_grad for p in enc.parameters())   # the opt-in does not un-freeze anything by itself


def test_full_finetune_refuses_adapters():
    enc, _ = _micro()
    get_peft_model(enc, LoraConfig(use_dora=True, r=8, lora_alpha=32, target_modules=["layers.0.self_attn.q_proj"]))
    with pytest.raises(GwwError, match="adapters"):
        enc.enable_full_finetune()
    with pytest.raises(GwwError, match="adapter"):
        enc.save_pretrained("unused")


def test_full_finetune_needs_bf16():
    d, L, H, F = synth.ENCODER_SIZES["micro"]
    with pytest.raises(GwwError, match="bf16"):
        WhisperEncoder(WhisperConfig(d, L, H, F), precision="fp32").enable_full_finetune()
