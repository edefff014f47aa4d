"""CPU checks of the per-layer output surface (output_hidden_states / output_attentions): the BaseModelOutput tuple
semantics HF's ModelOutput has, the config fields, and the HF golden of tools/make_golden_outputs.py."""

import json

import numpy as np
import pytest
import torch

from gw_whisper_amd.encoder import BaseModelOutput, WhisperConfig


def test_base_model_output_skips_none_fields():
    last = torch.zeros(2, 3)
    o = BaseModelOutput(last_hidden_state=last)
    assert o.hidden_states is None and o.attentions is None
    assert o.to_tuple() == (last,)
    assert o[0] is last and o["last_hidden_state"] is last
    with pytest.raises(IndexError):
        o[1]
    hs, at = (torch.ones(1), torch.ones(2)), (torch.ones(3),)
    o = BaseModelOutput(last_hidden_state=last, attentions=at)
    assert o.to_tuple() == (last, at) and o[1] is at and o[-1] is at
    o = BaseModelOutput(last_hidden_state=last, hidden_states=hs, attentions=at)
    t = o.to_tuple()
    assert len(t) == 3 and t[0] is last and t[1] is hs and t[2] is at
    assert o[1:] == (hs, at)


def test_config_output_fields(tmp_path):
    c = WhisperConfig()
    assert (c.output_hidden_states, c.output_attentions, c.return_dict) == (False, False, True)
    assert WhisperConfig.named("tiny").return_dict is True
    base = {"d_model": 384, "encoder_layers": 4, "encoder_attention_heads": 6, "encoder_ffn_dim": 1536}
    p = tmp_path / "config.json"
    p.write_text(json.dumps(base))
    c = WhisperConfig.from_json_file(str(p))
    assert (c.output_hidden_states, c.output_attentions, c.return_dict) == (False, False, True)
    p.write_text(json.dumps(dict(base, output_hidden_states=True, output_attentions=True, return_dict=False)))
    c = WhisperConfig.from_json_file(str(p))
    assert (c.output_hidden_states, c.output_attentions, c.return_dict) == (True, True, False)
    assert (c.d_model, c.encoder_layers, c.num_mel_bins) == (384, 4, 80)


def test_outputs_golden_is_consistent(golden):
    g = golden("encoder_outputs.npz")
    rows, qrows = g["rows"], g["qrows"]
    assert list(qrows) == [0, 50, 777, 1499] and rows[-1] == 1499
    for name, (d, H) in {"tiny": (384, 6), "base": (512, 8)}.items():
        cd, L, cH, F, _, _ = g[f"{name}_config"]
        assert (cd, L, cH) == (d, 2, H) and F == 4 * d
        for i in range(L + 1):
            assert g[f"{name}_hidden{i}"].shape == (2, len(rows), d)
            assert np.isfinite(g[f"{name}_hidden{i}"]).all()
        for l in range(L):
            a = g[f"{name}_attn{l}"]
            assert a.shape == (H, len(qrows), 1500) and a.dtype == np.float32
            assert (a >= 0).all()
            np.testing.assert_allclose(a.astype(np.float64).sum(-1), 1.0, atol=1e-5)
        # the residual stream changes from layer to layer; the last entry is after the final LayerNorm
        assert not np.allclose(g[f"{name}_hidden0"], g[f"{name}_hidden1"])
        last = g[f"{name}_hidden{L}"].astype(np.float64)
        assert np.abs(last.mean(-1)).max() < 1.0
