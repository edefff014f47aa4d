"""The residual stream in accumulator order between the fused blocks (csrc/common.h x_native_offset, k_mlp_fused<., ., ., XL>,
FwdPlan::x_native) against row order (needs an MI355X, -m gpu).

Every comparison is between the switch on and off in the same process (``set_x_native``) and is exact: ``torch.equal`` on
the int32 view of the fp32 outputs.  The order only changes where a block leaves x_next for the next block in the
workspace; ``last_hidden_state`` and ``last_token`` stay in rows, so they must not change by a bit.

Which launches a case runs, d = 384, L layers (the constant tail of a padded log-mel makes layer 0 form x in registers,
an instantiation that keeps rows on both sides; dense features take the plain layer-0 block):
    log-mel, L = 4 : rows -> rows (X0), rows -> order, order -> order, order -> last_hidden
    dense,   L = 4 : rows -> order, order -> order, order -> order, order -> last_hidden
    dense,   L = 2 : rows -> order, order -> last_hidden          (no order -> order block)
    log-mel, L = 2 : rows -> rows (X0), rows -> last_hidden       (the plan has nothing to switch; still equal)
B = 1: M = 1500 rows = 11 panels + 92 live rows in the last one.  B = 3: 4500 rows, panels straddle segments, 20 live rows
in the last one.
"""

import numpy as np
import pytest

from gw_whisper_amd import synth
from tests.guard import encoder_arena_row_bytes, run_contract

pytestmark = pytest.mark.gpu

SPLIT_MIN = 32      # csrc/encoder.hip: kSplitMin


@pytest.fixture(scope="module")
def T():
    import torch
    assert torch.cuda.is_available()
    return torch


def _bits_equal(T, a, b):
    return a.shape == b.shape and a.dtype == b.dtype and T.equal(a.contiguous().view(T.int32), b.contiguous().view(T.int32))


_ENC, _MEL, _REF = {}, {}, {}


def _encoder(layers):
    if layers not in _ENC:
        from gw_whisper_amd.encoder import WhisperConfig, WhisperEncoder
        sd = synth.encoder_state_dict(384, layers, 6, 1536, seed=40 + layers)
        _ENC[layers] = WhisperEncoder.from_numpy_state_dict(sd, WhisperConfig(384, layers, 6, 1536), precision="bf16").cuda()
    enc = _ENC[layers]
    enc.set_split(False)
    enc.set_stem_shortcut(True)
    enc.set_x_native(True)
    return enc


def _features(T, kind, B):
    """'logmel': 1 s of strain zero-padded to 30 s (constant tail); 'dense': random features, no constant tail."""
    if (kind, B) not in _MEL:
        if kind == "logmel":
            from gw_whisper_amd import ops
            m = ops.logmel(T.from_numpy(synth.strain_segments(B, seed=1000 + B, n_samples=16000)).cuda())
        else:
            rng = np.random.default_rng(7 + B)
            m = T.from_numpy(np.clip(rng.standard_normal((B, 80, 3000)) * 0.5, -1.5, 1.5).astype(np.float32)).cuda()
        _MEL[(kind, B)] = m
    return _MEL[(kind, B)]


def _both(enc, mel):
    h, l = enc.forward_raw(mel, want_hidden=True, want_last=True)
    return h.clone(), l.clone()


def _reference(T, layers, kind, B):
    """(last_hidden, last_token) with the switch off, once per case."""
    key = (layers, kind, B)
    if key not in _REF:
        enc = _encoder(layers)
        enc.set_x_native(False)
        _REF[key] = _both(enc, _features(T, kind, B))
        enc.set_x_native(True)
        assert bool(T.isfinite(_REF[key][0]).all())
    return _REF[key]


@pytest.mark.parametrize("layers", [4, 2])
@pytest.mark.parametrize("kind", ["logmel", "dense"])
@pytest.mark.parametrize("B", [1, 3])
def test_on_equals_off(T, B, kind, layers):
    want_h, want_l = _reference(T, layers, kind, B)
    enc = _encoder(layers)
    mel = _features(T, kind, B)
    h, l = _both(enc, mel)
    assert enc.stem_shortcut_flags(B) == ((1, -1) if kind == "logmel" else (0, -1))
    assert _bits_equal(T, h, want_h), "last_hidden_state differs between accumulator order and row order"
    assert _bits_equal(T, l, want_l), "last_token differs between accumulator order and row order"
    assert _bits_equal(T, l, h[:, -1]), "last_token is not row T - 1 of last_hidden_state"
    # last_hidden alone: the same launches without the pooled row's stores
    h1 = enc.forward_raw(mel, want_hidden=True, want_last=False)[0]
    assert _bits_equal(T, h1, want_h)


@pytest.mark.parametrize("kind", ["logmel", "dense"])
def test_second_forward_on_the_same_workspace(T, kind):
    """on, on, off, on in one workspace: no forward reads what an earlier one left in the other order."""
    B = 3
    want_h, want_l = _reference(T, 4, kind, B)
    enc = _encoder(4)
    mel = _features(T, kind, B)
    ws = None
    for on in (True, True, False, True):
        enc.set_x_native(on)
        h, l = _both(enc, mel)
        assert ws is None or enc._ws.data_ptr() == ws, "the workspace was re-allocated between the forwards"
        ws = enc._ws.data_ptr()
        assert _bits_equal(T, h, want_h) and _bits_equal(T, l, want_l), f"forward with x_native = {on} differs"
    enc.set_x_native(True)


def test_hidden_slab_falls_back(T):
    """Per-layer hidden states are read from x in rows: the plan keeps row order for such a call."""
    B = 3
    enc = _encoder(4)
    mel = _features(T, "dense", B)
    want_h, _ = _reference(T, 4, "dense", B)
    last_on, hs_on, _ = enc.forward_outputs_raw(mel, True, False)
    last_on, hs_on = last_on.clone(), [t.clone() for t in hs_on]
    enc.set_x_native(False)
    last_off, hs_off, _ = enc.forward_outputs_raw(mel, True, False)
    enc.set_x_native(True)
    assert _bits_equal(T, last_on, last_off) and _bits_equal(T, last_on, want_h)
    for i, (a, b) in enumerate(zip(hs_on, hs_off)):
        assert _bits_equal(T, a, b), f"hidden_states[{i}] differs"
    # attention maps alone do not read x: that call runs in accumulator order
    last_at, _, at = enc.forward_outputs_raw(mel, False, True)
    assert _bits_equal(T, last_at, want_h) and bool(T.isfinite(at[-1]).all())


@pytest.mark.parametrize("B", [4, 2 * SPLIT_MIN + 3])
def test_split(T, B):
    """Split mode: at B = 4 the batch is below the split threshold and runs whole; at 67 two half batches of 33 and 34
    segments run in workspaces of their own (each half's stream starts a panel)."""
    enc = _encoder(4)
    mel = _features(T, "logmel", B)
    enc.set_x_native(False)
    want_h, want_l = _both(enc, mel)
    enc.set_x_native(True)
    enc.set_split(True)
    h, l = _both(enc, mel)
    enc.set_x_native(False)
    h_off, l_off = _both(enc, mel)
    enc.set_x_native(True)
    enc.set_split(False)
    assert _bits_equal(T, h, want_h) and _bits_equal(T, l, want_l), "split, accumulator order: differs from the plain forward"
    assert _bits_equal(T, h_off, want_h) and _bits_equal(T, l_off, want_l)


def test_memory_contract(T):
    """Under guard bands, the workspace re-allocated under the guard and filled with NaN, 3.39e38 and 0 in turn: nothing is
    written outside the workspace (whose x spans the whole panels the order needs) and the outputs do not depend on the
    fill -- no slot of a row past M, and no row-order byte of an earlier forward, is read."""
    from gw_whisper_amd._lib import PREC_BF16, lib
    B = 3
    enc = _encoder(4)
    mel = _features(T, "dense", B)
    want_h, want_l = _reference(T, 4, "dense", B)

    def case(g):
        enc._ws = None
        pm = g.place(mel)
        h, l = enc.forward_raw(pm, want_hidden=True, want_last=True)
        assert g.owns(enc._ws), "the encoder's workspace did not come from the guard"
        assert enc._ws.numel() == lib().gww_encoder_workspace_bytes(enc._handle, B, PREC_BF16)
        return {"hidden": h, "last": l}
    r = run_contract(case, arena_row_bytes=encoder_arena_row_bytes(384, 1536))
    enc._ws = None
    assert _bits_equal(T, r["hidden"], want_h) and _bits_equal(T, r["last"], want_l)
