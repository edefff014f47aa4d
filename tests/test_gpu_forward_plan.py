"""The launch plan of the inference forward, pinned through the encoder's own trace (needs an MI355X, -m gpu).

``trace_enable`` makes the forward record one span per kernel class (csrc/encoder.hip: TR(...)); ``trace_read`` returns
the span count of every class.  Which classes run, and how often, is the whole outcome of the path selection
(``plan_forward``): a drift in it changes a count here, in the suite, and not only in a profiling session.

The expected counts are those of the forward before it was split into a plan and its walks (commit ae0e61e), read off
its ``forward_impl`` and confirmed by that build's own ``trace_read`` (profiles/forward_plan.md): 2 layers, 2 segments,
3000 frames.
  d = 384, bf16 (A-stationary walk): the stem is one conv1 and one conv2 span whether the constant-tail shortcut runs or
    not (its launches are grouped under them).  Hidden wanted: LN1 + q/k/v of layer 0, attention, fused block + the next
    q/k/v, attention, fused block + final LayerNorm.  Only the last token: the last layer is the pooled one instead --
    attention, out_proj, LayerNorm on B rows, fc1, fc2, final LayerNorm on B rows.  Per-layer outputs add copies and
    the probability kernel, which carry no span.  The split at 64 segments runs two half batches: every count doubles.
  d = 512 / 768 bf16 and fp32 (generic walk): per layer LayerNorm, q/k/v, attention, out_proj, LayerNorm, fc1, fc2; the
    per-layer LayerNorms share the class of the final one.  fp32 has no direct conv1 (one mel_to_tokens span) and no
    pooled last layer.
"""

import pytest

from gw_whisper_amd import synth

pytestmark = pytest.mark.gpu

MEL, CONV1, CONV2, QKV, ATTN, OUT, FC1, FC2, LN = ("mel_to_tokens", "conv1_gelu", "conv2_gelu_pos", "ln+qkv_proj", "attention",
                                                   "out_proj", "ln+fc1_gelu", "fc2", "final_layernorm")
MLP, MLPQKV, LNROWS, MLPFIN = ("mlp_fused(ln+fc1+gelu+fc2)", "mlp_fused+next_ln_qkv", "layernorm_rows(B pooled rows)",
                               "mlp_fused+final_layernorm")

STEM = {CONV1: 1, CONV2: 1}
# d = 384, bf16, L layers
HIDDEN_384 = {**STEM, QKV: 1, ATTN: 2, MLPQKV: 1, MLPFIN: 1}
POOLED_384 = {**STEM, QKV: 1, ATTN: 2, MLPQKV: 1, OUT: 1, LNROWS: 2, FC1: 1, FC2: 1}
HIDDEN_384_L1 = {**STEM, QKV: 1, ATTN: 1, MLPFIN: 1}
POOLED_384_L1 = {**STEM, QKV: 1, ATTN: 1, OUT: 1, LNROWS: 2, FC1: 1, FC2: 1}
# the generic walk, 2 layers
LAYERS_GENERIC = {QKV: 2, ATTN: 2, OUT: 2, FC1: 2, FC2: 2}
HIDDEN_GENERIC = {**STEM, **LAYERS_GENERIC, LN: 5}
POOLED_GENERIC = {**STEM, **LAYERS_GENERIC, LN: 3, LNROWS: 2}
FP32_STEM = {MEL: 1, **STEM}

DIMS = {384: (384, 2, 6, 1536), 512: (512, 2, 8, 2048), 768: (768, 2, 12, 3072)}


def _double(counts):
    return {k: 2 * v for k, v in counts.items()}


@pytest.fixture(scope="module")
def T():
    import torch
    assert torch.cuda.is_available()
    return torch


@pytest.fixture(scope="module")
def mels(T):
    """(a padded log-mel: 1 s of strain in a 30 s window, whose constant tail the stem shortcut skips; a dense one)."""
    from gw_whisper_amd import ops
    padded = ops.logmel(T.from_numpy(synth.strain_segments(2, seed=33)).cuda())
    g = T.Generator().manual_seed(5)
    return {"padded": padded, "dense": (0.5 * T.randn((2, 80, 3000), generator=g)).cuda()}


_ENC = {}


def _encoder(dims, precision="bf16"):
    if (dims, precision) not in _ENC:
        from gw_whisper_amd.encoder import WhisperConfig, WhisperEncoder
        sd = synth.encoder_state_dict(*dims, seed=3)
        enc = WhisperEncoder.from_numpy_state_dict(sd, WhisperConfig(*dims), precision=precision).cuda()
        enc.trace_enable(True)
        enc.trace_read()
        _ENC[(dims, precision)] = enc
    enc = _ENC[(dims, precision)]
    enc.set_split(False)
    enc.set_stem_shortcut(True)
    return enc


def _counts(enc):
    return {k: n for k, (_, n) in enc.trace_read().items() if n}


def _check(T, enc, run, want, what, repeat=False):
    """The span counts of one forward; repeat: a second forward gives the same counts and the same bits (no state leaks
    from call to call)."""
    enc.trace_read()
    with T.no_grad():
        out = [t.clone() for t in run() if t is not None]
        got = _counts(enc)
        print(f"{what}: {got}")
        assert got == want, f"{what}: spans per class {got}, expected {want}"
        if repeat:
            again = [t for t in run() if t is not None]
            assert _counts(enc) == want, f"{what}: the second forward launched differently"
            for a, b in zip(out, again):
                assert T.equal(a.view(T.int32), b.view(T.int32)), f"{what}: the second forward computed differently"


@pytest.mark.parametrize("tag,flag", [("padded", 1), ("dense", 0)])
@pytest.mark.parametrize("want_h,want_l,want", [(True, False, HIDDEN_384), (False, True, POOLED_384), (True, True, HIDDEN_384)])
def test_plan_384(T, mels, tag, flag, want_h, want_l, want):
    enc = _encoder(DIMS[384])
    _check(T, enc, lambda: enc.forward_raw(mels[tag], want_hidden=want_h, want_last=want_l), want,
           f"384 {tag} hidden={want_h} last={want_l}", repeat=(tag == "padded" and want_h and want_l))
    assert enc.stem_shortcut_flags(2) == (flag, -1)


def test_plan_384_per_layer_outputs(T, mels):
    enc = _encoder(DIMS[384])

    def run():
        last, hs, at = enc.forward_outputs_raw(mels["padded"], True, True)
        return (last,) + hs + at
    _check(T, enc, run, HIDDEN_384, "384 per-layer outputs")
    assert enc.stem_shortcut_flags(2) == (1, -1)


def test_plan_384_shortcut_off(T, mels):
    enc = _encoder(DIMS[384])
    enc.set_stem_shortcut(False)
    try:
        _check(T, enc, lambda: enc.forward_raw(mels["padded"], want_hidden=True, want_last=True), HIDDEN_384, "384 shortcut off")
        assert enc.stem_shortcut_flags(2) == (-1, -1)
        _check(T, enc, lambda: enc.forward_raw(mels["padded"], want_hidden=False, want_last=True), POOLED_384,
               "384 shortcut off, last token")
    finally:
        enc.set_stem_shortcut(True)


def test_plan_384_split_at_64_segments(T, mels):
    enc = _encoder(DIMS[384])
    big = T.cat([mels["padded"].repeat(16, 1, 1), mels["dense"].repeat(16, 1, 1)])   # the second half batch is dense
    enc.set_split(True)
    try:
        _check(T, enc, lambda: enc.forward_raw(big, want_hidden=True, want_last=True), _double(HIDDEN_384), "384 split 64")
        assert enc.stem_shortcut_flags(64) == (1, 0)
        _check(T, enc, lambda: enc.forward_raw(big, want_hidden=False, want_last=True), _double(POOLED_384),
               "384 split 64, last token")
    finally:
        enc.set_split(False)


@pytest.mark.parametrize("want_h,want", [(True, HIDDEN_384_L1), (False, POOLED_384_L1)])
def test_plan_384_one_layer(T, mels, want_h, want):
    enc = _encoder((384, 1, 6, 1536))
    _check(T, enc, lambda: enc.forward_raw(mels["padded"], want_hidden=want_h, want_last=True), want, f"384 one layer hidden={want_h}")
    assert enc.stem_shortcut_flags(2) == (1, -1)


@pytest.mark.parametrize("d", [512, 768])
def test_plan_generic_widths(T, mels, d):
    enc = _encoder(DIMS[d])
    _check(T, enc, lambda: enc.forward_raw(mels["dense"], want_hidden=True, want_last=False), HIDDEN_GENERIC, f"{d} hidden",
           repeat=True)
    _check(T, enc, lambda: enc.forward_raw(mels["padded"], want_hidden=False, want_last=True), POOLED_GENERIC, f"{d} last token")


def test_plan_fp32(T, mels):
    enc = _encoder(DIMS[384], "fp32")
    _check(T, enc, lambda: enc.forward_raw(mels["padded"], want_hidden=True, want_last=True),
           {**FP32_STEM, **LAYERS_GENERIC, LN: 5, LNROWS: 1}, "fp32 hidden + last", repeat=True)
    _check(T, enc, lambda: enc.forward_raw(mels["padded"], want_hidden=False, want_last=True),
           {**FP32_STEM, **LAYERS_GENERIC, LN: 4, LNROWS: 1}, "fp32 last token")
    assert enc.stem_shortcut_flags(2) == (-1, -1)
