"""Layer 0 on the compact stem's output: its LN1 + q / k / v launch and its block form the residual stream in registers
(csrc/mlp_fused.hip, k_mlp_fused<., ., true>) instead of reading one that k_stem_fill wrote (needs an MI355X, -m gpu).

Every comparison is exact: ``torch.equal`` on int32 views, so that -0 / +0 and NaN payloads count.  The reference of the
kernel-level tests is the chain the encoder ran before: ``ops.stem_fill`` into x, then ``ops.lnqkv_fused`` and
``ops.attn_out_mlp_fused`` (with the q / k / v tail) on that x.
"""

import numpy as np
import pytest

from gw_whisper_amd import synth
from tests.guard import Guard, run_contract

pytestmark = pytest.mark.gpu

D, F, NQ = 384, 1536, 1152
SPLIT_MIN = 32      # csrc/encoder.hip: kSplitMin


@pytest.fixture(scope="module")
def T():
    import torch
    assert torch.cuda.is_available()
    return torch


def _bits(T, t):
    t = t.contiguous()
    return t.view(T.int16) if t.dtype == T.bfloat16 else t.view(T.int32)


def _bits_equal(T, a, b):
    return a.shape == b.shape and a.dtype == b.dtype and T.equal(_bits(T, a), _bits(T, b))


def _stem(T, B, Tn, Tt, seed):
    """Seeded xs [B, Tt, 384], tr [B, 384] (a sigmoid factor: in (0, 1)), pos [Tn, 384] on the device."""
    rng = np.random.default_rng(seed)
    xs = rng.standard_normal((B, Tt, D)).astype(np.float32)
    tr = (1.0 / (1.0 + np.exp(-rng.standard_normal((B, D))))).astype(np.float32)
    pos = (rng.standard_normal((Tn, D)) * 0.5).astype(np.float32)
    return tuple(T.from_numpy(a).cuda() for a in (xs, tr, pos))


_W = {}


def _weights(T, M):
    """Block operands for M rows (ctx and every weight; its x is not used), folded once per M."""
    if M not in _W:
        from gw_whisper_amd import ops
        from tests.test_gpu_memory_contract import _block
        _, d = _block(T, M, 4000 + M)
        w1f, u, cb = ops.ln_fold_weights(d["w1"], d["lw"], d["lb"], d["b1"])
        wqf, uq, cq = ops.ln_fold_weights(d["wq"], d["lw1"], d["lb1"], d["bq"])
        d.update(w1f=w1f, u=u, cb=cb, wqf=wqf, uq=uq, cq=cq, wtq=ops.mlp_pack(None, None, wqf))
        _W[M] = d
    return _W[M]


def _reference(T, x, w):
    """(q / k / v of layer 0, q / k / v of the next layer, x_next) by the existing ops on a dense x."""
    from gw_whisper_amd import ops
    q0 = ops.lnqkv_fused(x, w["wtq"], w["uq"], w["cq"])
    q1, xn = ops.attn_out_mlp_fused(x, w["ctx"], w["wo"], w["bo"], w["w1f"], w["w2"], w["u"], w["cb"], w["b2"],
                                    qkv=(w["wqf"], w["uq"], w["cq"]))
    return q0, q1, xn


def _candidate(T, xs, tr, pos, flag, x, w):
    from gw_whisper_amd import ops
    q0 = ops.lnqkv_fused_x0(xs, tr, pos, flag, w["wtq"], w["uq"], w["cq"], x=x)
    q1, xn = ops.attn_out_mlp_fused_x0(xs, tr, pos, flag, w["ctx"], w["wo"], w["bo"], w["w1f"], w["w2"], w["u"], w["cb"],
                                       w["b2"], (w["wqf"], w["uq"], w["cq"]), x=x)
    return q0, q1, xn


def _assert_same(T, got, want, what):
    for name, a, b in zip(("layer-0 qkv", "next-layer qkv", "x_next"), got, want):
        assert _bits_equal(T, a, b), f"{what}: {name} differs from the reference chain"


def _flag(T, v):
    return T.full((1,), v, dtype=T.int32, device="cuda")


# B = 3, T = 200: M = 600 = 4 panels + 88 rows (ragged last panel); panel 1 (rows 128 .. 255) holds segment 0's tail, its last
# token 199 and segment 1's head; panel 0 holds the head / tail boundary at token 126.  B = 1: one segment, ragged.
# B = 2, T = 192: M = 384 = 3 whole panels.  B = 2, T = 256, Tt = 100: another compact length, panels = segments.
SHAPES = [(3, 200, 128), (1, 200, 128), (2, 192, 128), (2, 256, 100)]


@pytest.mark.parametrize("B,Tn,Tt", SHAPES)
def test_kernels_form_the_stream(T, B, Tn, Tt):
    from gw_whisper_amd import ops
    xs, tr, pos = _stem(T, B, Tn, Tt, seed=B * 1000 + Tn)
    w = _weights(T, B * Tn)
    one = _flag(T, 1)
    x = ops.stem_fill(xs, tr, pos, one)
    x3 = x.view(B, Tn, D)
    assert T.equal(x3[:, :Tt - 2], xs[:, :Tt - 2]) and T.equal(x3[:, Tn - 1], xs[:, Tt - 1])
    want = _reference(T, x, w)
    poison = T.full_like(x, float("nan"))          # flag 1: x is not read
    got = _candidate(T, xs, tr, pos, one, poison, w)
    _assert_same(T, got, want, f"B = {B}, T = {Tn}, Tt = {Tt}")
    assert bool(T.isfinite(got[2]).all()) and bool(T.isfinite(got[0].float()).all())


@pytest.mark.parametrize("B,Tn,Tt", SHAPES[:3])
def test_flag_cleared_reads_x(T, B, Tn, Tt):
    """Flag 0 (the forward took the full stem): the new ops are the existing ones on the dense x; xs / tr hold NaN."""
    xs, tr, pos = _stem(T, B, Tn, Tt, seed=77)
    xs.fill_(float("nan"))
    tr.fill_(float("nan"))
    w = _weights(T, B * Tn)
    x = T.from_numpy(np.random.default_rng(5).standard_normal((B * Tn, D)).astype(np.float32)).cuda()
    want = _reference(T, x, w)
    got = _candidate(T, xs, tr, pos, _flag(T, 0), x, w)
    _assert_same(T, got, want, f"flag 0, B = {B}, T = {Tn}")
    assert bool(T.isfinite(got[2]).all())


def test_bit_patterns(T):
    """-0.0 and NaN payloads (quiet and signalling) in head rows of xs are taken bitwise, -0.0 in tr goes through the fma."""
    from gw_whisper_amd import ops
    B, Tn, Tt = 3, 200, 128
    xs, tr, pos = _stem(T, B, Tn, Tt, seed=91)
    xs[0, 5, 7] = -0.0
    xs[2, Tt - 1, 100] = -0.0                                     # the row of token T - 1
    xs.view(T.int32)[1, 20, 9] = 0x7FC12345                       # quiet NaN with a payload
    xs.view(T.int32)[1, 21, 300] = 0x7F812345                      # signalling NaN with a payload
    tr[1, 33] = -0.0
    assert bool(T.signbit(xs[0, 5, 7])) and bool(T.signbit(tr[1, 33]))
    w = _weights(T, B * Tn)
    one = _flag(T, 1)
    x = ops.stem_fill(xs, tr, pos, one)
    xi = x.view(T.int32).view(B, Tn, D)
    assert int(xi[1, 20, 9]) == 0x7FC12345 and int(xi[1, 21, 300]) == 0x7F812345 and bool(T.signbit(x.view(B, Tn, D)[0, 5, 7]))
    want = _reference(T, x, w)
    got = _candidate(T, xs, tr, pos, one, T.full_like(x, float("nan")), w)
    _assert_same(T, got, want, "bit patterns")
    rows = T.ones(B * Tn, dtype=T.bool, device="cuda")
    rows[[Tn + 20, Tn + 21]] = False                              # the two NaN rows
    assert bool(T.isfinite(got[2][rows]).all()) and bool(T.isnan(got[2][~rows]).all())


# ------------------------------------------------------------------ encoder level
_ENC = {}


def _encoder():
    if "tiny" not in _ENC:
        from gw_whisper_amd.encoder import WhisperConfig, WhisperEncoder
        sd = synth.named_encoder_state_dict("tiny", seed=11)
        _ENC["tiny"] = WhisperEncoder.from_numpy_state_dict(sd, WhisperConfig.named("tiny"), precision="bf16").cuda()
    enc = _ENC["tiny"]
    enc.set_split(False)
    enc.set_stem_shortcut(True)
    return enc


def _logmel(T, batch, seed=1000):
    from gw_whisper_amd import ops
    return ops.logmel(T.from_numpy(synth.strain_segments(batch, seed=seed, n_samples=16000)).cuda())


def _three(enc, mel):
    h = enc.forward_raw(mel, want_hidden=True, want_last=False)[0].clone()
    l = enc.forward_raw(mel, want_hidden=False, want_last=True)[1].clone()
    bh, bl = enc.forward_raw(mel, want_hidden=True, want_last=True)
    return {"hidden": h, "last": l, "both.hidden": bh.clone(), "both.last": bl.clone()}


def test_encoder_shortcut_on_off(T):
    """whisper-tiny, B = 3, log-mel of 1 s strain: the three output combinations with the shortcut on (layer 0 forms x itself,
    no fill) against off (full stem), then the kept fill path (per-layer hidden states) and attention maps."""
    enc = _encoder()
    mel = _logmel(T, 3)
    on = _three(enc, mel)
    assert enc.stem_shortcut_flags(3) == (1, -1)
    _, hs_on, _ = enc.forward_outputs_raw(mel, True, False)
    hs_on = [hs_on[0].clone(), hs_on[1].clone(), hs_on[-1].clone()]
    _, _, at_on = enc.forward_outputs_raw(mel, False, True)         # attention maps alone: still without the fill
    at_on = [at_on[0].clone(), at_on[-1].clone()]
    enc.set_stem_shortcut(False)
    off = _three(enc, mel)
    assert enc.stem_shortcut_flags(3) == (-1, -1)
    _, hs_off, _ = enc.forward_outputs_raw(mel, True, False)
    _, _, at_off = enc.forward_outputs_raw(mel, False, True)
    enc.set_stem_shortcut(True)
    for k in on:
        assert _bits_equal(T, on[k], off[k]), f"{k}: shortcut on and off differ"
    # (the pooled forward -- last token alone -- runs its last layer on B rows by other kernels: no bitwise relation to row T - 1)
    assert _bits_equal(T, on["hidden"], on["both.hidden"]) and _bits_equal(T, on["both.last"], on["hidden"][:, -1])
    for a, b, name in zip(hs_on, (hs_off[0], hs_off[1], hs_off[-1]), ("hidden_states[0]", "hidden_states[1]", "hidden_states[-1]")):
        assert _bits_equal(T, a, b), f"{name}: shortcut on and off differ"
    assert _bits_equal(T, hs_on[-1], on["hidden"]), "the fill path and the register path give other last hidden states"
    for a, b in zip(at_on, (at_off[0], at_off[-1])):
        assert _bits_equal(T, a, b), "attention maps: shortcut on and off differ"
    assert bool(T.isfinite(on["hidden"]).all())


def test_encoder_fallback_dense(T):
    """Dense features: the device flag reads 0 and the same two launches read the x the full conv2 wrote."""
    enc = _encoder()
    rng = np.random.default_rng(7)
    mel = T.from_numpy(np.clip(rng.standard_normal((3, 80, 3000)) * 0.5, -1.5, 1.5).astype(np.float32)).cuda()
    on = _three(enc, mel)
    assert enc.stem_shortcut_flags(3) == (0, -1)
    enc.set_stem_shortcut(False)
    off = _three(enc, mel)
    enc.set_stem_shortcut(True)
    for k in on:
        assert _bits_equal(T, on[k], off[k]), f"{k}: shortcut on and off differ on dense features"


def test_encoder_split(T):
    """Split mode (two half batches, one flag each): both halves on the register path, and a batch whose second half alone
    is dense takes it in the first half only."""
    enc = _encoder()
    B = 2 * SPLIT_MIN + 3
    mel = _logmel(T, B)
    plain = enc.forward_raw(mel)[0].clone()
    enc.set_split(True)
    for m, flags in ((mel, (1, 1)), (None, (1, 0))):
        if m is None:
            m = mel.clone()
            m[B - 1, 17, 1500] += 0.25
        enc.set_stem_shortcut(True)
        on = _three(enc, m)
        assert enc.stem_shortcut_flags(B) == flags
        enc.set_stem_shortcut(False)
        off = _three(enc, m)
        enc.set_stem_shortcut(True)
        for k in on:
            assert _bits_equal(T, on[k], off[k]), f"{k}: split, flags {flags}: shortcut on and off differ"
        if flags == (1, 1):
            assert _bits_equal(T, on["hidden"], plain), "split and unsplit forwards differ"
    enc.set_split(False)


# ------------------------------------------------------------------ memory contract
def _stream(T):
    return T.cuda.current_stream().cuda_stream


def _ok(rc, what):
    from gw_whisper_amd._lib import check
    check(rc, what)


@pytest.mark.parametrize("B,Tn,Tt", [(3, 200, 128), (2, 192, 128)])
def test_memory_contract(T, B, Tn, Tt):
    """The three entry points on guarded, exact-size operands.  gww_stem_fill_f32 writes all of x and nothing else; the x0
    q / k / v launch writes qkv (rows padded to 128) and leaves x alone; the x0 block writes qkv and x_next (= x) and nothing
    else.  x is allocated from the guard's fill (NaN, 3.39e38, 0 in turn) and the results must not depend on it."""
    from gw_whisper_amd import ops
    from gw_whisper_amd._lib import lib
    from tests.test_gpu_memory_contract import _folded
    M, Mp = B * Tn, (B * Tn + 127) // 128 * 128
    xs, tr, pos = _stem(T, B, Tn, Tt, seed=31)
    d = _weights(T, M)
    one = _flag(T, 1)

    def case(g):
        w1f, u, cb, wqf, uq, cq = _folded(T, ops, g, d)
        wtq = ops.mlp_pack(None, None, wqf)
        pwo, pw2 = g.place(d["wo"]), g.place(d["w2"])
        wt = g.empty((D * D + 2 * D * F + NQ * D,), T.bfloat16)
        _ok(lib().gww_mlp_pack_op_bf16(pwo.data_ptr(), w1f.data_ptr(), pw2.data_ptr(), wqf.data_ptr(), wt.data_ptr(), D, F, NQ,
                                       _stream(T)), "gww_mlp_pack_op_bf16")
        pxs, ptr, ppos, pflag = g.place(xs), g.place(tr), g.place(pos), g.place(one)
        pctx, pbo, pb2 = g.place(d["ctx"]), g.place(d["bo"]), g.place(d["b2"])
        x_fill = g.empty((M, D), T.float32)
        _ok(lib().gww_stem_fill_f32(pxs.data_ptr(), ptr.data_ptr(), ppos.data_ptr(), pflag.data_ptr(), x_fill.data_ptr(), B, Tn, Tt,
                                    D, _stream(T)), "gww_stem_fill_f32")
        x = g.empty((M, D), T.float32)              # holds the guard's fill: unread where the flag is 1
        q0 = g.empty((Mp, NQ), T.bfloat16)
        _ok(lib().gww_lnqkv_fused_x0_bf16(pxs.data_ptr(), ptr.data_ptr(), ppos.data_ptr(), pflag.data_ptr(), x.data_ptr(), Tn, Tt,
                                          uq.data_ptr(), cq.data_ptr(), wtq.data_ptr(), q0.data_ptr(), M, D, NQ, _stream(T)),
            "gww_lnqkv_fused_x0_bf16")
        if isinstance(g, Guard):
            assert g.unwritten(x) == x.numel(), "the q / k / v launch wrote to x"
        q1 = g.empty((Mp, NQ), T.bfloat16)
        _ok(lib().gww_attn_out_mlp_fused_x0_bf16(pxs.data_ptr(), ptr.data_ptr(), ppos.data_ptr(), pflag.data_ptr(), x.data_ptr(), Tn,
                                                 Tt, pctx.data_ptr(), pbo.data_ptr(), u.data_ptr(), cb.data_ptr(), wt.data_ptr(),
                                                 pb2.data_ptr(), M, D, F, uq.data_ptr(), cq.data_ptr(), q1.data_ptr(), NQ,
                                                 _stream(T)), "gww_attn_out_mlp_fused_x0_bf16")
        for name, a, b in (("xs", pxs, xs), ("tr", ptr, tr), ("pos", ppos, pos), ("ctx", pctx, d["ctx"])):
            assert _bits_equal(T, a, b), f"{name} is only read"
        return {"x_fill": x_fill, "q0": q0[:M], "q1": q1[:M], "x_next": x}
    r = run_contract(case, arena_row_bytes=2 * 1536)
    want = _reference(T, r["x_fill"], d)
    _assert_same(T, (r["q0"], r["q1"], r["x_next"]), want, "under the guard")
