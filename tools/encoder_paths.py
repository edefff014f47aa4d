"""Every branch of the encoder's host drivers (csrc/encoder.hip, encoder_train.hip, encoder_train_f32.hip), once, with
seeded inputs, through the public Python surface; every output goes into one .npz.  Made for A/B runs of two builds of
the library: GWW_LIB selects the build (gw_whisper_amd/_lib.py), e.g. under ``rocprofv3 --kernel-trace`` to compare the
launch sequences, and ``--compare a.npz b.npz`` compares two results.

Cases: bf16 inference on whisper-tiny (hidden, last token, both; per-layer outputs; the split at 64 segments; a padded
log-mel that takes the stem shortcut and a dense one that does not), at d = 512 / 768 (the generic pooled last layer),
with 128 mels, in fp32; the bf16 training step on tiny dims pooled and unpooled (rank-8 q/k/v DoRA, rank-8 out_proj,
all-linear rank 4, plain LoRA, full fine-tuning with d_mel), at d = 512 / 768 / 128; the fp32 step pooled and unpooled
(all-linear, d_mel); what only the C entries can ask for, through ctypes (d_x0 alone and with d_mel, base gradients together
with all-linear rank-4 targets through gww_encoder_train_backward_full, d_x0 of the fp32 entry); and every gww_*_bytes query of the named sizes at 1 / 32 / 64 / 256 segments.

Arrays above 4 M elements are stored as their SHA-256 and their first 4096 values.  The gradients that are
summed with float atomics are listed under ``atomic``: every adapter gradient of the d = 128 step (k_dora_grads adds dA,
dB and dm atomically) and the magnitude gradients of the rank-8 bf16 steps at d = 384 / 512 / 768 (k_dora_reduce adds
five partial sums into every dm element; dA and dB have one adder per element and are exact).  --compare holds those to
1e-4 of their largest entry, max|a - b| <= 1e-4 max|a|, the form and bound of ATOMIC_MODES in
tests/test_gpu_memory_contract.py, and everything else to bit equality."""

import argparse
import ctypes as C
import hashlib
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

QKV = ["self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj"]
ATOMIC_BOUND = 1e-4   # tests/test_gpu_memory_contract.py: ATOMIC_MODES


class Recorder:
    def __init__(self):
        self.out, self.atomic = {}, []

    def put(self, name, t, atomic=False):
        a = t.detach().float().cpu().numpy() if hasattr(t, "detach") else np.asarray(t)
        if a.size > (4 << 20):
            self.out[name + "#sha256"] = np.frombuffer(hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest(), np.uint8)
            a = a.reshape(-1)[:4096].copy()
        self.out[name] = a
        if atomic:
            self.atomic.append(name)


def encoder(dims, precision="bf16", n_mels=80, seed=3):
    from gw_whisper_amd import synth
    from gw_whisper_amd.encoder import WhisperConfig, WhisperEncoder
    sd = synth.encoder_state_dict(*dims, seed=seed, n_mels=n_mels)
    return WhisperEncoder.from_numpy_state_dict(sd, WhisperConfig(*dims, num_mel_bins=n_mels), precision=precision), sd


def mels(torch, batch, n_mels=80):
    """(a padded log-mel: 1 s of strain in a 30 s window, whose constant tail the stem shortcut skips; a dense one)."""
    from gw_whisper_amd import ops, synth
    padded = ops.logmel(torch.from_numpy(synth.strain_segments(batch, seed=33)).cuda())
    g = torch.Generator().manual_seed(5)
    dense = (0.5 * torch.randn((batch, n_mels, 3000), generator=g)).cuda()
    return padded, dense


def inference(torch, rec, trace=False):
    """trace: also record the encoder's own span count per kernel class (trace_read) of every forward, under <key>/trace."""
    def enc_for(dims, **kw):
        enc = encoder(dims, **kw)[0].cuda()
        enc.trace_enable(trace)
        return enc

    def run(enc, key, fn):
        out = fn()
        if trace:
            rec.put(key + "/trace", np.asarray([n for _, n in enc.trace_read().values()], dtype=np.int64))
        return out

    enc = enc_for((384, 4, 6, 1536))
    padded, dense = mels(torch, 2)
    with torch.no_grad():
        for tag, mel in (("padded", padded), ("dense", dense)):
            for want_h, want_l in ((True, False), (False, True), (True, True)):
                key = f"inf/tiny/{tag}/{'h' if want_h else ''}{'l' if want_l else ''}"
                h, l = run(enc, key, lambda: enc.forward_raw(mel, want_hidden=want_h, want_last=want_l))
                torch.cuda.synchronize()
                rec.put(key + "/shortcut", np.asarray(enc.stem_shortcut_flags(2)))
                if want_h:
                    rec.put(key + "/hidden", h)
                if want_l:
                    rec.put(key + "/last", l)
        o = run(enc, "inf/tiny/outputs", lambda: enc(padded[:1], output_hidden_states=True, output_attentions=True))
        rec.put("inf/tiny/outputs/last", o.last_hidden_state)
        for i, t in enumerate(o.hidden_states):
            rec.put(f"inf/tiny/outputs/hidden{i}", t)
        for i, t in enumerate(o.attentions):
            rec.put(f"inf/tiny/outputs/attn{i}", t)
        del o
        # the dual-stream split: 64 segments, half of them dense
        big = torch.cat([mels(torch, 32)[0], dense.repeat(16, 1, 1)])
        enc.set_split(True)
        h, l = run(enc, "inf/tiny/split64", lambda: enc.forward_raw(big, want_hidden=True, want_last=True))
        rec.put("inf/tiny/split64/hidden", h)
        rec.put("inf/tiny/split64/last", l)
        rec.put("inf/tiny/split64/last_only", run(enc, "inf/tiny/split64/last_only",
                                                  lambda: enc.forward_raw(big, want_hidden=False, want_last=True))[1])
        enc.set_split(False)
        del enc, big, h, l
        for dims in ((512, 2, 8, 2048), (768, 2, 12, 3072)):
            enc = enc_for(dims)
            key = f"inf/d{dims[0]}"
            rec.put(key + "/last_only", run(enc, key + "/last_only", lambda: enc.forward_raw(padded, want_hidden=False, want_last=True))[1])
            rec.put(key + "/hidden", run(enc, key + "/hidden", lambda: enc.forward_raw(dense, want_hidden=True, want_last=True))[0])
        enc = enc_for((384, 2, 6, 1536), n_mels=128)
        m128 = mels(torch, 2, 128)[1]
        rec.put("inf/mels128/hidden", run(enc, "inf/mels128/hidden", lambda: enc.forward_raw(m128, want_hidden=True, want_last=False))[0])
        rec.put("inf/mels128/last_only", run(enc, "inf/mels128/last_only",
                                             lambda: enc.forward_raw(m128, want_hidden=False, want_last=True))[1])
        enc = enc_for((384, 2, 6, 1536), precision="fp32")
        for tag, mel in (("padded", padded), ("dense", dense)):
            key = f"inf/fp32/{tag}"
            h, l = run(enc, key, lambda: enc.forward_raw(mel, want_hidden=True, want_last=True))
            rec.put(key + "/hidden", h)
            rec.put(key + "/last", l)
            rec.put(key + "/last_only", run(enc, key + "/last_only", lambda: enc.forward_raw(mel, want_hidden=False, want_last=True))[1])


def train_model(torch, dims, precision, projs, r, dora):
    """(model, [(name, trainable parameter)]): adapters initialised away from B = 0; projs None = full fine-tuning."""
    from gw_whisper_amd import synth
    from gw_whisper_amd.peft import LoraConfig, get_peft_model
    enc, sd = encoder(dims, precision)
    if projs is None:
        enc = enc.cuda()
        enc.enable_full_finetune()
        for p in enc.parameters():
            p.requires_grad = True
        return enc, list(enc.named_parameters())
    if projs == "all-linear":
        peft = get_peft_model(enc, LoraConfig(use_dora=dora, r=r, lora_alpha=32, target_modules="all-linear")).cuda()
        names = [f"layers.{i}.{p}" for i in range(dims[1]) for p in QKV + ["self_attn.out_proj", "fc1", "fc2"]]
    else:
        names = [f"layers.{i}.{p}" for i in range(dims[1]) for p in projs]
        peft = get_peft_model(enc, LoraConfig(use_dora=dora, r=r, lora_alpha=32, target_modules=names)).cuda()
    with torch.no_grad():
        for j, n in enumerate(names):
            lin = peft.base_model.model.get_submodule(n)
            W0 = sd[n + ".weight"]
            A, Bm, mag = synth.dora_adapter(W0.shape[0], W0.shape[1], r, W0, seed=70 + j)
            lin.lora_A["default"].weight.copy_(torch.from_numpy(A))
            lin.lora_B["default"].weight.copy_(torch.from_numpy(Bm))
            if dora:
                lin.lora_magnitude_vector["default"].weight.copy_(torch.from_numpy(mag))
    return peft, [(n, p) for n, p in peft.named_parameters() if p.requires_grad]


def training(torch, rec):
    tiny2 = (384, 2, 6, 1536)
    padded, _ = mels(torch, 2)
    cases = [  # name, dims, precision, projections, rank, DoRA, d_mel, name part of the gradients summed with float atomics
        ("qkv_r8", tiny2, "bf16", QKV, 8, True, True, "magnitude"),
        ("out_r8", tiny2, "bf16", ["self_attn.out_proj"], 8, True, False, "magnitude"),
        ("all_r4", tiny2, "bf16", "all-linear", 4, True, False, ""),
        ("lora_r8", tiny2, "bf16", QKV, 8, False, False, ""),
        ("full", tiny2, "bf16", None, 0, False, True, ""),
        ("d512_r8", (512, 2, 8, 2048), "bf16", QKV + ["self_attn.out_proj"], 8, True, False, "magnitude"),
        ("d768_r8", (768, 2, 12, 3072), "bf16", QKV + ["self_attn.out_proj"], 8, True, False, "magnitude"),
        ("d128_r8", (128, 2, 2, 512), "bf16", QKV, 8, True, True, "lora_"),
        ("fp32_all_r4", tiny2, "fp32", "all-linear", 4, True, True, ""),
    ]
    for name, dims, precision, projs, r, dora, want_mel, atomic in cases:
        model, params = train_model(torch, dims, precision, projs, r, dora)
        for pooled in (True, False):
            g = torch.Generator().manual_seed(7)
            wl = torch.randn((2, dims[0]) if pooled else (2, 1500, dims[0]), generator=g).cuda()
            mel = padded.clone().requires_grad_(want_mel)
            out = model.last_token(mel) if pooled else model(mel).last_hidden_state
            (out * wl).sum().backward()
            torch.cuda.synchronize()
            key = f"train/{name}/{'pooled' if pooled else 'dense'}"
            rec.put(key + "/out", out)
            for n, p in params:
                if p.grad is not None:
                    rec.put(f"{key}/grad/{n}", p.grad, atomic=bool(atomic) and atomic in n)
                    p.grad = None
            if want_mel:
                rec.put(key + "/d_mel", mel.grad)
        del model, params


def c_entries(torch, rec):
    """What only the C ABI can ask of the training step, through ctypes on the encoder's handle and the *_bytes queries:
    tiny-width two-layer dims, 2 segments, pooled and dense.  d_x0 with no targets; d_x0 with d_mel; base gradients
    (every field) together with an all-linear rank-4 DoRA target set through gww_encoder_train_backward_full, run twice
    (run0 / run1: the same step again on re-zeroed buffers, which shows whether anything on that path sums with float
    atomics); d_x0 through the fp32 entry.  The adapters are merged into the weights the encoder packs, as peft would."""
    from gw_whisper_amd import _lib, synth
    from gw_whisper_amd import encoder as _enc
    from gw_whisper_amd.encoder import WhisperConfig, WhisperEncoder
    lib = _lib.lib()
    dims, B, r, scaling = (384, 2, 6, 1536), 2, 4, 8.0
    mel = mels(torch, B)[0].float().contiguous()
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()
    sd = synth.encoder_state_dict(*dims, seed=3)
    base_shapes = {None: {f: sd[f"{path}.{attr}"].shape for f, path, attr in _enc._fields(_enc._GLOBALS)}}
    for li in range(dims[1]):
        base_shapes[li] = {f: sd[f"layers.{li}.{path}.{attr}"].shape for f, path, attr in _enc._fields(_enc._LAYER)}
    adapters, sd_merged = [], dict(sd)
    for li in range(dims[1]):
        for row in _enc._LAYER:
            if row[4] is not None:
                name = f"layers.{li}.{row[0]}.weight"
                A, Bm, mag = synth.dora_adapter(*sd[name].shape, r, sd[name], seed=90 + len(adapters))
                Wd = sd[name] + scaling * (Bm @ A)
                nrm = np.linalg.norm(Wd, axis=1).astype(np.float32)
                sd_merged[name] = ((mag / nrm)[:, None] * Wd).astype(np.float32)
                adapters.append((li, row[4], row[0], [dev(x) for x in (A, Bm, mag, nrm)]))

    def step(enc, key, pooled, want_x0, want_mel, with_targets=False, bwd="gww_encoder_train_backward"):
        sfx = "_f32" if bwd.endswith("_f32") else ""
        g = torch.Generator().manual_seed(7)
        d_hidden = torch.randn((B, dims[0]) if pooled else (B, 1500, dims[0]), generator=g).cuda()
        enc._sync_weights()
        h = enc._ensure_handle()
        ws_query = "gww_train_workspace_bytes" + ("_full" if bwd.endswith("_full") else sfx)
        ws = torch.empty((getattr(lib, ws_query)(h, B),), dtype=torch.uint8, device="cuda")
        saved = torch.empty((getattr(lib, "gww_train_saved_bytes" + sfx)(h, B),), dtype=torch.uint8, device="cuda")
        hidden = torch.empty_like(d_hidden)
        stream = torch.cuda.current_stream().cuda_stream
        _lib.check(getattr(lib, "gww_encoder_train_forward" + sfx)(
            h, mel.data_ptr(), B, ws.data_ptr(), ws.numel(), saved.data_ptr(), saved.numel(), hidden.data_ptr(), int(pooled),
            stream), "train_forward" + sfx)
        rec.put(key + "/out", hidden)
        d_x0 = torch.zeros((B, 1500, dims[0]), device="cuda") if want_x0 else None
        d_mel = torch.zeros_like(mel) if want_mel else None
        arr, named, extra = (_lib.DoraTarget * max(len(adapters), 1))(), [], ()
        if with_targets:
            for i, (li, pid, mod, (A, Bm, mag, nrm)) in enumerate(adapters):
                dA, dB, dm = torch.zeros_like(A), torch.zeros_like(Bm), torch.zeros_like(mag)
                arr[i] = _lib.DoraTarget(li, pid, r, scaling, A.data_ptr(), Bm.data_ptr(), mag.data_ptr(), nrm.data_ptr(),
                                         dA.data_ptr(), dB.data_ptr(), dm.data_ptr())
                named += [(f"layers.{li}.{mod}.{n}", t) for n, t in (("dA", dA), ("dB", dB), ("dm", dm))]
        if bwd.endswith("_full"):
            gl, layers = _lib.EncGrads(), (_lib.EncLayerGrads * dims[1])()
            gl.layers = layers
            for li, fields in base_shapes.items():
                for f, shape in fields.items():
                    buf = torch.zeros(tuple(shape), device="cuda")
                    setattr(gl if li is None else layers[li], f, buf.data_ptr())
                    named.append((f"base.{f}" if li is None else f"base.layers.{li}.{f}", buf))
            extra = (C.byref(gl),)
        _lib.check(getattr(lib, bwd)(
            h, B, ws.data_ptr(), ws.numel(), saved.data_ptr(), saved.numel(), d_hidden.data_ptr(), arr,
            len(adapters) if with_targets else 0, d_x0.data_ptr() if want_x0 else None,
            d_mel.data_ptr() if want_mel else None, int(pooled), *extra, stream), bwd)
        torch.cuda.synchronize()
        for n, t in named + [("d_x0", d_x0), ("d_mel", d_mel)]:
            if t is not None:
                rec.put(f"{key}/{n}", t)

    plain = WhisperEncoder.from_numpy_state_dict(sd, WhisperConfig(*dims), precision="bf16").cuda()
    merged = WhisperEncoder.from_numpy_state_dict(sd_merged, WhisperConfig(*dims), precision="bf16").cuda()
    plain32 = WhisperEncoder.from_numpy_state_dict(sd, WhisperConfig(*dims), precision="fp32").cuda()
    for pooled in (True, False):
        mode = "pooled" if pooled else "dense"
        step(plain, f"c/x0/{mode}", pooled, True, False)
        step(plain, f"c/x0_mel/{mode}", pooled, True, True)
        for run in (0, 1):
            step(merged, f"c/full_all_r4/{mode}/run{run}", pooled, False, False, True, "gww_encoder_train_backward_full")
        step(plain32, f"c/fp32_x0/{mode}", pooled, True, False, bwd="gww_encoder_train_backward_f32")


def sizes(rec):
    from gw_whisper_amd import _lib, synth
    lib = _lib.lib()
    for name, (d, L, H, F) in sorted(synth.ENCODER_SIZES.items()):
        cfg = _lib.EncCfg(d, L, H, F, synth.encoder_mels(name), 3000)
        h = C.c_void_p()
        _lib.check(lib.gww_encoder_create(C.byref(cfg), C.byref(h)), "gww_encoder_create")
        rows = []
        for split in (0, 1):
            _lib.check(lib.gww_encoder_set_split(h, split), "gww_encoder_set_split")
            for B in (1, 32, 64, 256):
                rows.append([split, B,
                             lib.gww_encoder_workspace_bytes(h, B, _lib.PREC_BF16), lib.gww_encoder_workspace_bytes(h, B, _lib.PREC_F32),
                             lib.gww_train_saved_bytes(h, B), lib.gww_train_workspace_bytes(h, B),
                             lib.gww_train_workspace_bytes_full(h, B), lib.gww_train_workspace_bytes_adapters(h, B, 4),
                             lib.gww_train_workspace_bytes_adapters(h, B, 64), lib.gww_train_saved_bytes_f32(h, B),
                             lib.gww_train_workspace_bytes_f32(h, B)])
        lib.gww_encoder_destroy(h)
        rec.put(f"bytes/{name}", np.asarray(rows, dtype=np.int64))


def compare(path_a, path_b):
    a, b = np.load(path_a), np.load(path_b)
    atomic = set(a["atomic"].tolist())
    assert set(a.files) == set(b.files), sorted(set(a.files) ^ set(b.files))
    bad, n_equal, worst = [], 0, (0.0, "")
    for k in sorted(a.files):
        if np.array_equal(a[k], b[k], equal_nan=False) and a[k].dtype == b[k].dtype:
            n_equal += 1
            continue
        x, y = a[k].astype(np.float64), b[k].astype(np.float64)
        rel = float(np.abs(x - y).max() / max(np.abs(x).max(), 1e-300)) if x.shape == y.shape and np.isfinite(x).all() \
            and np.isfinite(y).all() else float("inf")
        if k in atomic and rel <= ATOMIC_BOUND:
            worst = max(worst, (rel, k))
        else:
            bad.append((k, rel))
    print(f"{len(a.files)} arrays: {n_equal} bit-identical, {len(a.files) - n_equal - len(bad)} atomics-path gradients within "
          f"{ATOMIC_BOUND:g} of their largest entry (worst {worst[0]:.3g}: {worst[1]}), {len(bad)} MISMATCHES")
    for k, rel in bad:
        print("MISMATCH", k, rel)
    return 1 if bad else 0


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--out", default="encoder_paths.npz")
    ap.add_argument("--compare", nargs=2, metavar=("A", "B"), help="compare two results instead of running")
    ap.add_argument("--only", choices=["inference", "training", "c-entries", "sizes"], default=None)
    ap.add_argument("--inference-trace", action="store_true",
                    help="only the inference section, with the encoder's span count per kernel class of every forward "
                         "(for the laboratory library under each GWW_GENERIC_PATH mask, one process per mask)")
    args = ap.parse_args()
    if args.compare:
        sys.exit(compare(*args.compare))
    import torch
    rec = Recorder()
    if args.inference_trace:
        args.only = "inference"
    if args.only in (None, "sizes"):
        sizes(rec)
    if args.only in (None, "inference"):
        inference(torch, rec, trace=args.inference_trace)
    if args.only in (None, "training"):
        training(torch, rec)
    if args.only in (None, "c-entries"):
        c_entries(torch, rec)
    torch.cuda.synchronize()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    np.savez(args.out, atomic=np.asarray(rec.atomic, dtype=str), **rec.out)
    print(f"{len(rec.out)} arrays -> {args.out}")


if __name__ == "__main__":
    main()
