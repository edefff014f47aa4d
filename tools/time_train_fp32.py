"""Timings of the exact-fp32 training step, in one call:
  * the DoRA step of one encoder (32 segments x 2 detectors, MLP head, BCEWithLogits, AdamW, q / k / v at r = 8: the
    bench's configuration) in bf16 and in fp32, and their ratio (whisper-tiny; --small adds the whisper-small pair);
  * the fp32 attention backward alone at whisper-tiny shapes (64 segments, 6 heads, T = 1500): us per layer and its
    fraction of the 155 TFLOP/s fp32 MFMA peak (7 x 2 T^2 x 64 FLOP per (segment, head): S and dP in both passes, dV,
    dK, dQ);
  * the saved arena and workspace bytes of the fp32 and bf16 steps at 64 segments (the library's size queries).
--profile runs the whisper-tiny fp32 step alone (for a kernel-trace run of its own).
Prints one JSON object; --out also writes it to a file."""

import argparse
import ctypes as C
import fnmatch
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

QKV = ["layers.*.self_attn.q_proj", "layers.*.self_attn.k_proj", "layers.*.self_attn.v_proj"]
FP32_PEAK_TFLOPS = 155.0


def step_ms(precision, enc_name="tiny", batch=32, steps=6, warmup=2):
    from gw_whisper_amd import dist as gdist, ops, synth
    from gw_whisper_amd.encoder import WhisperConfig, WhisperEncoder
    from gw_whisper_amd.models import two_channel_ligo_binary_classifier
    from gw_whisper_amd.peft import LoraConfig, get_peft_model
    dev = torch.device("cuda")
    torch.manual_seed(0)
    sd = synth.named_encoder_state_dict(enc_name, seed=0)
    enc = WhisperEncoder.from_numpy_state_dict(sd, WhisperConfig.named(enc_name), precision=precision)
    targets = [n for n, _ in enc.named_modules() if any(fnmatch.fnmatch(n, p) for p in QKV)]
    peft = get_peft_model(enc, LoraConfig(use_dora=True, r=8, lora_alpha=32, target_modules=targets))
    for name, p in peft.named_parameters():
        p.requires_grad = "lora" in name
    model = two_channel_ligo_binary_classifier(peft).to(dev)
    params = [p for p in model.parameters() if p.requires_grad]
    opt = torch.optim.AdamW(params, lr=1e-4)
    bucket = gdist.FlatGradBucket(params)
    crit = torch.nn.BCEWithLogitsLoss()
    h1 = ops.logmel(torch.from_numpy(synth.strain_segments(batch, seed=7)).to(dev))
    l1 = ops.logmel(torch.from_numpy(synth.strain_segments(batch, seed=77)).to(dev))
    labels = (torch.arange(batch, device=dev) % 2).float()[:, None]
    times = []
    for it in range(warmup + steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        bucket.zero()
        e0.record()
        loss = crit(model(h1, l1), labels)
        loss.backward()
        opt.step()
        e1.record()
        torch.cuda.synchronize()
        if it >= warmup:
            times.append(e0.elapsed_time(e1))
    assert torch.isfinite(loss).all()
    times.sort()
    return {"ms_median": round(times[len(times) // 2], 2), "ms_min": round(times[0], 2), "ms_max": round(times[-1], 2)}


def attention_bwd_us(B=64, Tn=1500, H=6, reps=10):
    from gw_whisper_amd import ops
    g = torch.Generator(device="cuda").manual_seed(0)
    d = 64 * H
    qkv = 0.4 * torch.randn((B, Tn, 3 * d), device="cuda", generator=g)
    dctx = 0.5 * torch.randn((B, Tn, d), device="cuda", generator=g)
    ctx, lse = ops.attention_lse_f32(qkv, H)
    for _ in range(2):
        ops.attention_bwd_f32(qkv, ctx, dctx, lse, H)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        ops.attention_bwd_f32(qkv, ctx, dctx, lse, H)
    e1.record()
    torch.cuda.synchronize()
    us = e0.elapsed_time(e1) * 1e3 / reps
    tflops = 7 * 2.0 * Tn * Tn * 64 * B * H / us / 1e6
    return {"B": B, "T": Tn, "H": H, "us": round(us, 1), "TFLOPs": round(tflops, 1),
            "fraction_of_fp32_peak": round(tflops / FP32_PEAK_TFLOPS, 3)}


def arena_bytes(enc_name, batch):
    from gw_whisper_amd import _lib
    from gw_whisper_amd.encoder import WhisperConfig
    c = WhisperConfig.named(enc_name)
    lib = _lib.lib()
    cfg = _lib.EncCfg(c.d_model, c.encoder_layers, c.encoder_attention_heads, c.encoder_ffn_dim, c.num_mel_bins,
                      2 * c.max_source_positions)
    h = C.c_void_p()
    _lib.check(lib.gww_encoder_create(C.byref(cfg), C.byref(h)), "gww_encoder_create")
    try:
        return {"fp32_saved": int(lib.gww_train_saved_bytes_f32(h, batch)),
                "fp32_workspace": int(lib.gww_train_workspace_bytes_f32(h, batch)),
                "bf16_saved": int(lib.gww_train_saved_bytes(h, batch)),
                "bf16_workspace": int(lib.gww_train_workspace_bytes_adapters(h, batch, 8))}
    finally:
        lib.gww_encoder_destroy(h)


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--out", default=None)
    ap.add_argument("--small", action="store_true", help="also time the whisper-small bf16 and fp32 steps")
    ap.add_argument("--profile", action="store_true", help="only the whisper-tiny fp32 step (3 timed steps)")
    args = ap.parse_args()
    if args.profile:
        res = {"tiny_fp32": step_ms("fp32", steps=3, warmup=1)}
    else:
        res = {"tiny_bf16": step_ms("bf16"), "tiny_fp32": step_ms("fp32")}
        res["tiny_fp32_over_bf16"] = round(res["tiny_fp32"]["ms_median"] / res["tiny_bf16"]["ms_median"], 2)
        if args.small:
            res["small_bf16"] = step_ms("bf16", "small", steps=3, warmup=1)
            res["small_fp32"] = step_ms("fp32", "small", steps=3, warmup=1)
            res["small_fp32_over_bf16"] = round(res["small_fp32"]["ms_median"] / res["small_bf16"]["ms_median"], 2)
        res["attention_bwd_f32_tiny"] = attention_bwd_us()
        res["arena_bytes_64_segments"] = {n: arena_bytes(n, 64) for n in ("tiny", "small", "large-v3")}
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
