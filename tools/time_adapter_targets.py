"""Step and kernel timings of adapters beyond rank-8 q / k / v, on whisper-tiny with the bench's
DoRA step (32 segments x 2 detectors, MLP head, BCEWithLogits, AdamW):
  * the step with DoRA on q, k, v at r = 8 (the bench's configuration), on all six linear layers at r = 8, and on
    q, k, v at r = 16 and r = 64;
  * the adapter-gradient kernel (ops.adapter_grads) alone on the fc1 / fc2 shapes of the step (M = 96000 rows):
    effective bytes/s = bytes of x, dy and y read once / time.
Prints one JSON object; --out also writes it to a file."""

import argparse
import fnmatch
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402


def step_ms(pats, r, batch=32, steps=8, warmup=3, enc_name="tiny"):
    from gw_whisper_amd import dist as gdist, ops, synth
    from gw_whisper_amd.encoder import WhisperConfig, WhisperEncoder
    from gw_whisper_amd.models import two_channel_ligo_binary_classifier
    from gw_whisper_amd.peft import LoraConfig, get_peft_model
    dev = torch.device("cuda")
    torch.manual_seed(0)
    sd = synth.named_encoder_state_dict(enc_name, seed=0)
    enc = WhisperEncoder.from_numpy_state_dict(sd, WhisperConfig.named(enc_name), precision="bf16")
    targets = [n for n, _ in enc.named_modules() if any(fnmatch.fnmatch(n, p) for p in pats)]
    peft = get_peft_model(enc, LoraConfig(use_dora=True, r=r, lora_alpha=32, target_modules=targets))
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
    return {"ms_median": times[len(times) // 2], "ms_min": times[0], "ms_max": times[-1], "modules": len(targets), "r": r}


def kernel_rate(d_in, d_out, r, M=96000, reps=20):
    from gw_whisper_amd import ops
    g = torch.Generator(device="cuda").manual_seed(0)
    x = torch.randn((M, d_in), device="cuda", generator=g).bfloat16()
    dy = (0.1 * torch.randn((M, d_out), device="cuda", generator=g)).bfloat16()
    y = torch.randn((M, d_out), device="cuda", generator=g).bfloat16()
    A = torch.randn((r, d_in), device="cuda", generator=g) / d_in ** 0.5
    B = 0.05 * torch.randn((d_out, r), device="cuda", generator=g)
    ones = torch.ones(d_out, device="cuda")
    b = torch.zeros(d_out, device="cuda")
    for _ in range(3):
        ops.adapter_grads(x, dy, y, b, 1.0, 4.0, A, B, ones, ones)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        ops.adapter_grads(x, dy, y, b, 1.0, 4.0, A, B, ones, ones)
    e1.record()
    torch.cuda.synchronize()
    us = e0.elapsed_time(e1) * 1e3 / reps
    bytes_once = M * (d_in + 2 * d_out) * 2
    return {"d_in": d_in, "d_out": d_out, "r": r, "M": M, "us": round(us, 1),
            "effective_TBps": round(bytes_once / us / 1e6, 2)}


QKV = ["layers.*.self_attn.q_proj", "layers.*.self_attn.k_proj", "layers.*.self_attn.v_proj"]
ALL = QKV + ["layers.*.self_attn.out_proj", "layers.*.fc1", "layers.*.fc2"]


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    res = {"steps": {}, "kernel": []}
    res["steps"]["qkv_r8"] = step_ms(QKV, 8)
    res["steps"]["all_linear_r8"] = step_ms(ALL, 8)
    res["steps"]["qkv_r16"] = step_ms(QKV, 16)
    res["steps"]["qkv_r64"] = step_ms(QKV, 64)
    res["steps"]["all_linear_over_qkv"] = round(res["steps"]["all_linear_r8"]["ms_median"] /
                                                res["steps"]["qkv_r8"]["ms_median"], 3)
    for d_in, d_out in ((384, 1536), (1536, 384)):
        for r in (8, 16, 64):
            res["kernel"].append(kernel_rate(d_in, d_out, r))
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
