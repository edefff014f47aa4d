"""Whisper-tiny full fine-tuning step next to the DoRA step, timed with CUDA events: 32 x 2 segments through
``two_channel_ligo_binary_classifier`` (pooled last token), BCE loss, AdamW, the re-pack of the changed weights
included (Signal_vs_Noise/src/train.py:163-168 with the models of :243-269).  Also times the weight-gradient GEMM
alone at M = 96 000 on the tiny shapes.  Prints one JSON line.  usage: time_full_finetune.py [--steps N] [--warmup W]"""
import argparse
import fnmatch
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from gw_whisper_amd import ops, synth  # noqa: E402
from gw_whisper_amd.encoder import WhisperConfig, WhisperEncoder  # noqa: E402
from gw_whisper_amd.models import two_channel_ligo_binary_classifier  # noqa: E402
from gw_whisper_amd.peft import LoraConfig, get_peft_model  # noqa: E402


def step_ms(method, mel0, mel1, y, steps, warmup):
    enc = WhisperEncoder.from_numpy_state_dict(synth.named_encoder_state_dict("tiny", seed=0), WhisperConfig.named("tiny"),
                                               precision="bf16")
    if method == "full_finetune":
        root = enc.enable_full_finetune()
    else:
        pats = ["layers.*.self_attn.q_proj", "layers.*.self_attn.k_proj", "layers.*.self_attn.v_proj"]
        targets = [n for n, _ in enc.named_modules() if any(fnmatch.fnmatch(n, p) for p in pats)]
        root = get_peft_model(enc, LoraConfig(use_dora=True, r=8, lora_alpha=32, target_modules=targets))
        for name, p in root.named_parameters():
            p.requires_grad = "lora" in name
    model = two_channel_ligo_binary_classifier(root).cuda()
    if method == "full_finetune":
        for p in model.parameters():
            p.requires_grad = True
    params = [p for p in model.parameters() if p.requires_grad]
    opt = torch.optim.AdamW(params, lr=1e-5, betas=(0.9, 0.999), eps=1e-8)
    crit = torch.nn.BCEWithLogitsLoss()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    times = []
    for it in range(warmup + steps):
        ev[0].record()
        opt.zero_grad(set_to_none=False)
        loss = crit(model(mel0, mel1), y)
        loss.backward()
        opt.step()
        ev[1].record()
        torch.cuda.synchronize()
        if it >= warmup:
            times.append(ev[0].elapsed_time(ev[1]))
    times.sort()
    return {"ms_median": times[len(times) // 2], "ms_min": times[0], "trainable": sum(p.numel() for p in params),
            "loss": float(loss)}


def wgrad_tflops(steps):
    out = {}
    M = 96000
    for N, K in ((1152, 384), (384, 384), (1536, 384), (384, 1536)):
        dy = torch.randn((M, N), device="cuda").bfloat16()
        x = torch.randn((M, K), device="cuda").bfloat16()
        dw = torch.zeros((N, K), device="cuda")
        db = torch.zeros((N,), device="cuda")
        for _ in range(3):
            ops.gemm_wgrad(dy, x, dw=dw, db=db)
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ev[0].record()
        for _ in range(steps):
            ops.gemm_wgrad(dy, x, dw=dw, db=db)
        ev[1].record()
        torch.cuda.synchronize()
        ms = ev[0].elapsed_time(ev[1]) / steps
        tf = 2.0 * M * N * K / (ms * 1e-3) / 1e12
        out[f"{N}x{K}"] = {"us": round(ms * 1e3, 1), "tflops": round(tf, 1), "frac_of_2500": round(tf / 2500, 3)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=32)
    a = ap.parse_args()
    torch.manual_seed(0)
    w = torch.from_numpy(synth.strain_segments(2 * a.batch, seed=3)).cuda()
    mel = ops.logmel(w)
    mel0, mel1 = mel[: a.batch].contiguous(), mel[a.batch:].contiguous()
    y = (torch.arange(a.batch, device="cuda") % 2).float().view(-1, 1)
    res = {"batch": a.batch, "dora": step_ms("DoRA", mel0, mel1, y, a.steps, a.warmup),
           "full_finetune": step_ms("full_finetune", mel0, mel1, y, a.steps, a.warmup)}
    res["ratio_full_over_dora"] = round(res["full_finetune"]["ms_median"] / res["dora"]["ms_median"], 3)
    res["wgrad_M96000"] = wgrad_tflops(a.steps)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
