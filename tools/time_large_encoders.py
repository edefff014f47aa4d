"""The wide encoders timed with CUDA events; prints one JSON line.

  * bf16 forward (last_hidden_state) per 64 segments for medium, large and large-v3, with the fraction of the
    2.5 PFLOP/s bf16 peak (FLOPs: the two convs, the four projections, fc1 / fc2 and attention's two products);
  * the 128-bin log-mel kernel against the 80-bin one (64 one-second segments);
  * conv1 at 128 mels: the stem's per-kernel trace (mel_to_tokens + conv1 GEMM) at d = 1024 and 1280, next to the
    direct 80-mel kernel (conv1_mel.hip) at d = 1024, the widest width it covers;
  * a DoRA step (q, k, v of every layer, r 8) of the two-detector classifier at large-v3, 32 x 2 segments.

usage: time_large_encoders.py [--steps N] [--warmup W] [--sizes medium,large,large-v3]"""
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

PEAK = 2.5e15


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    times = []
    for _ in range(steps):
        ev[0].record()
        fn()
        ev[1].record()
        torch.cuda.synchronize()
        times.append(ev[0].elapsed_time(ev[1]))
    times.sort()
    return times[len(times) // 2]


def forward_flops(d, L, F, C, B, Tin=3000):
    T = Tin // 2
    stem = 2 * B * Tin * d * 3 * C + 2 * B * T * d * 3 * d
    layer = 2 * B * T * (4 * d * d + 2 * d * F) + 4 * B * T * T * d
    return stem + L * layer


def encoder(name, precision="bf16"):
    return WhisperEncoder.from_numpy_state_dict(synth.named_encoder_state_dict(name, seed=0), WhisperConfig.named(name),
                                                precision=precision).cuda()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--sizes", default="medium,large,large-v3")
    a = ap.parse_args()
    torch.manual_seed(0)
    B = 64
    wave = torch.from_numpy(synth.strain_segments(B, seed=3)).cuda()
    res = {"segments": B}
    mels = {n: ops.logmel(wave, n_mels=n) for n in (80, 128)}
    res["logmel_ms_per_64"] = {str(n): round(timed(lambda n=n: ops.logmel(wave, n_mels=n), a.steps * 4, a.warmup), 4)
                               for n in (80, 128)}

    res["forward_bf16"] = {}
    for name in a.sizes.split(","):
        d, L, H, F = synth.ENCODER_SIZES[name]
        C = synth.encoder_mels(name)
        enc = encoder(name)
        mel = mels[C]
        with torch.no_grad():
            ms = timed(lambda: enc(mel), a.steps, a.warmup)
            enc.trace_enable(True)
            enc(mel)
            torch.cuda.synchronize()
            tr = enc.trace_read()
            enc.trace_enable(False)
        fl = forward_flops(d, L, F, C, B)
        res["forward_bf16"][name] = {"ms_per_64": round(ms, 2), "frac_of_peak": round(fl / (ms * 1e-3) / PEAK, 3),
                                     "stem_ms": {k: round(v[0], 4) for k, v in tr.items() if k in ("mel_to_tokens", "conv1_gelu")
                                                 and v[1]}}
        del enc
        torch.cuda.empty_cache()

    # conv1: the direct 80-mel kernel at d = 1024 (its widest width) through the stand-alone entry
    w = torch.randn((1024, 80, 3), device="cuda") / 15.5
    b = torch.randn(1024, device="cuda") * 0.02
    res["conv1_direct_80mel_d1024_ms"] = round(timed(lambda: ops.conv1_gelu(mels[80], w, b), a.steps * 4, a.warmup), 4)

    # DoRA step at large-v3, 32 x 2 segments
    enc = WhisperEncoder.from_numpy_state_dict(synth.named_encoder_state_dict("large-v3", seed=0),
                                               WhisperConfig.named("large-v3"), precision="bf16")
    pats = ["layers.*.self_attn.q_proj", "layers.*.self_attn.k_proj", "layers.*.self_attn.v_proj"]
    targets = [n for n, _ in enc.named_modules() if any(fnmatch.fnmatch(n, p) for p in pats)]
    root = get_peft_model(enc, LoraConfig(use_dora=True, r=8, lora_alpha=32, target_modules=targets))
    for name, p in root.named_parameters():
        p.requires_grad = "lora" in name
    model = two_channel_ligo_binary_classifier(root).cuda()
    params = [p for p in model.parameters() if p.requires_grad]
    opt = torch.optim.AdamW(params, lr=1e-5, betas=(0.9, 0.999), eps=1e-8)
    crit = torch.nn.BCEWithLogitsLoss()
    mel0, mel1 = mels[128][:32].contiguous(), mels[128][32:].contiguous()
    y = (torch.arange(32, device="cuda") % 2).float().view(-1, 1)

    def step():
        opt.zero_grad(set_to_none=False)
        crit(model(mel0, mel1), y).backward()
        opt.step()

    res["dora_step_large_v3_32x2_ms"] = round(timed(step, a.steps, a.warmup), 2)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
