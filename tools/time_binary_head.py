#!/usr/bin/env python3
"""Timings of the binary head step (csrc/binary_head.hip) against the ``torch.nn`` head it can replace, on the same device
in the same process (profiles/binary_head.md).

    head    forward + backward of the head alone, both layouts, at B = 32 and 256 and d_model = 384 and 768 (the
            two-detector head's d_in is 2 d_model): ``binary.head_bce_with_logits`` (four launches) against
            ``classifier(x)`` + ``BCEWithLogitsLoss`` + autograd; dx and every parameter gradient on both sides.  Also the
            device kernels each side launches per step, counted by torch.profiler in one extra iteration
    step    the whole whisper-tiny DoRA step of harness/run_train.py (log-mel, encoder forward, head, backward, AdamW) at
            B = 32 under ``--head-step torch`` -- the code of the default path: torch head, one ``loss.item()`` per step --
            and under ``--head-step hip`` (HIP head, the loss stays on the device), for --detectors 2 and 1

Device-event time per call over alternating iterations after warm-up; median, p10, p90.  Every mode needs the GPU and
prints one JSON line per configuration."""
import argparse
import fnmatch
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402


def _time(kinds, warmup, iters):
    for _ in range(warmup):
        for f in kinds.values():
            f()
    torch.cuda.synchronize()
    ev = {k: [] for k in kinds}
    for _ in range(iters):
        for k, f in kinds.items():                  # alternating
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            f()
            b.record()
            ev[k].append((a, b))
    torch.cuda.synchronize()
    out = {}
    for k, pairs in ev.items():
        us = sorted(1e3 * a.elapsed_time(b) for a, b in pairs)
        out[k + "_us_median"], out[k + "_us_p10"], out[k + "_us_p90"] = (round(us[len(us) // 2], 2), round(us[len(us) // 10], 2),
                                                                        round(us[9 * len(us) // 10], 2))
    return out


def _launches(f):
    """Device kernels of one call of f, by torch.profiler; None (and the reason) where the profiler is not available."""
    try:
        from torch.profiler import ProfilerActivity, profile
        f()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            f()
            torch.cuda.synchronize()
        names = [e.name for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA")
                 and not e.name.lower().startswith(("memcpy", "memset"))]
        return len(names), sorted(set(names))
    except Exception as e:   # noqa: BLE001 -- a count that cannot be taken is reported as such, the timings stand
        return None, [f"{type(e).__name__}: {e}"]


def _classifier(detectors, d_model, dev):
    from gw_whisper_amd import models
    enc = type("Enc", (torch.nn.Module,), {"config": type("Cfg", (), {"d_model": d_model})()})()
    torch.manual_seed(0)
    cls = models.one_channel_ligo_binary_classifier if detectors == 1 else models.two_channel_ligo_binary_classifier
    return cls(enc).classifier.to(dev)


def mode_head(args, dev):
    from gw_whisper_amd import binary
    crit = torch.nn.BCEWithLogitsLoss()
    for detectors in (1, 2):
        for d_model in (384, 768):
            for B in (32, 256):
                cls = _classifier(detectors, d_model, dev)
                x = torch.randn(B, d_model * detectors, device=dev)
                y = (torch.rand(B, 1, device=dev) > 0.5).float()

                def step(hip):
                    def f():
                        for p in cls.parameters():
                            p.grad = None
                        xr = x.detach().requires_grad_(True)
                        loss = binary.head_bce_with_logits(cls, xr, y)[0] if hip else crit(cls(xr), y)
                        loss.backward()
                        return xr.grad
                    return f
                rec = {"mode": "head", "detectors": detectors, "d_in": d_model * detectors, "B": B, "iters": args.iters,
                       "max_abs_diff_dx_hip_torch": float((step(True)() - step(False)()).abs().max())}
                rec.update(_time({"hip": step(True), "torch": step(False)}, args.warmup, args.iters))
                rec["torch_over_hip"] = round(rec["torch_us_median"] / rec["hip_us_median"], 3)
                rec["hip_kernels"], hip_names = _launches(step(True))
                rec["torch_kernels"], torch_names = _launches(step(False))
                if rec["hip_kernels"] is None or args.names:
                    rec["hip_kernel_names"], rec["torch_kernel_names"] = hip_names, torch_names
                print(json.dumps(rec), flush=True)


def _train_model(detectors, dev, seed=42):
    """harness/run_train.py's default construction: whisper-tiny (seeded weights), bf16, DoRA r = 8 alpha = 32 on q / k / v."""
    from gw_whisper_amd import models, synth
    from gw_whisper_amd.encoder import WhisperConfig, WhisperEncoder
    from gw_whisper_amd.peft import LoraConfig, get_peft_model
    torch.manual_seed(seed)
    d, L, H, F = synth.ENCODER_SIZES["tiny"]
    enc = WhisperEncoder(WhisperConfig.named("tiny"), precision="bf16")
    enc.load_state_dict({k: torch.from_numpy(v) for k, v in synth.encoder_state_dict(d, L, H, F, seed=seed).items()})
    names = [n for n, _ in enc.named_modules()]
    matched = [m for p in ("layers.*.self_attn.q_proj", "layers.*.self_attn.k_proj", "layers.*.self_attn.v_proj",
                           "layers.*.self_attn.o_proj") for m in fnmatch.filter(names, p)]
    peft = get_peft_model(enc, LoraConfig(use_dora=True, r=8, lora_alpha=32, target_modules=matched)).to(dev)
    for name, p in peft.named_parameters():
        p.requires_grad = "lora" in name
    cls = models.one_channel_ligo_binary_classifier if detectors == 1 else models.two_channel_ligo_binary_classifier
    model = cls(peft).to(dev).train()
    params = [p for p in model.parameters() if p.requires_grad]
    return model, torch.optim.AdamW(params, lr=1e-4, betas=(0.9, 0.999), eps=1e-08)


def mode_step(args, dev):
    from gw_whisper_amd import binary, ops, synth
    B = args.batch
    crit = torch.nn.BCEWithLogitsLoss().to(dev)
    for detectors in (2, 1):
        # one model and optimizer per head step, from the same seed: the two runs do not share adapter updates
        runs = {k: _train_model(detectors, dev) for k in ("torch", "hip")}
        wave = torch.from_numpy(synth.strain_segments(B * detectors, seed=7)).to(dev)
        y = (torch.arange(B, device=dev) % 2).float().view(-1, 1)
        kept = []

        def step(kind):
            model, opt = runs[kind]

            def f():
                opt.zero_grad(set_to_none=True)
                mel = ops.logmel(wave)
                mels = (mel,) if detectors == 1 else (mel[:B], mel[B:])
                if kind == "hip":
                    loss, _ = binary.head_bce_with_logits(model.classifier, model.pooled(*mels), y)
                    loss.backward()
                    kept.append(loss.detach())      # read once per epoch in the harness
                else:
                    loss = crit(model(*mels), y)
                    loss.backward()
                    loss.item()                     # the default path's one host read per step
                opt.step()
            return f
        rec = {"mode": "step", "encoder": "tiny", "method": "DoRA", "detectors": detectors, "B": B, "iters": args.iters}
        rec.update(_time({"torch": step("torch"), "hip": step("hip")}, args.warmup, args.iters))
        rec["hip_over_torch"] = round(rec["hip_us_median"] / rec["torch_us_median"], 4)
        rec["last_loss_hip"] = float(kept[-1])
        print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("mode", choices=("head", "step"))
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--batch", type=int, default=32, help="step mode: segments per step")
    ap.add_argument("--names", action="store_true", help="head mode: list the kernel names of both sides")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_binary_head.py measures on the GPU; there is no CPU figure")
    {"head": mode_head, "step": mode_step}[a.mode](a, torch.device("cuda", 0))
