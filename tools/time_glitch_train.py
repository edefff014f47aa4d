#!/usr/bin/env python3
"""Timings behind ``--head``'s default in harness/run_glitch_train.py (profiles/glitch_train.md).

    head    head step (forward + loss + backward, dropout on) with glitch.head_cross_entropy against
            models.glitch_classifier(...).classifier + nn.CrossEntropyLoss: device-event time over alternating
            iterations after warm-up, B x d_in x C grid
    step    the whole training step (32 one-detector segments, DoRA r 8 on q / k / v, AdamW, bf16) with each head,
            alternating in one call, host wall clock around a synchronise, five repeats.  hip: no host read inside the
            window (the program reads its losses once per epoch); torch: ``loss.item()`` per step as the reference's loop;
            torch_nosync: the torch head without that read, to separate the two effects
    val     a validation pass of 3358 segments (the reference's test-set size): device accumulate + one host read against
            the reference's per-batch ``loss.item()`` + ``argmax(...).cpu()``
    trace   N head steps of ONE kind and nothing else, for a ``rocprofv3 --kernel-trace --stats`` run of its own:
            kernels per step = calls in the trace / N (warm-up steps included in N)

Every mode needs the GPU and prints one JSON line per measurement."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402


def _head(d_in, C, dev):
    from gw_whisper_amd.models import glitch_classifier
    enc = type("Enc", (), {"config": type("Cfg", (), {"d_model": d_in})()})()
    torch.manual_seed(0)
    return glitch_classifier(enc, num_classes=C).classifier.to(dev).train()


def _head_steps(B, d_in, C, dev):
    from gw_whisper_amd import glitch
    cls = _head(d_in, C, dev)
    crit = torch.nn.CrossEntropyLoss()
    x = torch.randn(B, d_in, device=dev)
    y = torch.randint(0, C, (B,), device=dev)
    state = {"n": 0}

    def zero(xr):
        for p in cls.parameters():
            p.grad = None
        return xr

    def hip():
        xr = zero(x.detach().requires_grad_(True))
        state["n"] += 1
        loss, _ = glitch.head_cross_entropy(cls, xr, y, seed=1, offset=state["n"])
        loss.backward()

    def tor():
        xr = zero(x.detach().requires_grad_(True))
        crit(cls(xr), y).backward()

    return {"hip": hip, "torch": tor}


def mode_head(args, dev):
    for B in (32, 256):
        for d_in in (384, 512):
            for C in (11, 22):
                steps = _head_steps(B, d_in, C, dev)
                for _ in range(args.warmup):
                    for f in steps.values():
                        f()
                torch.cuda.synchronize()
                ev = {k: [] for k in steps}
                for _ in range(args.iters):
                    for k, f in steps.items():          # alternating
                        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        a.record()
                        f()
                        b.record()
                        ev[k].append((a, b))
                torch.cuda.synchronize()
                rec = {"mode": "head", "B": B, "d_in": d_in, "C": C, "iters": args.iters}
                for k, pairs in ev.items():
                    us = sorted(1e3 * a.elapsed_time(b) for a, b in pairs)
                    rec[k + "_us_median"], rec[k + "_us_p10"], rec[k + "_us_p90"] = (round(us[len(us) // 2], 2),
                                                                                    round(us[len(us) // 10], 2),
                                                                                    round(us[9 * len(us) // 10], 2))
                print(json.dumps(rec), flush=True)


def mode_trace(args, dev):
    steps = _head_steps(args.batch, args.d_in, args.classes, dev)
    for _ in range(args.iters):
        steps[args.which]()
    torch.cuda.synchronize()
    print(json.dumps({"mode": "trace", "which": args.which, "steps": args.iters, "B": args.batch, "d_in": args.d_in,
                      "C": args.classes}), flush=True)


def _model(encoder, dev, C=11):
    from gw_whisper_amd import glitch
    torch.manual_seed(0)
    return glitch.build_model(encoder, C, "DoRA", 8, 32, "bf16", seed=0, device=dev)


def mode_step(args, dev):
    from gw_whisper_amd import glitch, ops, synth
    from gw_whisper_amd.models import _pooled
    for encoder in ("tiny", "base"):
        model = _model(encoder, dev).train()
        params = [p for p in model.parameters() if p.requires_grad]
        opt = torch.optim.AdamW(params, lr=1e-5)
        crit = torch.nn.CrossEntropyLoss()
        wave, cls, _ = synth.glitch_segments(32, 11, seed=0)
        wave, y = torch.from_numpy(wave).to(dev), torch.from_numpy(cls).to(dev)
        n = {"step": 0}

        def one(kind):
            opt.zero_grad(set_to_none=True)
            mel = ops.logmel(wave)
            if kind == "hip":
                n["step"] += 1
                loss, _ = glitch.head_cross_entropy(model.classifier, _pooled(model.encoder, mel), y, seed=0, offset=n["step"])
                loss.backward()
            else:
                loss = crit(model(mel).float(), y)
                loss.backward()
                if kind == "torch":
                    loss.item()                      # Glitch_classification/src/train.py:108
            opt.step()

        kinds = ("hip", "torch", "torch_nosync")
        for _ in range(args.warmup_steps):
            for k in kinds:
                one(k)
        torch.cuda.synchronize()
        ms = {k: [] for k in kinds}
        for _ in range(5):
            for k in kinds:                              # alternating within every repeat
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(args.steps):
                    one(k)
                torch.cuda.synchronize()
                ms[k].append(1e3 * (time.perf_counter() - t0) / args.steps)
        rec = {"mode": "step", "encoder": encoder, "segments": 32, "steps_per_repeat": args.steps, "repeats": 5}
        for k in kinds:
            rec[k + "_ms"] = [round(v, 4) for v in ms[k]]
            rec[k + "_ms_median"] = round(statistics.median(ms[k]), 4)
        print(json.dumps(rec), flush=True)
        del model, opt


def mode_val(args, dev):
    from gw_whisper_amd import glitch, synth
    model = _model("tiny", dev)
    n = 3358
    wave, cls, _ = synth.glitch_segments(n, 11, seed=1)
    for head in ("hip", "torch"):
        glitch.evaluate_model(model, wave[:256], cls[:256], 32, head)
    s = {"hip": [], "torch": []}
    cms = {}
    for _ in range(3):
        for head in ("hip", "torch"):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            loss, cm = glitch.evaluate_model(model, wave, cls, 32, head)
            torch.cuda.synchronize()
            s[head].append(round(time.perf_counter() - t0, 4))
            cms[head] = (loss, cm)
    print(json.dumps({"mode": "val", "encoder": "tiny", "segments": n, "batch": 32, "hip_s": s["hip"], "torch_s": s["torch"],
                      "confusion_equal": bool(np.array_equal(cms["hip"][1], cms["torch"][1])),
                      "loss_hip": cms["hip"][0], "loss_torch": cms["torch"][0]}), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("mode", choices=("head", "step", "val", "trace"))
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--steps", type=int, default=20, help="step: training steps per timed window")
    ap.add_argument("--warmup-steps", type=int, default=3)
    ap.add_argument("--which", choices=("hip", "torch"), default="hip", help="trace: the head to run")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--d-in", type=int, default=384)
    ap.add_argument("--classes", type=int, default=11)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_glitch_train.py measures on the GPU; there is no CPU figure")
    {"head": mode_head, "step": mode_step, "val": mode_val, "trace": mode_trace}[a.mode](a, torch.device("cuda", 0))
