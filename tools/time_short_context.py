#!/usr/bin/env python3
"""Front end, whisper-tiny forward and DoRA step at the default and at two short-context configurations, on one MI355X.

    python tools/time_short_context.py --out profiles/short_context.md

Configurations (input -> front end -> frames -> tokens):
  default   1 s at 16 kHz  -> Whisper's (n_fft 400, hop 160, 30 s chunks)          -> 3000 -> 1500
  gw2048    2 s at 2048 Hz -> n_fft 128, hop 16, 2 s chunks, mel band to 1024 Hz   ->  256 ->  128
  chunk1    1 s at 16 kHz  -> Whisper's window, chunk_length 1                     ->  100 ->   50

Per configuration: segments/s of the front end alone (``ops.logmel``), of the whisper-tiny bf16 forward
(``last_hidden_state``) on features already on the device, and the time of one DoRA training step (r 8 on q / k / v, the
pooled ``last_token`` under a linear head, AdamW) -- each a window of device events around ``--iters`` back-to-back calls
after a warm-up of the same shape, the median of ``--repeats`` windows, with the spread (min .. max) beside it.  Next to
the measured ratios stands the FLOP-count estimate of the encoder forward (an estimate from the shapes, not a measurement).
"""

from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

CONFIGS = {
    # name: (input samples, extractor keyword arguments or None for the default, tokens)
    "default": (16000, None, 1500),
    "gw2048": (4096, dict(sampling_rate=2048, n_fft=128, hop_length=16, chunk_length=2, max_frequency=1024.0), 128),
    "chunk1": (16000, dict(chunk_length=1), 50),
}


def encoder_flops(d, L, F, n_mels, T):
    """Multiply-add FLOPs (2 per MAC) of one segment's encoder forward: the conv stem, per layer the four d x d
    projections, the two MLP GEMMs and the two T x T attention products."""
    stem = 2 * (2 * T) * d * 3 * n_mels + 2 * T * d * 3 * d
    layer = T * (8 * d * d + 4 * d * F) + 4 * T * T * d
    return stem + L * layer


def window(fn, iters):
    """Milliseconds of ``iters`` back-to-back calls between two device events."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def measure(fn, iters, repeats, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = [window(fn, iters) / iters for _ in range(repeats)]
    return statistics.median(ms), min(ms), max(ms)


def main(args):
    from gw_whisper_amd import ops, synth
    from gw_whisper_amd.encoder import WhisperConfig, WhisperEncoder
    from gw_whisper_amd.feature_extraction import WhisperFeatureExtractor
    from gw_whisper_amd.peft import LoraConfig, get_peft_model
    assert torch.cuda.is_available(), "time_short_context.py measures on an MI355X: no GPU, no number"
    dev = torch.device("cuda", 0)
    d, L, H, F = synth.ENCODER_SIZES["tiny"]
    sd = {k: torch.from_numpy(v) for k, v in synth.encoder_state_dict(d, L, H, F, seed=5).items()}
    base = WhisperEncoder(WhisperConfig.named("tiny"))
    base.load_state_dict(sd)
    rows = {}
    for name, (n_in, kw, T) in CONFIGS.items():
        fe = WhisperFeatureExtractor(**(kw or {}))
        assert fe.nb_max_frames == 2 * T
        wave = torch.from_numpy(np.random.default_rng(1).standard_normal((args.batch, n_in)).astype(np.float32)).to(dev)
        logmel = lambda w=wave: ops.logmel(w, config=fe.frontend_config)
        enc = (base if T == 1500 else base.with_context(T)).to(dev)
        mel = logmel()
        with torch.no_grad():
            fwd = lambda: enc(mel).last_hidden_state
            r = {"frontend_ms": measure(logmel, args.iters, args.repeats, args.warmup),
                 "forward_ms": measure(fwd, args.iters, args.repeats, args.warmup)}
        # the DoRA step of harness/run_train.py: r 8 on q / k / v, the pooled token under a linear head, AdamW
        train = WhisperEncoder(enc.config)
        train.load_state_dict(enc.state_dict())
        targets = [f"layers.{i}.self_attn.{p}" for i in range(L) for p in ("q_proj", "k_proj", "v_proj")]
        peft = get_peft_model(train, LoraConfig(use_dora=True, r=8, lora_alpha=32, target_modules=targets)).to(dev)
        head = torch.nn.Linear(d, 1).to(dev)
        params = [p for p in peft.parameters() if p.requires_grad] + list(head.parameters())
        opt = torch.optim.AdamW(params, lr=1e-4)
        mel_t, y = mel[:args.train_batch], torch.zeros((args.train_batch, 1), device=dev)

        def step():
            opt.zero_grad(set_to_none=True)
            loss = torch.nn.functional.binary_cross_entropy_with_logits(head(peft.last_token(mel_t)), y)
            loss.backward()
            opt.step()
        r["dora_step_ms"] = measure(step, args.iters, args.repeats, args.warmup)
        r["tokens"], r["flops_per_segment"] = T, encoder_flops(d, L, F, 80, T)
        rows[name] = r
        print(name, json.dumps(r), flush=True)

    ref = rows["default"]
    lines = ["# Short-context configurations on one MI355X", "",
             f"`python tools/time_short_context.py` -- whisper-tiny, bf16, batch {args.batch} (front end, forward) and "
             f"{args.train_batch} (DoRA step); device events around {args.iters} back-to-back calls after {args.warmup} "
             f"warm-up calls of the same shape, median of {args.repeats} windows (min .. max in brackets).", "",
             "| configuration | tokens | front end, segments/s | forward, segments/s | DoRA step, ms | forward FLOPs per segment (estimate) |",
             "|---|---|---|---|---|---|"]
    rate = lambda t, n: n / (t[0] * 1e-3)
    for name, r in rows.items():
        span = lambda t: f"[{t[1]:.3f} .. {t[2]:.3f} ms]"
        lines.append(f"| {name} | {r['tokens']} | {rate(r['frontend_ms'], args.batch):,.0f} {span(r['frontend_ms'])} | "
                     f"{rate(r['forward_ms'], args.batch):,.0f} {span(r['forward_ms'])} | {r['dora_step_ms'][0]:.3f} "
                     f"{span(r['dora_step_ms'])} | {r['flops_per_segment'] / 1e9:.3f} G |")
    lines += ["", "Ratios to the default configuration (measured: time of the default over time of the configuration; "
              "estimate: FLOPs of the default over FLOPs of the configuration):", "",
              "| configuration | front end | forward | DoRA step | forward FLOP-count estimate |", "|---|---|---|---|---|"]
    for name, r in rows.items():
        lines.append(f"| {name} | {ref['frontend_ms'][0] / r['frontend_ms'][0]:.1f} x | {ref['forward_ms'][0] / r['forward_ms'][0]:.1f} x | "
                     f"{ref['dora_step_ms'][0] / r['dora_step_ms'][0]:.1f} x | {ref['flops_per_segment'] / r['flops_per_segment']:.1f} x |")
    text = "\n".join(lines) + "\n"
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)
    print(text)


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--train-batch", type=int, default=32)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", type=str, default=None)
    main(ap.parse_args())
