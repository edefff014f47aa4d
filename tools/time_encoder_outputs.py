#!/usr/bin/env python3
"""Cost of the encoder's per-layer outputs (output_hidden_states / output_attentions) on one MI355X.

For whisper-tiny and whisper-small, bf16, B 16 and 64: the forward with no flag, with each flag alone and with both
(median of --reps timed calls after --warmup, CUDA events around each call); and the attention-probability kernel alone
(gww_attention_probs_bf16 on a random qkv buffer with q in log2 units, as the encoder's bf16 paths feed it) with its
achieved HBM write rate: B H T^2 4 bytes per call against the 6.3 TB/s the issue's target is stated in.

    python tools/time_encoder_outputs.py [--sizes tiny small] [--batches 16 64] [--reps 10] [--warmup 3]
"""

from __future__ import annotations

import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from gw_whisper_amd import _lib, synth  # noqa: E402
from gw_whisper_amd.encoder import WhisperConfig, WhisperEncoder  # noqa: E402

HBM_TBS = 6.3


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    ms.sort()
    return ms[len(ms) // 2], ms[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", nargs="+", default=["tiny", "small"])
    ap.add_argument("--batches", nargs="+", type=int, default=[16, 64])
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    lib = _lib.lib()
    T = 1500
    results = []
    for name in args.sizes:
        d, L, H, F = synth.ENCODER_SIZES[name]
        enc = WhisperEncoder.from_numpy_state_dict(synth.named_encoder_state_dict(name, seed=1),
                                                   WhisperConfig.named(name), precision="bf16").to(dev)
        for B in args.batches:
            mel = torch.randn(B, 80, 3000, device=dev) * 0.5
            row = {"size": name, "B": B}
            with torch.no_grad():
                for tag, kw in (("plain", {}), ("hidden", {"output_hidden_states": True}),
                                ("attn", {"output_attentions": True}),
                                ("both", {"output_hidden_states": True, "output_attentions": True})):
                    med, best = timed(lambda: enc(mel, **kw), args.reps, args.warmup)
                    row[f"{tag}_ms"] = round(med, 3)
                    row[f"{tag}_best_ms"] = round(best, 3)
            torch.cuda.empty_cache()
            # the probability kernel alone, one layer
            qkv = (torch.randn(B * T, 3 * d, device=dev) * 0.5).to(torch.bfloat16)
            probs = torch.empty(B, H, T, T, device=dev)
            stream = torch.cuda.current_stream().cuda_stream
            fn = lambda: _lib.check(lib.gww_attention_probs_bf16(qkv.data_ptr(), 1, probs.data_ptr(), B, T, H, stream),
                                    "gww_attention_probs_bf16")
            med, best = timed(fn, args.reps, args.warmup)
            nbytes = B * H * T * T * 4
            row["probs_kernel_ms"] = round(med, 4)
            row["probs_write_TBs"] = round(nbytes / (med * 1e-3) / 1e12, 2)
            row["probs_vs_6p3TBs"] = round(med / (nbytes / (HBM_TBS * 1e12) * 1e3), 3)
            del qkv, probs
            torch.cuda.empty_cache()
            results.append(row)
            print(json.dumps(row), flush=True)
        del enc
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
