#!/usr/bin/env python3
"""Time the search background from time slides (gw_whisper_amd/time_slides.py) on one GPU: N windows of tiny-width tokens
(D = 2, d = 384), S slides through the first-layer partials, the slid scores and the clustering, against

  * the only way to the same numbers without it: per slide, the torch head on the gathered rows
    ``cat(tok[:, 0], roll(tok[:, 1], -o))`` followed by ``inference.cluster_triggers_device``;
  * the encoder pass over the same N windows (whisper-tiny, ``last_token``, batches of 256 log-mels): ``--enc-batches``
    batches are timed and scaled to the N * D / 256 the pass needs.

Device events around each stage, one warm-up excluded, the median of ``--repeat``; the baseline ends in a host read per
slide (that is how it works), so its figure is the host clock to the last read.  The score kernel's FLOP count is
2 (512 * 256 + 256 * 128 + 128 * 64 + 64 C) per pair, its share of peak is against the 157 TFLOP/s of the fp32 MFMA.
Prints one JSON line; ``--out FILE`` also writes it.

usage: time_slides.py [--windows 65536] [--slides 100] [--repeat 10] [--enc-batches 8] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_F32_MFMA = 157.0e12


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--windows", type=int, default=65536)
    ap.add_argument("--slides", type=int, default=100)
    ap.add_argument("--repeat", type=int, default=10)
    ap.add_argument("--enc-batches", type=int, default=8)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import torch.nn as nn
    from gw_whisper_amd import inference as inf
    from gw_whisper_amd import ops, synth
    from gw_whisper_amd import time_slides as ts
    from gw_whisper_amd.encoder import WhisperConfig, WhisperEncoder
    assert torch.cuda.is_available(), "time_slides needs a GPU"
    N, S, D, d, C = args.windows, args.slides, 2, 384, 2
    torch.manual_seed(0)
    head = nn.Sequential(nn.Linear(D * d, 512), nn.ReLU(), nn.Linear(512, 256), nn.ReLU(), nn.Linear(256, 128), nn.ReLU(),
                         nn.Linear(128, 64), nn.ReLU(), nn.Linear(64, C)).cuda().eval()
    tokens = torch.randn((N, D, d), generator=torch.Generator().manual_seed(1)).cuda()
    step = 204.0 / 2048.0
    steps = np.full((N,), step)
    steps[0] = 1.0e9
    times_host = np.add.accumulate(steps) + 0.6
    times = torch.from_numpy(times_host).cuda()
    plan = ts.slide_plan(N, 0.1, 2.0, S, 1.0, step)
    assert len(plan.offsets) == S, "every slide must fit the segment"
    lin, _ = ts.head_layers(head)
    params = ts._tail_params(lin)
    cap = ts.cluster_capacity(times_host, 0.35)
    thr = float(np.percentile(ts.slide_scores(tokens, head, plan.offsets[:1]).cpu().numpy(), 99.0))

    def ev():
        return torch.cuda.Event(enable_timing=True)

    def slides_once():
        e = [ev() for _ in range(4)]
        e[0].record()
        P = ts.head_partials(tokens, head)
        e[1].record()
        sc = ops.slide_scores(P, params, plan.offsets)
        e[2].record()
        out = ops.cluster_slides(times, sc, thr, 0.35, cap)
        e[3].record()
        torch.cuda.synchronize()
        return {"partials_ms": e[0].elapsed_time(e[1]), "scores_ms": e[1].elapsed_time(e[2]),
                "cluster_ms": e[2].elapsed_time(e[3]), "total_ms": e[0].elapsed_time(e[3])}, sc, out

    def baseline_once():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        n_events, first = 0, None
        with torch.no_grad():
            for o in plan.offsets:
                rows = torch.cat((tokens[:, 0], torch.roll(tokens[:, 1], -o, dims=0)), dim=1)
                sc = head(rows)[:, 0].contiguous()
                if first is None:
                    first = sc
                n_events += len(inf.cluster_triggers_device(times, sc, thr, 0.35)[0])
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, n_events, first

    slides_once()
    runs = [slides_once() for _ in range(args.repeat)]
    new = {k: statistics.median(r[0][k] for r in runs) for k in runs[0][0]}
    sc, (_, _, cnt) = runs[-1][1], runs[-1][2]
    baseline_once()
    base = [baseline_once() for _ in range(max(3, args.repeat // 3))]
    base_ms = statistics.median(b[0] for b in base)
    diff = float((sc[0] - base[-1][2]).abs().max())

    # the encoder pass: whisper-tiny, bf16, last_token on batches of 256 log-mels
    size = synth.ENCODER_SIZES["tiny"]
    enc = WhisperEncoder.from_numpy_state_dict(synth.encoder_state_dict(*size, seed=5), WhisperConfig.named("tiny"),
                                               precision="bf16").cuda()
    mel = torch.randn((256, 80, 3000), generator=torch.Generator().manual_seed(2)).cuda()
    with torch.no_grad():
        enc.last_token(mel)
        torch.cuda.synchronize()
        per_batch = []
        for _ in range(args.repeat):
            a, b = ev(), ev()
            a.record()
            for _ in range(args.enc_batches):
                enc.last_token(mel)
            b.record()
            torch.cuda.synchronize()
            per_batch.append(a.elapsed_time(b) / args.enc_batches)
    enc_batch_ms = statistics.median(per_batch)
    enc_pass_ms = enc_batch_ms * (N * D / 256.0)

    flop = 2.0 * (512 * 256 + 256 * 128 + 128 * 64 + 64 * C) * S * N
    line = {"N": N, "S": S, "D": D, "d": d, "C": C, "repeat": args.repeat, "threshold_percentile": 99.0, "cap": cap,
            "slides_device_events_ms": new, "slid_events": int(cnt.sum().item()),
            "baseline_torch_head_plus_cluster_per_slide_host_ms": base_ms, "baseline_events": base[-1][1],
            "max_abs_score_difference_slide_1": diff,
            "encoder_last_token_batch256_ms": enc_batch_ms, "encoder_pass_ms_scaled": enc_pass_ms,
            "slides_share_of_encoder_pass": new["total_ms"] / enc_pass_ms,
            "baseline_over_slides": base_ms / new["total_ms"],
            "score_kernel_tflops": flop / (new["scores_ms"] * 1e-3) / 1e12,
            "score_kernel_share_of_f32_mfma_peak": flop / (new["scores_ms"] * 1e-3) / PEAK_F32_MFMA}
    print(json.dumps(line), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(line, f, indent=1)


if __name__ == "__main__":
    main()
