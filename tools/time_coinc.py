#!/usr/bin/env python3
"""Time the single-detector coincident search (gw_whisper_amd/coinc.py) on one GPU:

  * ``detector_scores`` over N windows x 2 detectors of white noise with whisper-tiny (bf16, resample + published log-mel,
    batches of 256 windows = 512 encoder rows): one pass, device events around it, after a warm-up on a short segment;
  * the three coincidence launches (``gww_coinc_count_f64``, ``gww_coinc_offsets``, ``gww_coinc_emit_f64``) for S = 100,
    1 000, 10 000 and 65 535 slides, at the event counts that pass produces with the trigger threshold at the 90th and at
    the 99th percentile of its scores: device events around each launch on preallocated buffers, one warm-up excluded, the
    median of ``--repeat``.  The shifts are ``s k`` steps with the largest k for which S slides fit the segment (k = 1 at
    65 535: a timing shape, not a search one would run);
  * for comparison the existing head-level path, ``time_slides.slide_background`` for S = 100 on seeded tokens of the same
    N windows (host clock to its last read: it reads per chunk).

Prints one JSON line; ``--out FILE`` also writes it, ``--md FILE`` writes the table of profiles/coinc_search.md.

usage: time_coinc.py [--windows 65536] [--repeat 10] [--slides 100 1000 10000 65535] [--out FILE] [--md FILE]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--windows", type=int, default=65536)
    ap.add_argument("--repeat", type=int, default=10)
    ap.add_argument("--slides", type=int, nargs="+", default=[100, 1000, 10000, 65535])
    ap.add_argument("--out", default=None)
    ap.add_argument("--md", default=None)
    args = ap.parse_args()
    import torch
    import torch.nn as nn
    from gw_whisper_amd import coinc, models, ops, synth
    from gw_whisper_amd import time_slides as ts
    from gw_whisper_amd._lib import check, lib
    from gw_whisper_amd.encoder import WhisperConfig, WhisperEncoder
    from gw_whisper_amd.inference import DeviceSegmentSlicer
    assert torch.cuda.is_available(), "time_coinc needs a GPU"
    N, step, L = args.windows, 204, 2048

    def ev():
        return torch.cuda.Event(enable_timing=True)

    # ---- the pass: every window of both detectors through whisper-tiny
    enc = WhisperEncoder.from_numpy_state_dict(synth.encoder_state_dict(*synth.ENCODER_SIZES["tiny"], seed=5),
                                               WhisperConfig.named("tiny"), precision="bf16").cuda()
    torch.manual_seed(0)
    model = models.one_channel_ligo_binary_classifier(enc, num_classes=1).cuda().eval()
    with torch.no_grad():
        model.classifier[0].weight.mul_(200.0)            # a seeded head's logits move with the strain (tests)
    rng = np.random.default_rng(0)
    strain = rng.standard_normal((2, L + (N - 1) * step)).astype(np.float32)
    slicer = DeviceSegmentSlicer(strain, start_time=1.0e9)
    assert len(slicer) == N
    coinc.detector_scores(DeviceSegmentSlicer(strain[:, :L + 511 * step], start_time=1.0e9), model)      # warm-up: 2 batches
    torch.cuda.synchronize()
    a, b = ev(), ev()
    a.record()
    scores = coinc.detector_scores(slicer, model)
    b.record()
    torch.cuda.synchronize()
    pass_ms = a.elapsed_time(b)

    # ---- the coincidence launches on that pass's events
    sc = scores.cpu().numpy()
    times_host = slicer.times_host(0, N)
    times = torch.from_numpy(times_host).cuda()
    cap = ts.cluster_capacity(times_host, 0.35)
    stream = torch.cuda.current_stream().cuda_stream
    rows = []
    for pct in (90.0, 99.0):
        thr = float(np.float32(np.percentile(sc, pct)))
        t, v, cnt = ops.cluster_slides(times, scores, thr, 0.35, cap)
        n0, n1 = (int(c) for c in cnt.cpu().numpy())
        for S in args.slides:
            k = max(1, (N - 11) // S)
            shifts = torch.tensor([(s * k) * slicer.time_step_size for s in range(S)], dtype=torch.float64).cuda()
            total = int(ops.coinc_slides(t[0], v[0], n0, t[1], v[1], n1, shifts, 0.15, cap_total=0)["offsets"][-1])
            nb = int(lib().gww_coinc_blocks(n0))
            partner = torch.empty((S, n0), dtype=torch.int32, device="cuda")
            blocks = torch.empty((S * nb,), dtype=torch.int64, device="cuda")
            offsets = torch.empty((S + 1,), dtype=torch.int64, device="cuda")
            out = [torch.empty((max(total, 1),), dtype=dt, device="cuda")
                   for dt in (torch.float64, torch.float64, torch.float64, torch.int32, torch.int32)]
            p = [x.data_ptr() for x in (t[0], v[0], t[1], v[1], shifts, partner, blocks, offsets)]

            def once():
                e = [ev() for _ in range(4)]
                e[0].record()
                check(lib().gww_coinc_count_f64(p[0], 0, n0, p[2], p[3], 0, n1, p[4], S, 0.15, p[5], p[6], stream))
                e[1].record()
                check(lib().gww_coinc_offsets(p[6], n0, S, p[7], stream))
                e[2].record()
                check(lib().gww_coinc_emit_f64(p[0], p[1], 0, n0, p[2], p[3], 0, n1, p[4], S, p[5], p[6], total,
                                               *[o.data_ptr() for o in out], stream))
                e[3].record()
                torch.cuda.synchronize()
                return [e[i].elapsed_time(e[i + 1]) for i in range(3)] + [e[0].elapsed_time(e[3])]
            once()
            runs = [once() for _ in range(args.repeat)]
            med = [statistics.median(r[i] for r in runs) for i in range(4)]
            assert int(offsets[-1]) == total
            rows.append({"threshold_percentile": pct, "events": [n0, n1], "S": S, "shift_steps": k, "coincidences": total,
                         "count_ms": med[0], "offsets_ms": med[1], "emit_ms": med[2], "total_ms": med[3],
                         "share_of_pass": med[3] / pass_ms})
            del partner, blocks, out

    # ---- the existing head-level slides, S = 100, seeded tokens of the same N windows
    D, d = 2, 384
    torch.manual_seed(0)
    head = nn.Sequential(nn.Linear(D * d, 512), nn.ReLU(), nn.Linear(512, 256), nn.ReLU(), nn.Linear(256, 128), nn.ReLU(),
                         nn.Linear(128, 64), nn.ReLU(), nn.Linear(64, 2)).cuda().eval()
    tokens = torch.randn((N, D, d), generator=torch.Generator().manual_seed(1)).cuda()
    plan = ts.slide_plan(N, 0.1, 2.0, 100, 1.0, slicer.time_step_size)
    thr = float(np.percentile(ts.slide_scores(tokens, head, plan.offsets[:1]).cpu().numpy(), 99.0))

    def background_once():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = ts.slide_background(slicer, tokens, head, plan, thr, 0.35)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, len(r[0])
    background_once()
    bg = [background_once() for _ in range(max(3, args.repeat // 3))]

    line = {"N": N, "repeat": args.repeat, "encoder": "tiny bf16", "batch_size": 256,
            "detector_scores_ms": pass_ms, "detector_scores_us_per_window_and_detector": 1e3 * pass_ms / (2 * N),
            "coincidences": rows,
            "slide_background_S100_host_ms": statistics.median(x[0] for x in bg), "slide_background_S100_events": bg[-1][1]}
    print(json.dumps(line), flush=True)
    for path, text in ((args.out, json.dumps(line, indent=1)), (args.md, table(line))):
        if path:
            os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
            with open(path, "w") as f:
                f.write(text)


def table(line):
    out = [f"`detector_scores`, {line['N']} windows x 2 detectors, whisper-{line['encoder']}, batches of {line['batch_size']}: "
           f"{line['detector_scores_ms'] / 1e3:.2f} s ({line['detector_scores_us_per_window_and_detector']:.1f} us per window and "
           f"detector).", "",
           "| threshold percentile | events H1 / L1 | S | coincidences | count ms | offsets ms | emit ms | total ms | share of the pass |",
           "|---|---|---|---|---|---|---|---|---|"]
    for r in line["coincidences"]:
        out.append(f"| {r['threshold_percentile']:.0f} | {r['events'][0]} / {r['events'][1]} | {r['S']} | {r['coincidences']} | "
                   f"{r['count_ms']:.3f} | {r['offsets_ms']:.3f} | {r['emit_ms']:.3f} | {r['total_ms']:.3f} | {r['share_of_pass']:.2e} |")
    out += ["", f"`time_slides.slide_background`, S = 100, the same {line['N']} windows (the existing head-level path, host clock): "
            f"{line['slide_background_S100_host_ms']:.1f} ms, {line['slide_background_S100_events']} events.", ""]
    return "\n".join(out)


if __name__ == "__main__":
    main()
