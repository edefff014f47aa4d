#!/usr/bin/env python3
"""Time the glitch scan (gw_whisper_amd/glitch_scan.py) on one GPU.

  scan     ``GlitchScanner.scan`` over ``--seconds`` of synthetic conditioned noise (one detector, 0.1 s step, batches of
           ``--batch-size``), for whisper-tiny and whisper-base and both front ends: the reference's (resample to 16 kHz,
           ``ops.logmel``, the 1500-token encoder) and a native one (2048 Hz, 64-point frames every 12 samples: 170 frames,
           an 85-token encoder; the 204-sample step is 17 hops, so the STFT frames of a batch are shared).  Beside each:
           the SAME windows through the front end and the bare pooled encoder pass in the same batches -- no head, no
           events, no read -- so that the difference is what the head launch per batch, the event launches and the one
           host read add.  Host clock around work that ends in a synchronise (the scan
           ends in its read), one warm-up excluded, the median of ``--repeat``.
  events   one ``ops.glitch_events`` call at ``--event-windows`` windows (a day of one detector at 0.1 s is 864 000), for a
           model-like class mix (22 classes, every window a trigger: the dense case), a sparse one (threshold 0.98) and
           one class throughout; device events around the call, the median of ``--repeat``.

Prints one JSON line; ``--out FILE`` also writes it.

usage: time_glitch_scan.py [--seconds 120] [--batch-size 256] [--repeat 5] [--event-windows 864000] [--encoders tiny base]
                           [--out FILE]"""
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
    ap.add_argument("--seconds", type=float, default=120.0)
    ap.add_argument("--batch-size", type=int, default=256)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--event-windows", type=int, default=864000)
    ap.add_argument("--encoders", nargs="+", default=["tiny", "base"])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from gw_whisper_amd import glitch, models, ops, synth
    from gw_whisper_amd.encoder import WhisperConfig, WhisperEncoder
    from gw_whisper_amd.glitch_scan import GlitchScanner
    from gw_whisper_amd.inference import DeviceSegmentSlicer, resample
    from gw_whisper_amd.models import _pooled
    assert torch.cuda.is_available(), "time_glitch_scan needs a GPU"
    C, bs = 22, args.batch_size
    names = [f"class_{i:02d}" for i in range(C)]
    strain = np.random.default_rng(0).standard_normal(int(round(args.seconds * 2048))).astype(np.float32)
    dev = torch.from_numpy(strain).cuda()
    result = {"seconds": args.seconds, "batch_size": bs, "repeat": args.repeat, "scan": [], "events": []}

    def median_wall(fn):
        fn()                                            # warm-up: code objects, allocator, the encoder's workspaces
        torch.cuda.synchronize()
        ts = []
        for _ in range(args.repeat):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        return statistics.median(ts), min(ts), max(ts)

    native_cfg = ops.FrontendConfig(80, 2048, 64, 12, 2048, 0.0, 1024.0)
    for enc_name in args.encoders:
        for front in ("resample", "native"):
            torch.manual_seed(0)
            if front == "resample":
                model = glitch.build_model(enc_name, C, "DoRA", seed=1).eval()
                scanner = GlitchScanner(model, names)
            else:
                d, L, H, F = synth.ENCODER_SIZES[enc_name]
                T_ctx = native_cfg.n_frames // 2
                sd = synth.encoder_state_dict(d, L, H, F, seed=1)
                sd["embed_positions.weight"] = sd["embed_positions.weight"][:T_ctx].copy()
                enc = WhisperEncoder.from_numpy_state_dict(sd, WhisperConfig(d, L, H, F, max_source_positions=T_ctx),
                                                           precision="bf16")
                model = models.glitch_classifier(enc, num_classes=C).cuda().eval()
                scanner = GlitchScanner(model, names, frontend=native_cfg)
            slicer = DeviceSegmentSlicer(dev[None], step_size=0.1, peak_offset=0.8, slice_length=2048)
            n = len(slicer)

            def scan():
                return scanner.scan(dev, start_time=1.0e9, batch_size=bs)

            def bare():
                with torch.no_grad():
                    for i0 in range(0, n, bs):
                        i1 = min(n, i0 + bs)
                        if front == "resample":
                            feats = ops.logmel(resample(slicer.windows(i0, i1)[:, 0].contiguous()))
                        else:
                            feats = scanner.adapter.from_series(slicer.dss, slicer.index_step_size, i0, i1 - i0, window=2048)[:, 0]
                        _pooled(model.encoder, feats)
            t_scan, lo_s, hi_s = median_wall(scan)
            t_bare, lo_b, hi_b = median_wall(bare)
            n_events = len(scan()["class"])
            result["scan"].append({"encoder": enc_name, "frontend": front, "windows": n, "events": n_events,
                                   "scan_s": t_scan, "scan_s_min_max": [lo_s, hi_s], "scan_windows_per_s": n / t_scan,
                                   "bare_encoder_s": t_bare, "bare_s_min_max": [lo_b, hi_b],
                                   "bare_windows_per_s": n / t_bare, "added_ms": 1e3 * (t_scan - t_bare),
                                   "added_us_per_batch": 1e6 * (t_scan - t_bare) / ((n + bs - 1) // bs)})
            del model, scanner
            torch.cuda.empty_cache()

    # ---- one events call at a day's length
    n = args.event_windows
    rng = np.random.default_rng(1)
    step = np.full((n,), 204.0 / 2048.0)
    step[0] = 1.0e9 + 0.8
    times = torch.from_numpy(np.add.accumulate(step)).cuda()
    mixes = {"dense_22_classes": (rng.integers(0, C, n).astype(np.int32), (0.5 + 0.5 * rng.random(n)).astype(np.float32), 0.5),
             "sparse_thr_0.98": (rng.integers(0, C, n).astype(np.int32), rng.random(n).astype(np.float32), 0.98),
             "one_class": (np.zeros(n, np.int32), (0.5 + 0.5 * rng.random(n)).astype(np.float32), 0.5)}
    for name, (cls, prob, thr) in mixes.items():
        cls_d, prob_d = torch.from_numpy(cls).cuda(), torch.from_numpy(prob).cuda()
        ev = ops.glitch_events(times, cls_d, prob_d, thr)           # warm-up
        torch.cuda.synchronize()
        ms = []
        for _ in range(args.repeat):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            ev = ops.glitch_events(times, cls_d, prob_d, thr)
            b.record()
            torch.cuda.synchronize()
            ms.append(a.elapsed_time(b))
        result["events"].append({"mix": name, "windows": n, "events": int(ev["count"].item()), "call_ms": statistics.median(ms),
                                 "call_ms_min_max": [min(ms), max(ms)]})
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
