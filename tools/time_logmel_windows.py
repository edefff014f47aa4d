#!/usr/bin/env python3
"""Times the front end of the sliding-window consumers at their workload's shape -- a batch of 256 windows of 2048 samples
every 204, two detectors -- on the MI355X (profiles/logmel_windows.md):

  (a) the route before native-rate front ends: ``inference.resample`` to 16 kHz + the published ``ops.logmel`` (30 s frames)
  (b) ``ops.logmel_windows(route="per_window")``: the general kernels on every window, n_fft 128, hop 12
  (c) ``ops.logmel_windows``, the shared route: every STFT frame of the batch once

and then the whole ``inference.evaluate_slices`` pass over 60 s of two-detector noise with a whisper-tiny-width encoder
(d 384, 4 layers, 6 heads) at a context of 85 tokens under (b) and (c).

Method: device events around ``--calls`` back-to-back calls after ``--warmup`` calls of the same shape, ``--repeats``
times, the variants ALTERNATING inside every repeat; the median and the range over the repeats are printed (the range is
the noise a difference has to beat).  (c) against (b) is also checked for equal bits on the timed input.  No GPU, no number:
the tool fails without one.  One JSON line at the end."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402


def timed(fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / calls


def compare(variants, calls, warmup, repeats):
    """{name: (median ms, min ms, max ms)} of the variants, alternated within every repeat."""
    for fn in variants.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    got = {k: [] for k in variants}
    for _ in range(repeats):
        for k, fn in variants.items():
            got[k].append(timed(fn, calls))
    return {k: (float(np.median(v)), float(min(v)), float(max(v))) for k, v in got.items()}


def main(args):
    from gw_whisper_amd import ops, synth
    from gw_whisper_amd.encoder import WhisperConfig, WhisperEncoder
    from gw_whisper_amd.inference import DeviceSegmentSlicer, GWWhisperClassifier, NativeMelAdapter, evaluate_slices, resample
    assert torch.cuda.is_available(), "time_logmel_windows.py needs an MI355X: a CPU gives no number"
    dev = torch.device("cuda", 0)
    L, step, n, D = 2048, 204, args.batch, 2
    cfg = ops.FrontendConfig(80, 2048, 128, 12, L, 0.0, 1024.0)
    rng = np.random.default_rng(0)
    series = torch.from_numpy(rng.standard_normal((D, L + (n - 1) * step)).astype(np.float32)).to(dev)
    plan = ops.logmel_windows_plan(cfg, step, n)
    print(f"batch {n} x {D} detectors, window {L} every {step}, n_fft {cfg.n_fft} hop {cfg.hop_length}: {plan}")

    def parent():
        w = series.as_strided((n, D, L), (step, series.stride(0), 1)).contiguous()
        return ops.logmel(resample(w.reshape(n * D, L)))

    def per_window():
        return ops.logmel_windows(series, cfg, step, n_windows=n, route="per_window")

    def shared():
        return ops.logmel_windows(series, cfg, step, n_windows=n)

    assert torch.equal(per_window(), shared()) and ops.last_logmel_windows_route() == "shared"
    front = compare({"a_resample_published": parent, "b_per_window": per_window, "c_shared": shared}, args.calls, args.warmup,
                    args.repeats)
    for k, (med, lo, hi) in front.items():
        print(f"front end {k:22s} {med:8.4f} ms per batch (range {lo:.4f} .. {hi:.4f})")

    # the whole pass: 60 s of two-detector noise, whisper-tiny width at T 85 (170 frames), batches of 256 windows
    d, layers, heads, ffn = 384, 4, 6, 1536
    sd = synth.encoder_state_dict(d, layers, heads, ffn, seed=1)
    sd["embed_positions.weight"] = sd["embed_positions.weight"][:85].copy()
    enc = WhisperEncoder.from_numpy_state_dict(sd, WhisperConfig(d, layers, heads, ffn, max_source_positions=85), precision="bf16").to(dev)
    strain = rng.standard_normal((D, args.seconds * 2048)).astype(np.float32)
    slicer = DeviceSegmentSlicer(strain, step_size=step / 2048.0, slice_length=L, device=dev)
    nets = {}
    for name, route in (("b_per_window", "per_window"), ("c_shared", None)):
        torch.manual_seed(0)
        nets[name] = GWWhisperClassifier(enc, adapter=NativeMelAdapter(cfg, route=route)).to(dev).eval()
    runs = {k: (lambda net=net: evaluate_slices(slicer, net, batch_size=n)) for k, net in nets.items()}
    sb, sc = (np.concatenate(runs[k]()[1]) for k in ("b_per_window", "c_shared"))
    assert np.array_equal(sb, sc), "the two routes must give the same scores"
    whole = compare(runs, max(1, args.calls // 10), max(1, args.warmup // 5), args.repeats)
    for k, (med, lo, hi) in whole.items():
        print(f"evaluate_slices {k:16s} {med:8.3f} ms per {args.seconds} s segment of {len(slicer)} windows (range {lo:.3f} .. {hi:.3f})")
    print(json.dumps({"batch": n, "detectors": D, "front_end_ms": front, "evaluate_slices_ms": whole, "windows": len(slicer),
                      "device": torch.cuda.get_device_name(0), "plan": plan}))


if __name__ == "__main__":
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--batch", type=int, default=256, help="windows per call")
    p.add_argument("--calls", type=int, default=100, help="back-to-back calls per timing")
    p.add_argument("--warmup", type=int, default=20)
    p.add_argument("--repeats", type=int, default=7)
    p.add_argument("--seconds", type=int, default=60, help="length of the evaluate_slices segment")
    main(p.parse_args())
