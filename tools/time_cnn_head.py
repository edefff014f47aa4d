#!/usr/bin/env python3
"""Timings of the CNN decoder head (csrc/cnn_head.hip) against the same ``nn.Sequential`` in ``torch.nn`` fp32 on the same
device (profiles/cnn_head.md).

    fwd     the inference forward at (B = 256, d = 384, C = 1): ``ops.cnn_head_forward`` against ``classifier(x)`` under
            no_grad.  Also the HIP forward as a share of the fp32-MFMA peak: the operations the chain needs, counted from
            its shapes, over the measured time
    step    forward + backward at (B = 32, d = 384, C = 1): ``_CnnHead`` (HIP forward with saved activations + HIP
            backward) against ``classifier(x)`` + autograd; dx and all eight parameter gradients on both sides

Device-event time per call over alternating iterations after warm-up; median, p10, p90.  Both kinds run in one call.
Every mode needs the GPU and prints one JSON line."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

PEAK_F32_MFMA = 157.3e12   # MI355X, v_mfma_f32_*_f32, FLOP/s


def chain_flops(B, d, C):
    """Multiply-adds x 2 of the three convolutions and the Linear (bias, ReLU and the mean not counted)."""
    return 2 * B * (d * 3 * (2 * 64 + 64 * 128 + 128 * 256) + 256 * C)


def _model(d, C, dev, head):
    from gw_whisper_amd.models import TwoChannelLIGOBinaryClassifierCNN
    enc = type("Enc", (torch.nn.Module,), {"config": type("Cfg", (), {"d_model": d})()})()
    torch.manual_seed(0)
    return TwoChannelLIGOBinaryClassifierCNN(enc, num_classes=C, head=head).to(dev)


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


def mode_fwd(args, dev):
    B, d, C = args.batch or 256, args.d, args.classes
    hip, tor = _model(d, C, dev, "hip").eval(), _model(d, C, dev, "torch").eval()
    tor.classifier.load_state_dict(hip.classifier.state_dict())
    x = torch.randn(B, 2, d, device=dev)

    def run_hip():
        with torch.no_grad():
            return hip.decode(x)

    def run_torch():
        with torch.no_grad():
            return tor.decode(x)
    diff = float((run_hip() - run_torch()).abs().max())
    rec = {"mode": "fwd", "B": B, "d": d, "C": C, "iters": args.iters, "max_abs_diff_hip_torch": diff}
    rec.update(_time({"hip": run_hip, "torch": run_torch}, args.warmup, args.iters))
    rec["torch_over_hip"] = round(rec["torch_us_median"] / rec["hip_us_median"], 3)
    flops = chain_flops(B, d, C)
    rec["gflop"] = round(flops / 1e9, 3)
    rec["hip_tflops"] = round(flops / (rec["hip_us_median"] * 1e-6) / 1e12, 2)
    rec["hip_share_of_f32_mfma_peak"] = round(flops / (rec["hip_us_median"] * 1e-6) / PEAK_F32_MFMA, 4)
    print(json.dumps(rec), flush=True)


def mode_step(args, dev):
    B, d, C = args.batch or 32, args.d, args.classes
    hip, tor = _model(d, C, dev, "hip").train(), _model(d, C, dev, "torch").train()
    tor.classifier.load_state_dict(hip.classifier.state_dict())
    x = torch.randn(B, 2, d, device=dev)
    w = torch.randn(B, C, device=dev)

    def step(model):
        def f():
            for p in model.classifier.parameters():
                p.grad = None
            xr = x.detach().requires_grad_(True)
            (model.decode(xr) * w).sum().backward()
            return xr.grad
        return f
    rec = {"mode": "step", "B": B, "d": d, "C": C, "iters": args.iters,
           "max_abs_diff_dx_hip_torch": float((step(hip)() - step(tor)()).abs().max())}
    rec.update(_time({"hip": step(hip), "torch": step(tor)}, args.warmup, args.iters))
    rec["torch_over_hip"] = round(rec["torch_us_median"] / rec["hip_us_median"], 3)
    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("mode", choices=("fwd", "step"))
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--batch", type=int, default=0, help="default: 256 (fwd), 32 (step)")
    ap.add_argument("--d", type=int, default=384)
    ap.add_argument("--classes", type=int, default=1)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_cnn_head.py measures on the GPU; there is no CPU figure")
    {"fwd": mode_fwd, "step": mode_step}[a.mode](a, torch.device("cuda", 0))
