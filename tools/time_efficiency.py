#!/usr/bin/env python3
"""Timing of the efficiency study on an MI355X (profiles/efficiency_train.md).

    time_efficiency.py step      the training step (batch 32, whisper-tiny bf16, DoRA r 8 on k_proj / v_proj, Adam):
                                 ``--head hip`` (efficiency.reg_bce_head, loss kept on the device) against ``--head torch``
                                 (nn.Sequential + inference.RegBCELoss + ``loss.item()`` per step, as the parent commit has
                                 them)
    time_efficiency.py val       one validation pass (batches of 32): head forward + device accumulate, one read, against
                                 the torch head with ``loss.item()`` and an argmax compare per batch
    time_efficiency.py estimate  a synthetic estimate (``--noise`` pure-noise and ``--snrs`` x ``--signals`` injected
                                 segments): segments/s of the whole pass, and of the statistics alone on the filled buffers

Every figure is the median of ``--repeats`` (default 5) timed runs after a warm-up, with the lowest and highest beside it;
every timed region ends in a device synchronisation.  One JSON line per measurement on stdout."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402


def spread(xs):
    xs = sorted(xs)
    return {"median": xs[len(xs) // 2], "min": xs[0], "max": xs[-1]}


def timed(fn, repeats, warmup=1):
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append(time.perf_counter() - t0)
    return out


def setup(n_wave, n_noise, seed=0):
    from gw_whisper_amd import efficiency
    torch.manual_seed(0)
    model = efficiency.build_model("tiny", seed=5)
    wave, noise = efficiency.synthetic_tensors(n_wave, n_noise, seed=seed)
    return model, torch.from_numpy(wave).cuda(), torch.from_numpy(noise).cuda()


def cmd_step(args):
    from gw_whisper_amd import efficiency, inference
    from gw_whisper_amd.models import _pooled
    model, wave, noise = setup(256, 512)
    ds = efficiency.ResampledDataset(wave, noise, (5., 15.), (0, 256), (0, 256), (256, 512), seed=1)
    crit = inference.RegBCELoss(dim=2, epsilon=1e-6)
    opt = torch.optim.Adam(model.parameters(), lr=1e-4)
    model.train()
    rng = np.random.default_rng(0)
    batches = [ds.batch(rng.permutation(len(ds))[:32])[:2] for _ in range(args.steps)]

    def run(head):
        losses = []
        for mel, targets in batches:
            opt.zero_grad()
            if head == "hip":
                loss, _ = efficiency.reg_bce_head(model.classifier, _pooled(model.encoder, mel), targets, 1e-6)
                loss.backward()
                losses.append(loss.detach())
            else:
                loss = crit(model(mel).float(), targets)
                loss.backward()
                losses.append(loss.detach().item())
            opt.step()
        if torch.is_tensor(losses[0]):
            torch.stack(losses).cpu()
    for head in ("torch", "hip", "torch", "hip"):        # interleaved: a drift of the machine shows as a spread
        ts = [t / args.steps * 1e3 for t in timed(lambda: run(head), args.repeats)]
        print(json.dumps({"what": "train_step_ms", "head": head, "batch": 32, "steps": args.steps, **spread(ts),
                          "samples_per_s": 32e3 / spread(ts)["median"]}), flush=True)


def cmd_val(args):
    from gw_whisper_amd import efficiency, inference, ops
    from gw_whisper_amd.models import _pooled
    model, wave, noise = setup(256, 512)
    ds = efficiency.ResampledDataset(wave, noise, (5., 15.), (0, 256), (0, 256), (256, 512), seed=1)
    crit = inference.RegBCELoss(dim=2, epsilon=1e-6)
    model.eval()
    n = args.batches * 32
    batches = [ds.batch(np.arange(i, i + 32) % len(ds))[:2] for i in range(0, n, 32)]
    params = [t.detach() for t in efficiency._det_parameters(model.classifier)]

    def run(head):
        with torch.no_grad():
            if head == "hip":
                state = efficiency.EvalState("cuda")
                for mel, targets in batches:
                    _, _, probs, row_loss, _ = ops.det_head_forward(_pooled(model.encoder, mel).float(), params, targets, 1e-6)
                    state.add(probs, targets, row_loss)
                state.read()
            else:
                loss, acc = 0.0, 0
                for mel, targets in batches:
                    out = model(mel).float()
                    loss += crit(out, targets).item()
                    acc += int((out.argmax(1) == targets.argmax(1)).sum().item())
    for head in ("torch", "hip", "torch", "hip"):
        ts = timed(lambda: run(head), args.repeats)
        print(json.dumps({"what": "validation_pass_s", "head": head, "segments": n, **spread(ts),
                          "samples_per_s": n / spread(ts)["median"]}), flush=True)


def cmd_estimate(args):
    from gw_whisper_amd import efficiency, ops
    n_sig, n_noise = args.signals, args.noise
    model, wave, noise = setup(min(n_sig, 4096), min(n_noise, 8192))
    model.eval()
    # the index arithmetic clamps to the tensors' ends, so a small resident set stands for the full-size one: the same
    # number of segments goes through assemble -> log-mel -> encoder -> head
    wave_ds = efficiency.ResampledDataset(wave, noise, (0., 0.), (0, n_sig), (0, n_sig), (0, 0))
    noise_ds = efficiency.ResampledDataset(wave, noise, (0., 0.), (0, 0), (0, 0), (0, n_noise))
    snrs = list(np.arange(5, 25, 2))[:args.snrs]
    faps = [0.1, 0.01, 0.001, 0.0001, 0.00001]
    est = efficiency.EfficiencyEstimator(wave_ds, noise_ds, snrs, batch_size=args.batch_size, faps=faps)
    total = n_noise + len(snrs) * n_sig
    ts = timed(lambda: est(model), args.repeats, warmup=1)
    print(json.dumps({"what": "estimate_s", "segments": total, "batch": args.batch_size, **spread(ts),
                      "segments_per_s": total / spread(ts)["median"]}), flush=True)
    scores = torch.randn(n_noise, device="cuda")
    ws = torch.randn(n_sig, device="cuda")
    ranks = torch.from_numpy(efficiency.false_alarm_ranks(faps, n_noise).astype(np.int64)).cuda()

    def stats():
        thr = ops.score_thresholds(scores, ranks)
        table = torch.zeros((len(snrs), len(faps)), dtype=torch.int64, device="cuda")
        for s in range(len(snrs)):
            ops.detection_counts(ws, thr, table[s])
        table.cpu()
    ts = [t * 1e3 for t in timed(stats, args.repeats)]
    print(json.dumps({"what": "statistics_ms", "noise": n_noise, "signals": n_sig, "snrs": len(snrs), **spread(ts)}), flush=True)

    def host_stats():                     # the reference's way: sort, index, one compare per batch of 16, on torch
        srt = torch.sort(scores).values
        thr = torch.tensor([srt[-int(r)] for r in ranks.tolist()], device="cuda")[None]
        for s in range(len(snrs)):
            det = torch.zeros(len(faps), dtype=torch.int64, device="cuda")
            for i in range(0, n_sig, 16):
                det += torch.sum(ws[i:i + 16, None] > thr, 0)
            det.cpu()
    if args.reference_stats:
        ts = [t * 1e3 for t in timed(host_stats, max(args.repeats // 2, 1))]
        print(json.dumps({"what": "statistics_torch_batches_of_16_ms", **spread(ts)}), flush=True)


if __name__ == "__main__":
    p = argparse.ArgumentParser()
    p.add_argument("what", choices=("step", "val", "estimate"))
    p.add_argument("--repeats", type=int, default=5)
    p.add_argument("--steps", type=int, default=40)
    p.add_argument("--batches", type=int, default=64)
    p.add_argument("--signals", type=int, default=100000)
    p.add_argument("--noise", type=int, default=400000)
    p.add_argument("--snrs", type=int, default=10)
    p.add_argument("--batch-size", type=int, default=256)
    p.add_argument("--reference-stats", action="store_true")
    a = p.parse_args()
    assert torch.cuda.is_available(), "time_efficiency.py needs an MI355X"
    {"step": cmd_step, "val": cmd_val, "estimate": cmd_estimate}[a.what](a)
