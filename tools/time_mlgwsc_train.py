#!/usr/bin/env python3
"""Median time of one InfoNCE pretraining step and one supervised step of the MLGWSC-1 training program
(harness/run_mlgwsc_train.py) at the reference defaults: batch 128 (pretraining: min(128, batch)), two detectors,
whisper-tiny, DoRA r 8 / alpha 32 on q / k / v / out_proj, the train.py adapter (128 x 128 Q-scan).  Batches are built
on the device (gww_assemble_batch_f32) as the harness builds them; the InfoNCE kernels are timed on their own too.

    python tools/time_mlgwsc_train.py [--batch 128] [--steps 6] [--warmup 2] [--encoder tiny]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts)), [round(t, 2) for t in ts]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--encoder", default="tiny")
    a = ap.parse_args()
    from gw_whisper_amd import synth
    from gw_whisper_amd.encoder import WhisperConfig, WhisperEncoder
    from gw_whisper_amd import mlgwsc_train as mt
    from gw_whisper_amd.qscan import QTransformAdapter
    dev = torch.device("cuda")
    torch.manual_seed(0)
    enc = WhisperEncoder.from_numpy_state_dict(synth.named_encoder_state_dict(a.encoder, seed=0),
                                               WhisperConfig.named(a.encoder), precision="bf16")
    enc = mt.apply_lora(enc, r=8, alpha=32, use_dora=True)
    net = mt.build_network(enc, QTransformAdapter.train_variant(n_detectors=2), 2, 2, dev)
    rng = np.random.default_rng(0)
    n = 2 * a.batch
    noises = torch.from_numpy(rng.standard_normal((n, 2, 2048)).astype(np.float32))
    waves = torch.from_numpy((0.1 * rng.standard_normal((n // 2, 2, 2048))).astype(np.float32))
    res = {"batch": a.batch, "encoder": a.encoder, "detectors": 2}

    # InfoNCE kernels alone at (min(128, B), 256)
    z1 = torch.randn(min(128, a.batch), 256, device=dev, requires_grad=True)
    z2 = torch.randn(min(128, a.batch), 256, device=dev, requires_grad=True)

    def nce():
        loss = mt.info_nce(z1, z2, 0.1)
        torch.autograd.grad(loss, (z1, z2))
    res["info_nce_fwd_bwd_ms"], _ = timed(nce, 20, 5)

    pre_ds = mt.PretrainDataset(noises, waves, noise_only_prob=0.25, device=dev)
    pre_dl = iter(mt.DeviceBatches(pre_ds, min(128, a.batch), shuffle=True, seed=1))
    pt = mt.ContrastivePretrainer(net.adapter, net.encoder, 2, device=dev, proj_dim=256, lr=1e-4, temperature=0.1)

    def pre_step():
        nonlocal pre_dl
        try:
            X1, X2 = next(pre_dl)
        except StopIteration:
            pre_dl = iter(mt.DeviceBatches(pre_ds, min(128, a.batch), shuffle=True, seed=1))
            X1, X2 = next(pre_dl)
        pt.step(X1, X2)
    res["pretrain_step_ms"], res["pretrain_all_ms"] = timed(pre_step, a.steps, a.warmup)
    del pt
    torch.cuda.empty_cache()

    data = mt.ConcatGWData([mt.BinaryGWDataset(noises.numpy(), waves.numpy())], dev)
    tr = mt.SupervisedTrainer(net, device=dev, lr=1e-5, clip_norm=100.0, loss_fn=mt.RegBCELoss(dim=2))
    dl = iter(mt.DeviceBatches(data, a.batch, shuffle=True, seed=2))

    def sup_step():
        nonlocal dl
        try:
            X, y = next(dl)
        except StopIteration:
            dl = iter(mt.DeviceBatches(data, a.batch, shuffle=True, seed=2))
            X, y = next(dl)
        net.train()
        loss = tr.loss_fn(net(X), y)
        tr.optimizer.zero_grad()
        loss.backward()
        torch.nn.utils.clip_grad_norm_(net.parameters(), max_norm=tr.clip_norm)
        tr.optimizer.step()
    res["supervised_step_ms"], res["supervised_all_ms"] = timed(sup_step, a.steps, a.warmup)
    res["supervised_ms_per_32_windows"] = res["supervised_step_ms"] * 32 / a.batch
    print(json.dumps(res))


if __name__ == "__main__":
    main()
