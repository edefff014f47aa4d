#!/usr/bin/env python3
"""Golden vectors of the MLGWSC-1 training program (``tests/golden/mlgwsc_train.npz``) from the reference's OWN
definitions in ``MLGWSC-1/train.py``, executed where they lie through ``tools/make_golden._reference_defs`` (nothing of
the text is stored; inputs come from seeds, only numbers are written).  Build container only, like ``make_golden.py``.

    python tools/make_golden_mlgwsc.py

  nce{k}_*   ``ContrastivePretrainer._info_nce`` called unbound on a namespace holding ``temp`` and ``_l2norm``, in fp64,
             with autograd gradients: (B, P, tau) = (1, 256, 0.1), (4, 256, 0.1), (37, 100, 0.05), (128, 256, 0.1),
             (16, 256, 0.01) -- where the fp32 reference overflows and fp64 does not -- and (8, 64, 0.1) with an all-zero
             row.  z1, z2 are ``numpy.random.default_rng(seed).standard_normal`` draws, stored as the fp32 inputs.
  pre_*      ``PretrainDataset.__getitem__`` items (D 2, T 64) with ``ds.rng = default_rng(seed)``: the generator calls it
             made, in order, and the two views it returned (noise-only pairs included).
  bin_*      ``BinaryGWDataset.__getitem__`` items likewise: the SNR draws, signals and labels.
  bce_*      ``RegBCELoss`` values.
"""

from __future__ import annotations

import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.make_golden import GOLD, _reference_defs  # noqa: E402

NCE_CASES = [(1, 256, 0.1, False), (4, 256, 0.1, False), (37, 100, 0.05, False), (128, 256, 0.1, False),
             (16, 256, 0.01, False), (8, 64, 0.1, True)]


def nce_inputs(k: int, B: int, P: int, zero_row: bool):
    """The fp32 z1, z2 of case k (the GPU test regenerates nothing: they are stored)."""
    rng = np.random.default_rng(1000 + k)
    z1 = (rng.standard_normal((B, P)) * 0.7).astype(np.float32)
    z2 = (z1 + 2.0 * rng.standard_normal((B, P))).astype(np.float32)      # positives correlated with their pair
    if zero_row:
        z1[3] = 0.0
    return z1, z2


class _Recorder:
    """numpy Generator proxy that logs every call the reference's __getitem__ makes (test INPUT plumbing)."""

    def __init__(self, rng):
        self.rng, self.log = rng, []

    def random(self, *a, **k):
        v = self.rng.random(*a, **k)
        self.log.append(("random", float(v)))
        return v

    def integers(self, *a, **k):
        v = self.rng.integers(*a, **k)
        self.log.append(("integers", float(v)))
        return v

    def uniform(self, *a, **k):
        v = self.rng.uniform(*a, **k)
        self.log.append(("uniform", float(v)))
        return v


def main():
    import torch.nn.functional as F
    from torch.utils.data import Dataset as TorchDataset
    ns = _reference_defs("MLGWSC-1/train.py", ["ContrastivePretrainer", "BinaryGWDataset", "PretrainDataset", "RegBCELoss"],
                         {"F": F, "TorchDataset": TorchDataset})
    out = {}
    CP = ns["ContrastivePretrainer"]
    for k, (B, P, tau, zero_row) in enumerate(NCE_CASES):
        z1, z2 = nce_inputs(k, B, P, zero_row)
        a = torch.from_numpy(z1).double().requires_grad_(True)
        b = torch.from_numpy(z2).double().requires_grad_(True)
        self_ = types.SimpleNamespace(temp=tau, _l2norm=CP._l2norm)
        loss = CP._info_nce(self_, a, b)
        loss.backward()
        with torch.no_grad():
            f32 = CP._info_nce(types.SimpleNamespace(temp=tau, _l2norm=CP._l2norm), a.float(), b.float())
        out[f"nce{k}_z1"], out[f"nce{k}_z2"] = z1, z2
        out[f"nce{k}_tau"] = np.float64(tau)
        out[f"nce{k}_loss"] = np.float64(loss.item())
        out[f"nce{k}_dz1"] = a.grad.numpy().astype(np.float32)
        out[f"nce{k}_dz2"] = b.grad.numpy().astype(np.float32)
        out[f"nce{k}_loss_ref_fp32"] = np.float64(f32.item())
        print(f"nce case {k}: B {B} P {P} tau {tau}: loss fp64 {loss.item():.6f}, fp32 reference {f32.item()}")
    out["nce_cases"] = np.int64(len(NCE_CASES))

    # ---- PretrainDataset items
    rng = np.random.default_rng(7)
    noises = rng.standard_normal((7, 2, 64)).astype(np.float32)
    waves = (0.3 * rng.standard_normal((5, 2, 64))).astype(np.float32)
    ds = ns["PretrainDataset"](torch.from_numpy(noises), torch.from_numpy(waves), snr_range=(5.0, 15.0),
                               noise_only_prob=0.4, device="cpu")
    ds.rng = rec = _Recorder(np.random.default_rng(11))
    idx = np.array([0, 3, 1, 4, 2, 2, 0, 4, 1, 3, 3, 0, 2, 1, 4, 0], np.int64)
    x1, x2, calls = [], [], []
    for i in idx:
        n0 = len(rec.log)
        a, b = ds[int(i)]
        x1.append(a.numpy()), x2.append(b.numpy())
        calls.append([c for c in rec.log[n0:]])
    only = np.array([len(c) == 3 for c in calls])          # random, integers, integers  vs  random, uniform, integers x 2
    n1 = np.array([c[1][1] if o else c[2][1] for c, o in zip(calls, only)], np.int64)
    n2 = np.array([c[2][1] if o else c[3][1] for c, o in zip(calls, only)], np.int64)
    snr = np.array([0.0 if o else c[1][1] for c, o in zip(calls, only)], np.float64)
    assert all([n for n, _ in c] == (["random", "integers", "integers"] if o else ["random", "uniform", "integers", "integers"])
               for c, o in zip(calls, only))
    assert only.any() and (~only).any()
    out.update(pre_noises=noises, pre_waves=waves, pre_seed=np.int64(11), pre_prob=np.float64(0.4), pre_idx=idx,
               pre_noise_only=only, pre_n1=n1, pre_n2=n2, pre_snr=snr, pre_x1=np.stack(x1), pre_x2=np.stack(x2))
    # the views are the fp32 product rounded, then the fp32 sum rounded
    for k in np.nonzero(~only)[0]:
        s = np.float32(snr[k])
        assert np.array_equal(out["pre_x1"][k], noises[n1[k]] + s * waves[idx[k]])

    # ---- BinaryGWDataset items
    noises = rng.standard_normal((9, 2, 64)).astype(np.float32)
    waves = (0.3 * rng.standard_normal((4, 2, 64))).astype(np.float32)
    bd = ns["BinaryGWDataset"](noises=noises, waveforms=waves, store_device="cpu", train_device="cpu", snr_range=(5.0, 15.0))
    bd.rng = rec = _Recorder(np.random.default_rng(13))
    bidx = np.array([8, 0, 3, 5, 1, 7, 2, 2, 6, 4, 0, 3], np.int64)
    xs, labels, snrs = [], [], []
    for i in bidx:
        n0 = len(rec.log)
        x, lab = bd[int(i)]
        xs.append(x.numpy()), labels.append(lab.numpy())
        snrs.append(rec.log[n0][1] if len(rec.log) > n0 else 0.0)
    out.update(bin_noises=noises, bin_waves=waves, bin_seed=np.int64(13), bin_idx=bidx, bin_snr=np.array(snrs),
               bin_x=np.stack(xs), bin_labels=np.stack(labels))
    for k, i in enumerate(bidx):
        if i < len(waves):
            assert np.array_equal(out["bin_x"][k], noises[i] + np.float32(snrs[k]) * waves[i])

    # ---- RegBCELoss
    g = torch.Generator().manual_seed(3)
    p = torch.softmax(torch.randn(6, 2, generator=g), dim=1)
    p[0] = torch.tensor([1.0, 0.0])                       # the epsilon keeps log(0) away
    y = torch.nn.functional.one_hot(torch.tensor([0, 1, 1, 0, 1, 0]), 2).float()
    out["bce_p"], out["bce_y"] = p.numpy(), y.numpy()
    out["bce_loss"] = np.float64(ns["RegBCELoss"](dim=2)(p, y).item())
    out["bce_loss_eps"] = np.float64(ns["RegBCELoss"](dim=2, epsilon=1e-3)(p, y).item())

    path = os.path.join(GOLD, "mlgwsc_train.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path} ({os.path.getsize(path)} bytes)")


if __name__ == "__main__":
    main()
