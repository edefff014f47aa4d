"""Signal-vs-noise evaluation (the reference's ``Signal_vs_Noise/src/evaluation.py``) on the device: the state of one
evaluation pass, and the ROC curve, its AUC and the bootstrap band of the TPR at a grid of FPRs (``evaluation.py:110-122``).

The arithmetic is integer counting plus a few fp64 divisions, so the device results equal sklearn's / numpy's bit for bit
(DESIGN.md section 22).  One sort of the scores serves every resample: a resample is a vector of multiplicities over the
sorted order.  The resample indices come from the host stream the reference draws from (``sklearn.utils.resample`` =
``RandomState.randint(0, n, size=n)`` per replicate), so a seed reproduces the reference's resamples."""

from __future__ import annotations

import numpy as np
import torch

from . import ops
from ._lib import GwwError


class BinaryEvalState:
    """The state of one evaluation pass over ``n`` items, kept on the device: ``add`` is one launch (plus the copies of the
    labels and SNRs into their buffers) and never synchronises, ``read`` is the one host read."""

    def __init__(self, n: int, device, with_snr: bool = True):
        if n < 1:
            raise GwwError(f"BinaryEvalState: n={n} must be >= 1")
        self.n, self.filled = int(n), 0
        self.scores = torch.zeros((n,), dtype=torch.float32, device=device)
        self.labels = torch.zeros((n,), dtype=torch.float32, device=device)
        self.snr = torch.zeros((n,), dtype=torch.float32, device=device) if with_snr else None
        self.loss_sum = torch.zeros((1,), dtype=torch.float64, device=device)
        self.batches = torch.zeros((1,), dtype=torch.int64, device=device)
        self.confusion = torch.zeros((2, 2), dtype=torch.int64, device=device)

    def add(self, logits, labels, snr=None):
        labels = labels.reshape(-1).to(torch.float32)
        B = labels.numel()
        if self.filled + B > self.n:
            raise GwwError(f"BinaryEvalState: {self.filled} + {B} items exceed the {self.n} the state was built for")
        ops.binary_eval_accumulate(logits, labels, self.scores, self.filled, self.loss_sum, self.batches, self.confusion)
        self.labels[self.filled:self.filled + B].copy_(labels)
        if snr is not None and self.snr is not None:
            self.snr[self.filled:self.filled + B].copy_(snr.reshape(-1))
        self.filled += B

    def read(self):
        """dict: loss (the sum of the batch losses / batches, ``evaluation.py:66``), confusion [2, 2] int64 (rows = the
        label), scores, labels, snr (numpy, the filled part), batches."""
        m = self.filled
        b = int(self.batches.item())
        return {"loss": float(self.loss_sum.item()) / max(b, 1), "batches": b, "confusion": self.confusion.cpu().numpy(),
                "scores": self.scores[:m].cpu().numpy(), "labels": self.labels[:m].cpu().numpy(),
                "snr": None if self.snr is None else self.snr[:m].cpu().numpy()}


def drop_collinear(fps, tps):
    """sklearn's ``drop_intermediate`` rule on the vertex counts (leading (0, 0) included): of the vertices behind the
    origin, keep the first, the last and every one where the second difference of fps or of tps is non-zero."""
    fps, tps = np.asarray(fps), np.asarray(tps)
    f, t = fps[1:], tps[1:]
    if len(f) <= 2:
        return fps, tps
    keep = np.ones(len(f), bool)
    keep[1:-1] = (np.diff(f, 2) != 0) | (np.diff(t, 2) != 0)
    sel = np.concatenate(([0], 1 + np.flatnonzero(keep)))
    return fps[sel], tps[sel]


class RocEvaluator:
    """``ev(scores, labels)`` -> dict with ``fpr``, ``tpr`` (``roc_curve``), ``auc`` (``roc_auc_score``), ``grid``,
    ``mean_tpr``, ``std_tpr`` (``bootstrap_roc_curve``), ``n_valid`` (the replicates that hold both classes; the band is
    taken over those) and ``n_nan``.  ``chunk_bytes`` bounds the device memory of one chunk of replicates (indices +
    workspace); the result does not depend on it."""

    def __init__(self, num_bootstrap: int = 1000, grid=None, seed=None, chunk_bytes: int = 1 << 30):
        self.num_bootstrap = int(num_bootstrap)
        self.grid = np.logspace(-4, 0, num=500) if grid is None else np.ascontiguousarray(grid, np.float64)
        if self.grid.ndim != 1 or not 1 <= self.grid.size <= ops.ROC_MAX_Q:
            raise GwwError(f"RocEvaluator: grid must be [Q] with 1 <= Q <= {ops.ROC_MAX_Q}")
        if not (np.all(np.diff(self.grid) >= 0) and self.grid[0] > 0 and self.grid[-1] <= 1):
            raise GwwError("RocEvaluator: grid must be ascending in (0, 1]")
        if self.num_bootstrap < 1:
            raise GwwError("RocEvaluator: num_bootstrap must be >= 1")
        self.seed, self.chunk_bytes = seed, int(chunk_bytes)

    def chunk_rows(self, n: int) -> int:
        return int(max(1, min(self.num_bootstrap, 65535, self.chunk_bytes // (12 * n))))

    def __call__(self, scores, labels, indices=None, drop_intermediate: bool = True):
        if not torch.is_tensor(scores):
            scores = torch.from_numpy(np.ascontiguousarray(np.asarray(scores, np.float32).reshape(-1))).cuda()
        if not torch.is_tensor(labels):
            labels = torch.from_numpy(np.ascontiguousarray(np.asarray(labels, np.float32).reshape(-1))).to(scores.device)
        scores, labels = scores.reshape(-1), labels.reshape(-1).to(torch.float32)
        n, dev = scores.numel(), scores.device
        order, rank, pos, gend, G, n_nan = ops.roc_sort(scores, labels)
        fps, tps, fpr, tpr, counts, auc = ops.roc_curve(pos, gend, G)
        g, nn = int(G.item()), int(n_nan.item())
        P, Nneg = (int(v) for v in counts.cpu().numpy())
        if nn > 0:
            raise GwwError(f"RocEvaluator: {nn} of the {n} scores are NaN")
        if P == 0 or Nneg == 0:
            raise GwwError(f"RocEvaluator: the labels hold one class only ({P} positive, {Nneg} negative)")
        if indices is not None:
            indices = np.asarray(indices)
            if indices.ndim != 2 or indices.shape[1] != n or indices.shape[0] < 1:
                raise GwwError(f"RocEvaluator: indices must be [R, N = {n}]")
            if indices.min() < 0 or indices.max() >= n:
                raise GwwError(f"RocEvaluator: indices must lie in 0..{n - 1}")
            R = indices.shape[0]
        else:
            R = self.num_bootstrap
            rs = np.random.RandomState(self.seed)
        grid = torch.from_numpy(self.grid).to(dev)
        rows, valids = [], []
        step = self.chunk_rows(n)
        for r0 in range(0, R, step):
            rc = min(step, R - r0)
            if indices is not None:
                host = np.ascontiguousarray(indices[r0:r0 + rc], np.int32)
            else:
                host = np.stack([rs.randint(0, n, size=n) for _ in range(rc)]).astype(np.int32)
            t, v = ops.roc_bootstrap_tpr(rank, pos, gend, G, torch.from_numpy(host).to(dev), grid)
            rows.append(t)
            valids.append(v)
        mean, std, n_valid = ops.roc_band(torch.cat(rows), torch.cat(valids))
        f, t = fps[:g + 1].cpu().numpy(), tps[:g + 1].cpu().numpy()
        if drop_intermediate:
            f, t = drop_collinear(f, t)
            out_fpr, out_tpr = f / np.float64(Nneg), t / np.float64(P)
        else:
            out_fpr, out_tpr = fpr[:g + 1].cpu().numpy(), tpr[:g + 1].cpu().numpy()
        return {"fpr": out_fpr, "tpr": out_tpr, "auc": float(auc.item()), "grid": self.grid.copy(),
                "mean_tpr": mean.cpu().numpy(), "std_tpr": std.cpu().numpy(), "n_valid": int(n_valid.item()), "n_nan": nn}
