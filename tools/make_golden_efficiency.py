#!/usr/bin/env python3
"""Writes tests/golden/efficiency.npz, efficiency_traces.json and efficiency_format.txt: what the efficiency-study tests
compare against (CPU only).  Usage: make_golden_efficiency.py REFERENCE_ROOT

The reference's ``Signal_vs_Noise/Efficiency_test/src/network.py`` and ``tools.py`` are loaded by path (an empty stub
module stands in for ``h5py``, which ``tools.py`` imports and these pieces never call).

  head        the reference's head class (network.py:69-90) and ``reg_BCELoss(dim=C, epsilon=1e-6)`` (tools.py:181-191) in
              fp64 on seeded pooled tokens and one-hot targets for the (d_in, C, B) of efficiency_helpers.CASES: logits,
              probs and loss in full, every gradient as a digest (its Frobenius norm and eight seeded sign projections;
              the fp64 gradients of the seven cases would not fit a committed file).  Weights and inputs are regenerated
              by the tests from the stored seeds.  ASSERTED for every stored case: every hidden pre-activation is at least
              2e-6 from zero (no fp32 implementation then opens a ReLU the fp64 one keeps shut); the input seed is the
              first for which that holds.
  plans       ``BaseDataset.__getitem__``'s index arithmetic (wave_i, noise_i, label) for several index arrays, among
              them ``noises_per_signal = 2`` and limits beyond the tensors' ends (the clamped tail), recorded through a
              stand-in feature extractor that returns the assembled sample itself
  traces      for all three scheduler classes: the ranges set on the datasets and the ``done`` / ``interrupt`` flags after
              construction and after every ``step`` of a recorded metric sequence
  estimator   ``EfficiencyEstimator`` on a tiny dataset with a stand-in network (a fixed linear score), among its FAPs one
              whose rank truncates to 0: the noise scores, the wave scores per SNR and the table
  format      a copy of the reference's shipped ``efficiencies/out_efficiencies_run_0000_epoch_0025.txt``
"""
import importlib.util
import json
import os
import shutil
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import efficiency_helpers as eh  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")


def load_reference(ref_root):
    src = os.path.join(ref_root, "Signal_vs_Noise", "Efficiency_test", "src")
    sys.modules.setdefault("h5py", types.ModuleType("h5py"))
    mods = []
    for name in ("network", "tools"):
        spec = importlib.util.spec_from_file_location(f"efficiency_ref_{name}", os.path.join(src, f"{name}.py"))
        m = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(m)
        mods.append(m)
    return mods[0], mods[1], src


class _Enc(torch.nn.Module):      # what the reference's class reads from its encoder: config.d_model
    def __init__(self, d):
        super().__init__()
        self.config = type("Cfg", (), {"d_model": d})()


def run_head(net, tools, d_in, C, x, t, params):
    model = net.one_channel_ligo_binary_classifier(_Enc(d_in), num_classes=C)
    model.classifier.load_state_dict({k: torch.from_numpy(v) for k, v in zip(eh.PARAM_KEYS, params)})
    model = model.double()
    xt = torch.from_numpy(x).double().requires_grad_(True)
    h, margin = xt, np.inf
    for i, m in enumerate(model.classifier):
        h = m(h)
        if isinstance(m, torch.nn.Linear) and i != 8:
            margin = min(margin, float(h.detach().abs().min()))
        if i == 8:
            logits = h.detach().numpy()
    loss = tools.reg_BCELoss(dim=C, epsilon=eh.EPSILON)(h, torch.from_numpy(t).double())
    loss.backward()
    grads = [model.classifier.state_dict(keep_vars=True)[k].grad.numpy() for k in eh.PARAM_KEYS]
    return logits, h.detach().numpy(), float(loss.detach()), xt.grad.numpy(), grads, margin


def make_head(net, tools, out):
    out["head_cases"] = np.asarray(eh.CASES, np.int64)
    seeds = []
    for ci, (d_in, C, B) in enumerate(eh.CASES):
        params = eh.case_params(ci, d_in, C)
        for seed in range(9000 + 10000 * ci, 9000 + 10000 * ci + 5000):
            x, t = eh.case_inputs(d_in, C, B, seed)
            logits, probs, loss, dx, grads, margin = run_head(net, tools, d_in, C, x, t, params)
            if margin >= 2e-6:
                break
        else:
            raise AssertionError(f"case {ci}: no seed with the required ReLU margin")
        assert margin >= 2e-6
        seeds.append(seed)
        print(f"case {ci} (d_in {d_in}, C {C}, B {B}): seed {seed}, ReLU margin {margin:.3e}, max|logit| "
              f"{np.abs(logits).max():.3f}, loss {loss:.6f}")
        out[f"head{ci}_logits"], out[f"head{ci}_probs"], out[f"head{ci}_loss"] = logits, probs, np.float64(loss)
        out[f"head{ci}_dx"] = eh.digest(dx, 0)
        for k, g in enumerate(grads):
            out[f"head{ci}_grad{k}"] = eh.digest(g, 1 + k)
        out[f"head{ci}_margin"] = np.float64(margin)
    out["head_seeds"] = np.asarray(seeds, np.int64)


class _Echo:       # stand-in feature extractor: the "features" are the assembled sample itself
    def __call__(self, sample, sampling_rate=None, return_tensors=None):
        return types.SimpleNamespace(input_features=torch.as_tensor(np.asarray(sample))[None])


# (n_wave rows, n_noise rows, [noises_per_signal, signals, combined_noises, pure_noises])
PLAN_CASES = (
    (6, 20, [1, [0, 6], [0, 6], [6, 14]]),
    (5, 24, [2, [1, 5], [3, 11], [11, 24]]),
    (4, 9, [2, [0, 6], [0, 12], [8, 14]]),          # limits beyond both tensors: the clamped tail
    (3, 7, [1, [0, 0], [0, 0], [0, 7]]),            # the estimator's noise dataset
    (3, 7, [3, [0, 2], [1, 7], [0, 0]]),            # the estimator's wave dataset
)


def make_plans(tools, out):
    for pi, (n_wave, n_noise, ia) in enumerate(PLAN_CASES):
        wave = torch.zeros(n_wave, 2)
        wave[:, 0] = torch.arange(1, n_wave + 1)
        noise = torch.zeros(n_noise, 2)
        noise[:, 1] = torch.arange(1, n_noise + 1)
        ds = tools.ResampledDataset(wave, noise, (1.0, 1.0), ia[1], ia[2], ia[3], _Echo(), noises_per_signal=ia[0])
        rows = []
        for i in range(len(ds)):
            feat, label = ds[i]
            rows.append([int(feat[0]) - 1, int(feat[1]) - 1, int(label[0])])        # wave_i (-1: pure noise), noise_i, is_wave
        out[f"plan{pi}"] = np.asarray(rows, np.int64).reshape(-1, 3)
        out[f"plan{pi}_len"] = np.int64(len(ds))
    out["plan_cases"] = np.asarray(json.dumps([list(c) for c in PLAN_CASES]))


class _DS:
    def __init__(self):
        self.r = (100.0, 200.0)

    def snrs(self, *a):
        if not a:
            return self.r
        self.r = a[0]


TRACE_RANGES = [(20.0, 30.0), (15.0, 25.0), (10.0, 20.0), (5.0, 15.0)]
TRACE_CASES = (
    ("PlateauCLScheduler", {"patience": 1}, [[1.0, .5], [.9, .5], [.95, .5], [.96, .6], [.5, .6], [.6, .6], [.7, .6], [.4, .7],
                                              [.5, .7], [.6, .7], [.3, .7], [.3, .7], [.3, .7], [.3, .7]]),
    ("PlateauCLScheduler", {"patience": 0, "allow_interrupt": True, "threshold": 0.1, "threshold_mode": "abs",
                            "optimization_mode": "max", "metric_index": 1},
     [[1.0, .5], [1.0, .55], [1.0, .7], [1.0, .7], [1.0, .9], [1.0, .1], [1.0, .2], [1.0, .25], [1.0, .5], [1.0, .5]]),
    ("ThresholdCLScheduler", {"threshold": 0.3}, [[.5, 0], [.3, 0], [.31, 0], [.2, 0], [.1, 0], [.1, 0], [.4, 0]]),
    ("ThresholdCLScheduler", {"threshold": 0.8, "optimization_mode": "max", "metric_index": 1},
     [[0, .5], [0, .8], [0, .79], [0, .9], [0, .95], [0, .99]]),
    ("EpochCLScheduler", {"patience": 2}, [[0, 0]] * 12),
    ("EpochCLScheduler", {"patience": 0}, [[0, 0]] * 5),
)


def make_traces(tools):
    traces = []
    for cls, kwargs, metrics in TRACE_CASES:
        dss = (_DS(), _DS())
        lin = torch.nn.Linear(2, 2)
        opt = torch.optim.Adam(lin.parameters(), lr=1e-3)
        sched = getattr(tools, cls)(TRACE_RANGES, dss, verbose=False, optim=opt, **kwargs)
        states = [[list(dss[0].snrs()), list(dss[1].snrs()), bool(sched.done), bool(sched.interrupt)]]
        for m in metrics:
            sched.step(*m)
            states.append([list(dss[0].snrs()), list(dss[1].snrs()), bool(sched.done), bool(sched.interrupt)])
        traces.append({"class": cls, "kwargs": kwargs, "ranges": [list(r) for r in TRACE_RANGES], "metrics": metrics,
                       "states": states})
    return traces


def make_estimator(tools, out):
    rng = np.random.default_rng(4242)
    L, n_wave, n_noise = 16, 12, 57
    wave = torch.from_numpy((rng.standard_normal((n_wave, L)) * 0.2 + 0.3).astype(np.float32))
    noise = torch.from_numpy(rng.standard_normal((n_noise + n_wave, L)).astype(np.float32))
    proj = torch.from_numpy(rng.standard_normal(L).astype(np.float32))
    wave_ds = tools.ResampledDataset(wave, noise, (0., 0.), (0, n_wave), (n_noise, n_noise + n_wave), (0, 0), _Echo(), bool=True)
    noise_ds = tools.ResampledDataset(wave, noise, (0., 0.), (0, 0), (0, 0), (0, n_noise), _Echo(), bool=True)
    seen = []

    def network(x):
        s = x.to(torch.float32) @ proj
        seen.append(s.clone())
        return torch.stack((s, -s), dim=1)
    snrs, faps = [0.0, 0.5, 1.0, 2.0, 4.0], (0.5, 0.1, 0.05, 0.01)      # 0.01 * 57 truncates to rank 0
    table = tools.EfficiencyEstimator(wave_ds, noise_ds, snrs, batch_size=5, faps=faps)(network)
    scores = torch.cat(seen).numpy()
    out["est_wave"], out["est_noise"], out["est_proj"] = wave.numpy(), noise.numpy(), proj.numpy()
    out["est_snrs"], out["est_faps"] = np.asarray(snrs), np.asarray(faps)
    out["est_noise_scores"] = scores[:n_noise]
    out["est_wave_scores"] = scores[n_noise:].reshape(len(snrs), n_wave)
    out["est_table"] = np.asarray(table, np.float64)
    assert (np.asarray(faps) * n_noise).astype(int).tolist() == [28, 5, 2, 0]
    print("estimator table\n", table)


if __name__ == "__main__":
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    net, tools, src = load_reference(sys.argv[1])
    os.makedirs(GOLD, exist_ok=True)
    out = {}
    make_head(net, tools, out)
    make_plans(tools, out)
    make_estimator(tools, out)
    path = os.path.join(GOLD, "efficiency.npz")
    np.savez_compressed(path, **out)
    print("efficiency.npz", os.path.getsize(path), "bytes")
    with open(os.path.join(GOLD, "efficiency_traces.json"), "w") as f:
        json.dump(make_traces(tools), f, indent=1)
    shutil.copyfile(os.path.join(src, "efficiencies", "out_efficiencies_run_0000_epoch_0025.txt"),
                    os.path.join(GOLD, "efficiency_format.txt"))
