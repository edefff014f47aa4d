"""The reference's single-detector efficiency study (``Signal_vs_Noise/Efficiency_test/src``: ``tools.py``, ``train.py``,
``calculate_efficiencies.py``) on the MI355X path: the pieces ``harness/run_efficiency_train.py`` and
``harness/run_efficiency_estimate.py`` are built from.

    ResampledDataset / load_resampled_dataset   <->  tools.py:16-104, 130-177 (index arithmetic, clamps, labels, ``snrs``)
    reg_bce_head              the head, its Softmax and ``reg_BCELoss`` (tools.py:181-191) as ONE autograd Function over the
                              HIP kernels of ``csrc/detect.hip`` (2 launches forward, 2 backward); reads the parameters of
                              the ``nn.Sequential`` ``models.efficiency_classifier`` builds, so ``.pth`` heads load unchanged
    PlateauCLScheduler / ThresholdCLScheduler / EpochCLScheduler   <->  tools.py:195-330
    EvalState                 correct count, sum of the batch losses, row and batch counts in device buffers, read once
    EfficiencyEstimator       <->  tools.py:334-369: scores, rank selection and detection counts stay on the device, ONE
                              read at the end
    remove_softmax            <->  calculate_efficiencies.py:93-106
    efficiency_text / parse_efficiency_text     the ``out_efficiencies_run_*`` file format (calculate_efficiencies.py:83-115)

Deliberate differences from the reference:
  * the SNR of an injected item is still one ``uniform(low, high)`` draw per item, but from a numpy ``Generator`` seeded by
    the dataset's ``seed`` (the reference's ``default_rng()`` is unseeded), drawn in the order of the batch's indices;
  * the waveforms and noises live in HBM at 16 kHz fp32 (the reference keeps them on the host and moves one item at a
    time); they are resampled once at load, in chunks, by the GEMM form of scipy's ``resample``;
  * features are computed per batch on the device (``ops.assemble_batch`` -> ``ops.logmel``), not per item by
    ``WhisperFeatureExtractor`` on the host;
  * the estimator's batch size is a parameter that defaults to 256 (the reference's DataLoader default is 16); the table
    does not depend on it beyond the summation order inside the encoder's kernels, which is per segment;
  * the reference's sorted-array indexing ``noise_outputs[-fac]`` with ``fac == 0`` picks the SMALLEST score; this is
    reproduced, and ``EfficiencyEstimator`` warns when a false-alarm probability truncates to rank 0.
"""

from __future__ import annotations

import fnmatch
import os
import warnings
from typing import Sequence

import numpy as np
import torch
import torch.nn as nn

from . import _lib

__all__ = ["ResampledDataset", "load_resampled_dataset", "synthetic_tensors", "reg_bce_head", "PlateauCLScheduler",
           "ThresholdCLScheduler", "EpochCLScheduler", "EvalState", "EfficiencyEstimator", "LogitDifference",
           "remove_softmax", "false_alarm_ranks", "efficiency_text", "parse_efficiency_text", "snr_ranges", "build_model",
           "LORA_TARGETS"]

# the adapted modules of the reference (train.py:58)
LORA_TARGETS = ("layers.*.self_attn.k_proj", "layers.*.self_attn.v_proj")


# =============================================================================================== data
class ResampledDataset:
    """``tools.py:16-104``: items ``0 .. signal_samples - 1`` are injections ``noise[noise_i] + snr * wave[wave_i]`` with
    label ``[1, 0]``, the rest pure noise with label ``[0, 1]``.  ``waveform_tensor`` [Nw, L] and ``noise_tensor``
    [Nn, L] are fp32 GPU tensors at 16 kHz.  ``plan`` is the reference's ``__getitem__`` arithmetic for a list of indices
    (host, no GPU needed); ``batch`` runs the plan on the device."""

    def __init__(self, waveform_tensor, noise_tensor, snr_range, wave_limits, noise_combined_limits, noise_pure_limits,
                 noises_per_signal: int = 1, seed: int = 0, n_mels: int = 80):
        assert len(wave_limits) == 2 and len(noise_combined_limits) == 2 and len(noise_pure_limits) == 2 and len(snr_range) == 2
        self.wave_tensor, self.noise_tensor = waveform_tensor, noise_tensor
        self.snr_range = snr_range
        self.wave_lim, self.noise_comb_lim, self.noise_pure_lim = wave_limits, noise_combined_limits, noise_pure_limits
        self.noises_per_signal = noises_per_signal
        self.signal_samples = (self.wave_lim[1] - self.wave_lim[0]) * self.noises_per_signal
        assert self.signal_samples == self.noise_comb_lim[1] - self.noise_comb_lim[0]
        self.gen = np.random.default_rng(seed)
        self.n_mels = n_mels
        self._labels = None

    @property
    def device(self):
        return self.noise_tensor.device

    def __len__(self):
        return (self.noise_comb_lim[1] - self.noise_comb_lim[0]) + (self.noise_pure_lim[1] - self.noise_pure_lim[0])

    def snrs(self, *args):
        if len(args) == 0:
            return self.snr_range
        if len(args) == 1:
            self.snr_range = args[0]
        elif len(args) == 2:
            self.snr_range = tuple(args)
        else:
            raise ValueError
        return None

    def plan(self, indices):
        """(noise_i int64 [R], wave_i int64 [R], snr float32 [R], is_wave bool [R]) of the items ``indices``; a pure-noise
        item has wave_i -1 and snr 0.  Draws one SNR per injected item, in the order given."""
        indices = np.asarray(indices, np.int64).reshape(-1)
        n_wave, n_noise = len(self.wave_tensor), len(self.noise_tensor)
        is_wave = indices < self.signal_samples
        wave_i = np.where(is_wave, np.minimum(indices // self.noises_per_signal + self.wave_lim[0], n_wave - 1), -1)
        noise_i = np.minimum(np.where(is_wave, indices + self.noise_comb_lim[0],
                                      indices - self.signal_samples + self.noise_pure_lim[0]), n_noise - 1)
        snr = np.zeros(len(indices), np.float32)
        # (one array draw consumes the generator exactly as that many scalar draws do)
        snr[is_wave] = self.gen.uniform(low=self.snr_range[0], high=self.snr_range[1], size=int(is_wave.sum()))
        return noise_i, wave_i, snr, is_wave

    def assemble(self, plan):
        """[R, L] fp32: ``noise + snr * wave`` per row of the plan (``snr * wave`` rounded to fp32 first, then the sum, as
        torch evaluates the reference's expression); a pure-noise row is the noise row alone."""
        from . import ops
        noise_i, wave_i, snr, _ = plan
        return ops.assemble_batch(self.noise_tensor, self.wave_tensor, noise_i, wave_i, snr)

    def batch(self, indices):
        """(features [R, n_mels, 3000] fp32, targets [R, 2] fp32, plan) on the device."""
        from . import ops
        plan = self.plan(indices)
        if self._labels is None:
            self._labels = torch.tensor([[0.0, 1.0], [1.0, 0.0]], dtype=torch.float32, device=self.device)   # noise, wave
        targets = self._labels[torch.from_numpy(plan[3].astype(np.int64)).to(self.device)]
        return ops.logmel(self.assemble(plan), n_mels=self.n_mels), targets, plan


def _read_rows(path: str, fname: str, n_rows: int) -> np.ndarray:
    """Rows ``[:n_rows]`` of dataset ``data/0``: HDF5 when h5py is importable and the file is not an ``.npz``, otherwise the
    ``.npz`` twin (``<fname>`` or ``<fname>.npz``) with an array named ``data/0``."""
    full = os.path.join(path, fname)
    try:
        import h5py
    except ImportError:
        h5py = None
    if full.endswith(".npz") or h5py is None or not os.path.exists(full):
        twin = full if full.endswith(".npz") else full + ".npz"
        if not os.path.exists(twin):
            raise FileNotFoundError(f"{full}: no such file (and no .npz twin {twin}); h5py "
                                    f"{'is not importable' if h5py is None else 'is present'}")
        with np.load(twin) as z:
            data = z["data/0"][:n_rows]
    else:
        with h5py.File(full, "r") as f:
            data = f["data/0"][:n_rows]
    data = np.asarray(data, np.float32)
    if data.ndim == 3 and data.shape[-1] == 1:       # the reference's waveform files carry a trailing channel axis
        data = data[..., 0]
    if data.ndim != 2:
        raise ValueError(f"{full}: data/0 has shape {data.shape}, expected [n, samples] (or [n, samples, 1])")
    return data


def _resample_to_device(data: np.ndarray, device, chunk: int) -> torch.Tensor:
    """tools.py:107-109 (``len * 16000 // 2048`` output samples) for every row, in chunks, into one fp32 HBM tensor."""
    from . import inference
    n_out = data.shape[1] * 16000 // 2048
    out = torch.empty((len(data), n_out), dtype=torch.float32, device=device)
    for i in range(0, len(data), chunk):
        out[i:i + chunk] = inference.resample(torch.from_numpy(data[i:i + chunk]).to(device), n_out)
    return out


def load_resampled_dataset(path, waveform_fname, noise_fname, snr_range, index_array, device="cuda", chunk: int = 1024,
                           seed: int = 0, n_mels: int = 80) -> ResampledDataset:
    """``tools.py:130-177``: ``index_array = [noises_per_signal, signals, combined_noises, pure_noises]``; reads
    ``data/0[:signals[1]]`` and ``data/0[:max(combined_noises[1], pure_noises[1])]`` at 2048 Hz."""
    device = torch.device(device)
    if device.type != "cuda":
        raise _lib.GwwError(f"load_resampled_dataset: device must be a GPU (got {device}); gw_whisper_amd has no CPU path")
    waves = _read_rows(path, waveform_fname, index_array[1][1])
    noises = _read_rows(path, noise_fname, max(index_array[2][1], index_array[3][1]))
    return ResampledDataset(_resample_to_device(waves, device, chunk), _resample_to_device(noises, device, chunk), snr_range,
                            index_array[1], index_array[2], index_array[3], noises_per_signal=index_array[0], seed=seed,
                            n_mels=n_mels)


def synthetic_tensors(n_wave: int, n_noise: int, seed: int, n_samples: int = 16000):
    """``--synthetic``: (waves [n_wave, n_samples], noises [n_noise, n_samples]) float32 at 16 kHz: unit-variance white
    noise and seeded chirps of unit matched-filter norm against it (so ``snr`` is the optimal SNR of the injection)."""
    from . import synth
    noise = synth.strain_segments(n_noise, seed=seed, n_samples=n_samples)
    rng = np.random.default_rng(seed + 15485863)
    t = np.arange(n_samples, dtype=np.float64) / 16000.0
    wave = np.empty((n_wave, n_samples), np.float32)
    for i in range(n_wave):
        f0, f1 = 30.0 + 40.0 * rng.random(), 200.0 + 600.0 * rng.random()
        tc, dur = 0.55 + 0.3 * rng.random(), 0.1 + 0.2 * rng.random()
        dt = np.minimum(t - tc, 0.0)
        w = np.sin(2 * np.pi * (f1 * dt + 0.5 * (f1 - f0) / dur * dt * dt)) * np.exp(-(dt / dur) ** 2) * (t <= tc)
        wave[i] = (w / np.sqrt((w * w).sum())).astype(np.float32)
    return wave, noise


# =============================================================================================== the HIP head step
def _det_parameters(classifier):
    """The ten ``nn.Linear`` tensors of ``efficiency_classifier.classifier`` (slots 0 2 4 6 8)."""
    from .models import linear_params
    return linear_params(classifier, (0, 2, 4, 6, 8), "the detection head needs the nn.Sequential of "
                         "models.efficiency_classifier (Linear ReLU x 4, Linear, Softmax)")


class _RegBCE(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pooled, targets, epsilon, *params):
        from . import ops
        loss, _logits, probs, _row_loss, saved = ops.det_head_forward(pooled.to(torch.float32), [t.detach() for t in params],
                                                                      targets, epsilon)
        ctx.saved, ctx.in_dtype = saved, pooled.dtype
        ctx.mark_non_differentiable(probs)
        return loss.reshape(()), probs

    @staticmethod
    def backward(ctx, g_loss, _g_probs):
        from . import ops
        dx, grads = ops.det_head_backward(ctx.saved, g_loss.to(torch.float32))
        ctx.saved = None
        return (dx.to(ctx.in_dtype), None, None, *grads)


def reg_bce_head(classifier, pooled: torch.Tensor, targets: torch.Tensor, epsilon: float = 1e-6):
    """``reg_BCELoss(dim=C, epsilon)(classifier(pooled), targets)`` -> (loss, probs) in four HIP launches for forward +
    backward (``csrc/detect.hip``), exact fp32, identical bits on identical calls.  ``classifier`` is the ``nn.Sequential``
    of ``models.efficiency_classifier``; its parameters receive their gradients through autograd as usual, ``pooled``
    [B, d_model] its own.  The probabilities are returned for metrics and carry no gradient."""
    if not pooled.is_cuda or not targets.is_cuda:
        raise _lib.GwwError("reg_bce_head needs GPU tensors: gw_whisper_amd has no CPU path")
    return _RegBCE.apply(pooled, targets.to(torch.float32), float(epsilon), *_det_parameters(classifier))


class EvalState:
    """Validation state kept on the device: ``add`` is one launch per batch and never synchronises, ``read`` copies the
    four buffers to the host once."""

    def __init__(self, device):
        self.correct = torch.zeros((1,), dtype=torch.int64, device=device)
        self.loss_sum = torch.zeros((1,), dtype=torch.float64, device=device)
        self.n = torch.zeros((1,), dtype=torch.int64, device=device)
        self.batches = torch.zeros((1,), dtype=torch.int64, device=device)

    def add(self, probs, targets, row_loss):
        from . import ops
        ops.det_eval_accumulate(probs, targets, row_loss, self.correct, self.loss_sum, self.n, self.batches)

    def read(self):
        """(valid_loss = sum of the batch losses / batches, valid_accuracy = correct / rows, rows, batches) as
        train.py:150-151 forms them."""
        c, s, n, b = int(self.correct.item()), float(self.loss_sum.item()), int(self.n.item()), int(self.batches.item())
        return s / max(b, 1), c / max(n, 1), n, b


# =============================================================================================== curriculum learning
def snr_ranges(initial, final, steps: int):
    """scheduler_pars.py:9-11: ``steps + 1`` ranges from ``initial`` to ``final``, both ends linearly."""
    lower = np.linspace(initial[0], final[0], steps + 1)
    upper = np.linspace(initial[1], final[1], steps + 1)
    return list(zip(lower, upper))


class CurriculumLearningScheduler:
    """tools.py:195-228.  ``optim``: reloaded with its state at construction on every range change."""

    def __init__(self, snr_ranges, datasets, verbose=True, optim=None):
        self.snr_ranges, self.datasets, self.verbose = snr_ranges, datasets, verbose
        self.done = False
        self.interrupt = False
        self.reload_optimizer = optim is not None
        if self.reload_optimizer:
            self.optim = optim
            self.optim_init_state_dict = self.optim.state_dict()
        self.snr_iter = iter(self.snr_ranges)
        self.next_range = next(self.snr_iter)
        self.set_next_range()

    def set_next_range(self):
        old_range = None
        for dataset in self.datasets:
            old_range = dataset.snrs()
            dataset.snrs(self.next_range)
        self.output_info(old_range, self.next_range)
        try:
            self.next_range = next(self.snr_iter)
        except StopIteration:
            self.done = True
        if self.reload_optimizer:
            self.optim.load_state_dict(self.optim_init_state_dict)

    def output_info(self, old_range, new_range):
        if self.verbose:
            print("# Reducing SNR range from %f-%f to %f-%f" % (old_range[0], old_range[1], new_range[0], new_range[1]))


class PlateauCLScheduler(CurriculumLearningScheduler):
    """tools.py:232-285: steps when the metric has not improved for more than ``patience`` epochs."""

    def __init__(self, *args, patience=4, threshold=1.e-4, threshold_mode="rel", optimization_mode="min", metric_index=0,
                 allow_interrupt=False, **kwargs):
        super().__init__(*args, **kwargs)
        self.patience, self.threshold, self.threshold_mode = patience, threshold, threshold_mode
        self.optimization_mode, self.metric_index, self.allow_interrupt = optimization_mode, metric_index, allow_interrupt
        self.best = None
        self.num_bad_epochs = None

    def is_better(self, a):
        if self.best is None:
            return True
        if self.threshold_mode not in ("rel", "abs") or self.optimization_mode not in ("min", "max"):
            raise NotImplementedError
        sign = -1.0 if self.optimization_mode == "min" else 1.0
        bound = self.best * (1.0 + sign * self.threshold) if self.threshold_mode == "rel" else self.best + sign * self.threshold
        return a < bound if self.optimization_mode == "min" else a > bound

    def step(self, *args):
        current = float(args[self.metric_index])
        if self.is_better(current):
            self.best = current
            self.num_bad_epochs = 0
        else:
            self.num_bad_epochs += 1
        if self.num_bad_epochs > self.patience:
            if self.done:
                if self.allow_interrupt:
                    self.interrupt = True
            else:
                self.set_next_range()
                self.best = None
                self.num_bad_epochs = None


class ThresholdCLScheduler(CurriculumLearningScheduler):
    """tools.py:289-312: steps when the metric is at least as good as ``threshold``."""

    def __init__(self, *args, threshold=0.2, optimization_mode="min", metric_index=0, **kwargs):
        super().__init__(*args, **kwargs)
        self.threshold, self.optimization_mode, self.metric_index = threshold, optimization_mode, metric_index

    def is_better(self, a):
        if self.optimization_mode == "min":
            return a <= self.threshold
        if self.optimization_mode == "max":
            return a >= self.threshold
        raise NotImplementedError

    def step(self, *args):
        if self.is_better(float(args[self.metric_index])) and not self.done:
            self.set_next_range()


class EpochCLScheduler(CurriculumLearningScheduler):
    """tools.py:316-330: steps after more than ``patience`` epochs on one range."""

    def __init__(self, *args, patience=4, **kwargs):
        super().__init__(*args, **kwargs)
        self.patience = patience
        self.num_epochs = 0

    def step(self, *args):
        self.num_epochs += 1
        if self.num_epochs > self.patience and not self.done:
            self.num_epochs = 0
            self.set_next_range()


# =============================================================================================== efficiencies
class LogitDifference(nn.Linear):
    """The layer calculate_efficiencies.py:94-95 puts in the Softmax's place: ``Linear(2, 2, bias=False)`` with the frozen
    weight ``[[1, -1], [-1, 1]]``; column 0 of its output is ``z0 - z1``."""

    def __init__(self):
        super().__init__(2, 2, bias=False)
        self.weight = nn.Parameter(torch.tensor([[1.0, -1.0], [-1.0, 1.0]]), requires_grad=False)


def remove_softmax(model):
    """calculate_efficiencies.py:93-106: the trailing Softmax of ``model.classifier`` replaced by ``LogitDifference``."""
    layers = list(model.classifier.children())
    if not isinstance(layers[-1], nn.Softmax):
        raise ValueError("The last layer of the classifier is not a Softmax layer.")
    dev = next(model.classifier.parameters()).device
    layers[-1] = LogitDifference().to(dev)
    model.classifier = nn.Sequential(*layers)
    return model


def false_alarm_ranks(faps, n_noise: int) -> np.ndarray:
    """tools.py:353, with exactly that expression: its truncation is part of the result."""
    return (np.array(faps) * n_noise).astype(int)


class EfficiencyEstimator:
    """tools.py:334-369.  ``__call__(network)`` -> float64 [len(snrs), len(faps)]: the fraction of the wave dataset's
    injections at each SNR whose score exceeds (strictly) the noise score of rank ``int(fap * len(noise_dataset))`` from
    the top.  The score is ``network``'s column 0: ``probs[:, 0]``, or ``z0 - z1`` after ``remove_softmax``.  All scores,
    the thresholds and the counts stay on the device; the host reads the [S, F] count table once."""

    def __init__(self, wave_dataset, noise_dataset, snrs, batch_size: int = 256, faps=(1.e-2, 1.e-3, 1.e-4)):
        self.snrs, self.wave_dataset, self.noise_dataset = snrs, wave_dataset, noise_dataset
        self.batch_size, self.faps = int(batch_size), faps

    def _scores(self, network, params, mode, dataset, out, want_wave):
        from . import ops
        from .models import _pooled
        for i in range(0, len(dataset), self.batch_size):
            idx = np.arange(i, min(i + self.batch_size, len(dataset)))
            mel, _targets, plan = dataset.batch(idx)
            assert bool(plan[3].all()) if want_wave else not bool(plan[3].any())     # tools.py:348 / :363
            ops.det_head_scores(_pooled(network.encoder, mel).to(torch.float32), params, out[i:i + len(idx)], mode)

    def __call__(self, network):
        from . import ops
        last = list(network.classifier.children())[-1]
        if isinstance(last, nn.Softmax):
            mode = ops.SCORE_PROB0
        elif isinstance(last, LogitDifference):
            mode = ops.SCORE_LOGIT_DIFF
        else:
            raise _lib.GwwError("EfficiencyEstimator: the classifier must end in Softmax or in remove_softmax's layer")
        params = [t.detach() for t in _det_parameters(network.classifier)]
        dev, n_noise, n_wave = self.noise_dataset.device, len(self.noise_dataset), len(self.wave_dataset)
        ranks = false_alarm_ranks(self.faps, n_noise)
        if (ranks < 0).any() or (ranks > n_noise).any():
            raise ValueError(f"false-alarm probabilities {self.faps} give ranks {ranks.tolist()} outside 0..{n_noise}")
        if (ranks == 0).any():
            warnings.warn(f"false-alarm probabilities {[f for f, r in zip(self.faps, ranks) if r == 0]} truncate to rank 0 of "
                          f"{n_noise} noise samples: the threshold is the SMALLEST noise score, as in the reference")
        with torch.no_grad():
            scores = torch.empty((n_noise,), dtype=torch.float32, device=dev)
            self.noise_dataset.snrs((0., 0.))
            self._scores(network, params, mode, self.noise_dataset, scores, False)
            ranks_d = torch.from_numpy(ranks.astype(np.int64)).to(dev)
            groups = [slice(i, min(i + ops.MAX_FAPS, len(ranks))) for i in range(0, len(ranks), ops.MAX_FAPS)]
            thr = [ops.score_thresholds(scores, ranks_d[g]) for g in groups]
            counts = [torch.zeros((len(self.snrs), g.stop - g.start), dtype=torch.int64, device=dev) for g in groups]
            wave_scores = torch.empty((n_wave,), dtype=torch.float32, device=dev)
            for s, snr in enumerate(self.snrs):
                self.wave_dataset.snrs((snr, snr))
                self._scores(network, params, mode, self.wave_dataset, wave_scores, True)
                for t, c in zip(thr, counts):
                    ops.detection_counts(wave_scores, t, c[s])
            table = torch.cat(counts, dim=1).cpu().numpy()
        self.thresholds = torch.cat(thr)          # device; for inspection
        return table / n_wave


def efficiency_text(faps: Sequence[float], snrs: Sequence[float], table) -> str:
    """The text of ``out_efficiencies_run_%04i_epoch_%04i.txt`` (calculate_efficiencies.py:84-114)."""
    out = "# FAPs: %f" % faps[0] + "".join("    %f" % f for f in faps[1:]) + "\n"
    for snr, effs in zip(snrs, table):
        out += "%f" % snr + "".join("    %f" % num for num in effs) + "\n"
    return out


def parse_efficiency_text(text: str):
    """(faps, snrs, table) of such a file."""
    lines = text.splitlines()
    if not lines or not lines[0].startswith("# FAPs:"):
        raise ValueError("not an efficiency file: the first line must start with '# FAPs:'")
    faps = [float(x) for x in lines[0][len("# FAPs:"):].split()]
    rows = [[float(x) for x in l.split()] for l in lines[1:] if l.strip()]
    return faps, [r[0] for r in rows], np.asarray([r[1:] for r in rows], np.float64)


# =============================================================================================== model
def build_model(encoder_name: str = "tiny", num_classes: int = 2, lora_rank: int = 8, lora_alpha: int = 32,
                precision: str = "bf16", encoder_weights: str = None, seed: int = 0, device="cuda", adapter_path: str = None):
    """train.py:52-76, 91 / calculate_efficiencies.py:65-78: encoder -> fnmatch search for ``k_proj`` / ``v_proj`` ->
    ``LoraConfig(use_dora=True, r, lora_alpha)`` -> ``get_peft_model`` (or ``PeftModel.from_pretrained(adapter_path)``) ->
    ``requires_grad = 'lora' in name`` -> ``efficiency_classifier``."""
    from . import synth
    from .encoder import WhisperConfig, WhisperEncoder
    from .models import efficiency_classifier
    from .peft import LoraConfig, PeftModel, get_peft_model
    d, L, H, F = synth.ENCODER_SIZES[encoder_name]
    config = WhisperConfig.named(encoder_name)
    encoder = WhisperEncoder(config, precision=precision)
    if encoder_weights:
        if encoder_weights.endswith(".safetensors"):
            from safetensors.torch import load_file
            encoder.load_state_dict(load_file(encoder_weights))
        else:
            encoder.load_state_dict(torch.load(encoder_weights, map_location="cpu"))
    else:
        sd = synth.encoder_state_dict(d, L, H, F, seed=seed, n_mels=config.num_mel_bins)
        encoder.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    if adapter_path:
        body = PeftModel.from_pretrained(encoder, adapter_path).to(device)
    else:
        names = [n for n, _ in encoder.named_modules()]
        matched = [m for pat in LORA_TARGETS for m in fnmatch.filter(names, pat)]
        body = get_peft_model(encoder, LoraConfig(use_dora=True, r=lora_rank, lora_alpha=lora_alpha,
                                                  target_modules=matched)).to(device)
        for name, p in body.named_parameters():
            p.requires_grad = "lora" in name
    return efficiency_classifier(body, num_classes=num_classes).to(device)
