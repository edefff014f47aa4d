#!/usr/bin/env python3
"""Counterpart of the reference's ``MLGWSC-1/train.py`` on the MI355X path: it trains the Q-transform search model that
``harness/run_inference.py --adapter-weights --lora-weights --dense-weights`` runs.

Same flags and defaults (``parse_args``, ``train.py:780-827``), same sequence (``main``, ``:829-937``): datasets from every
file of ``--dataset-dir`` (groups ``training`` / ``validation`` with ``noises [N, D, T]`` and ``waveforms [M, D, T]``),
the Q-transform adapter (``QTransformAdapter.train_variant``), whisper encoder with LoRA (DoRA with ``--use-dora``) on
q / k / v / out_proj, optional InfoNCE pretraining (``--pretrain-steps 0`` skips it) whose adapter and encoder are saved
to ``q_adapter_pretrained.pt`` / ``encoder_pretrained.pt`` and reloaded, then supervised fine-tuning with the reference's
artefacts under ``-o``: ``losses.txt``, ``last.pt``, ``state_dict_e_XXXX.pt``, ``best_state_dict.pt``,
``best_adapter.pt``, ``best_lora_weights/``, ``best_dense_layers.pth``.

Differences:
  * batches are built on the device from seeded plans (``mlgwsc_train.DeviceBatches``: the same generator calls per item as
    the reference's ``__getitem__``, one ``--seed``-derived generator per loader), not by per-item DataLoader workers; the
    arrays go to the device once (``--store-device`` is where they are read into first);
  * the validation SNRs are redrawn from a generator re-seeded every epoch, so validation losses are comparable across
    epochs;
  * ``last.pt`` records the best validation loss AFTER that epoch's comparison; the reference records the value before
    it, so a resume can overwrite a better ``best_state_dict.pt``;
  * ``torch.autograd.set_detect_anomaly`` is not replicated;
  * ``--num-workers`` / ``--pin-memory`` are accepted and ignored;
  * files are HDF5 when ``h5py`` is importable; otherwise each file's ``.npz`` twin with arrays ``training/noises``,
    ``training/waveforms``, ``validation/noises``, ``validation/waveforms``;
  * extras as in the other harnesses: ``--synthetic N`` (N seeded noise segments and N/2 seeded chirps ``[., D, 2048]``
    for training, a quarter of that for validation, instead of ``--dataset-dir``), ``--encoder`` (default tiny) and
    ``--encoder-weights`` (a HF WhisperEncoder ``state_dict``, .pth / .safetensors; otherwise seeded random weights --
    ``openai/whisper-tiny`` cannot be downloaded here);
  * one process, one GPU: ``WORLD_SIZE > 1`` is refused (InfoNCE across ranks needs gathered negatives).
"""
from __future__ import annotations

import logging
import os
import sys
from argparse import ArgumentParser

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402


def build_parser() -> ArgumentParser:
    parser = ArgumentParser(description="GW-Whisper (Q-Scan) training script (MI355X)")
    # Logging & reproducibility
    parser.add_argument("--verbose", action="store_true", help="Print info logs.")
    parser.add_argument("--debug", action="store_true", help="Enable debug logs.")
    parser.add_argument("--force", action="store_true", help="Overwrite existing outputs.")
    parser.add_argument("--seed", type=int, default=42, help="Random seed.")
    parser.add_argument("--deterministic", action="store_true", help="Deterministic torch backend.")
    # Data
    parser.add_argument("-d", "--dataset-dir", type=str, required=True, help="Directory with HDF5 (or .npz) dataset files.")
    parser.add_argument("--n-detectors", type=int, default=2, help="Number of detectors (channels).")
    parser.add_argument("--sample-rate", type=int, default=2048, help="Input sample rate.")
    parser.add_argument("--spectrogram-shape", type=int, nargs=2, default=[128, 128], help="Q-Scan base (F, T) shape.")
    parser.add_argument("--target-shape", type=int, nargs=2, default=[80, 3000], help="Pooled (F*, T*) shape.")
    parser.add_argument("--q-range", type=int, nargs=2, default=[4, 128], help="Q-Transform range.")
    parser.add_argument("--kernel-length", type=float, default=1.0, help="Q-Transform kernel/window length (s).")
    # Training
    parser.add_argument("-o", "--output-training", type=str, required=True, help="Output directory.")
    parser.add_argument("--snr", type=float, nargs=2, default=(5.0, 15.0), help="Uniform SNR range for injections.")
    parser.add_argument("--learning-rate", type=float, default=1e-5, help="Fine-tune learning rate.")
    parser.add_argument("--epochs", type=int, default=50, help="Fine-tune epochs.")
    parser.add_argument("--batch-size", type=int, default=128, help="Batch size.")
    parser.add_argument("--clip-norm", type=float, default=100.0, help="Gradient clipping norm.")
    parser.add_argument("--num-workers", type=int, default=2, help="Accepted for compatibility; batches are built on the GPU.")
    parser.add_argument("--pin-memory", action="store_true", help="Accepted for compatibility; batches are built on the GPU.")
    parser.add_argument("--early-stop-patience", type=int, default=10, help="Epochs of no improvement to stop.")
    parser.add_argument("--num-classes", type=int, default=2, help="Classifier output size (default 2).")
    parser.add_argument("--resume", nargs="?", const="latest", default=None, choices=["latest", "best"],
                        help="Resume training: 'latest' or 'best'. If flag given without value => 'latest'.")
    # Devices
    parser.add_argument("--train-device", type=str, default="cuda", help="Device for training ('cuda', 'cuda:1').")
    parser.add_argument("--store-device", type=str, default="cpu", help="Device the datasets are read into first.")
    # Pretraining
    parser.add_argument("--pretrain-steps", type=int, default=60000, help="Contrastive pretraining steps (0 to skip).")
    parser.add_argument("--pretrain-lr", type=float, default=1e-4, help="Pretraining learning rate.")
    parser.add_argument("--pretrain-temp", type=float, default=0.1, help="InfoNCE temperature.")
    parser.add_argument("--noise-only-prob", type=float, default=0.25, help="Probability of a noise-only pair.")
    # PEFT (LoRA/DoRA)
    parser.add_argument("--lora-rank", type=int, default=8, help="LoRA rank.")
    parser.add_argument("--lora-alpha", type=int, default=32, help="LoRA alpha.")
    parser.add_argument("--use-dora", action="store_true", help="Enable DoRA variant for LoRA.")
    # extras of this port
    parser.add_argument("--synthetic", type=int, default=0, help="Use N seeded synthetic segments instead of --dataset-dir.")
    parser.add_argument("--encoder", type=str, default="tiny", help="Whisper encoder size (tiny, base, small, ...).")
    parser.add_argument("--encoder-weights", type=str, default=None, help="HF WhisperEncoder state_dict (.pth / .safetensors).")
    return parser


def parse_args(argv=None):
    return build_parser().parse_args(argv)


# ---------------------------------------------------------------------------------------------- data
def _have_h5py() -> bool:
    try:
        import h5py  # noqa: F401
        return True
    except ImportError:
        return False


def read_dataset_dir(dataset_dir: str) -> list:
    """[(path, {"training": (noises, waveforms), "validation": (noises, waveforms)})] for every file of the directory
    (``load_concat_datasets``, MLGWSC-1/train.py:744-773), in name order: HDF5 through h5py when it is importable,
    otherwise the ``.npz`` twin of each file."""
    names = sorted(f for f in os.listdir(dataset_dir) if os.path.isfile(os.path.join(dataset_dir, f)))
    h5 = _have_h5py()
    stems_with_h5 = {os.path.splitext(f)[0] for f in names if not f.endswith(".npz")}
    out = []
    for f in names:
        path = os.path.join(dataset_dir, f)
        if f.endswith(".npz"):
            if h5 and os.path.splitext(f)[0] in stems_with_h5:
                continue                                   # its HDF5 original is read instead
            z = np.load(path)
            out.append((path, {g: (z[f"{g}/noises"], z[f"{g}/waveforms"]) for g in ("training", "validation")}))
        elif h5:
            import h5py
            with h5py.File(path, "r") as hf:
                out.append((path, {g: (hf[g]["noises"][()], hf[g]["waveforms"][()]) for g in ("training", "validation")}))
        elif os.path.splitext(f)[0] + ".npz" not in names:
            raise RuntimeError(f"{path}: h5py is not importable here and the file has no .npz twin")
    if not out:
        raise RuntimeError(f"no dataset files in {dataset_dir}")
    return out


def synthetic_arrays(n: int, n_detectors: int, seed: int, n_samples: int = 2048):
    """n seeded white-noise segments and n // 2 seeded chirps, [., D, n_samples] fp32 (unit-variance noise, unit-peak
    chirps: --snr scales them as the reference scales its waveforms)."""
    rng = np.random.default_rng(seed)
    noises = rng.standard_normal((n, n_detectors, n_samples)).astype(np.float32)
    t = np.arange(n_samples, dtype=np.float64) / n_samples
    waves = np.zeros((max(1, n // 2), n_detectors, n_samples), np.float32)
    for i in range(len(waves)):
        f0, tc = 30.0 + 40.0 * rng.random(), 0.5 + 0.3 * rng.random()
        s = np.sin(2 * np.pi * (f0 + 120.0 * t) * t) * np.exp(-((t - tc) / 0.1) ** 2)
        waves[i] = (0.1 * s / np.abs(s).max()).astype(np.float32)
    return noises, waves


def load_data(args):
    from gw_whisper_amd.mlgwsc_train import BinaryGWDataset
    if args.synthetic:
        n = int(args.synthetic)
        files = [("synthetic", {"training": synthetic_arrays(n, args.n_detectors, args.seed),
                                "validation": synthetic_arrays(max(4, n // 4), args.n_detectors, args.seed + 1)})]
    else:
        files = read_dataset_dir(args.dataset_dir)
    train, valid = [], []
    for path, groups in files:
        logging.info(f"Loading datasets from {path}")
        for g, dst in (("training", train), ("validation", valid)):
            noises, waves = groups[g]
            dst.append(BinaryGWDataset(noises, waves, store_device=args.store_device, train_device=args.train_device,
                                       snr_range=tuple(args.snr)))
    return train, valid


# ---------------------------------------------------------------------------------------------- model
def build_encoder(args):
    import torch
    from gw_whisper_amd import synth
    from gw_whisper_amd.encoder import WhisperConfig, WhisperEncoder
    config = WhisperConfig.named(args.encoder)
    if args.encoder_weights:
        if args.encoder_weights.endswith(".safetensors"):
            from safetensors.torch import load_file
            sd = load_file(args.encoder_weights)
        else:
            sd = torch.load(args.encoder_weights, map_location="cpu")
        enc = WhisperEncoder(config, precision="bf16")
        enc.load_state_dict(sd)
        return enc
    return WhisperEncoder.from_numpy_state_dict(synth.named_encoder_state_dict(args.encoder, seed=args.seed), config,
                                                precision="bf16")


def check_before_gpu(args) -> None:
    """The refusals that must come before any device is touched."""
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world > 1:
        raise SystemExit(f"run_mlgwsc_train: WORLD_SIZE={world}: this program trains on one GPU (InfoNCE across ranks "
                         "needs gathered negatives); launch it without torchrun")
    losses = os.path.join(args.output_training, "losses.txt")
    if os.path.isfile(losses) and not args.force:
        raise RuntimeError(f"Output file exists: {losses} (use --force)")


def main(argv=None) -> int:
    args = parse_args(argv)
    level = logging.DEBUG if args.debug else (logging.INFO if args.verbose else logging.WARN)
    logging.basicConfig(format="%(levelname)s | %(asctime)s: %(message)s", level=level, datefmt="%d-%m-%Y %H:%M:%S")
    check_before_gpu(args)

    import torch
    from gw_whisper_amd import mlgwsc_train as mt
    from gw_whisper_amd.qscan import QTransformAdapter
    if not torch.cuda.is_available():
        raise SystemExit("run_mlgwsc_train: no GPU -- gw_whisper_amd has no CPU fallback")
    device = torch.device(args.train_device)
    if device.type != "cuda":
        raise SystemExit(f"run_mlgwsc_train: --train-device {args.train_device}: gw_whisper_amd trains on the GPU only")
    if device.index is not None:
        torch.cuda.set_device(device)
    np.random.seed(args.seed)                                        # set_seed (train.py:51-65)
    torch.manual_seed(args.seed)
    torch.cuda.manual_seed_all(args.seed)
    if args.deterministic:
        torch.backends.cudnn.deterministic = True
        torch.backends.cudnn.benchmark = False

    train_list, valid_list = load_data(args)
    train_data = mt.ConcatGWData(train_list, device)
    valid_data = mt.ConcatGWData(valid_list, device)
    logging.info("Datasets loaded.")
    train_dl = mt.DeviceBatches(train_data, args.batch_size, shuffle=True, seed=args.seed + 1)
    valid_dl = mt.DeviceBatches(valid_data, max(32, args.batch_size), shuffle=False, seed=args.seed + 2, reseed=True)

    q_adapter = QTransformAdapter(kernel_length=args.kernel_length, sample_rate=args.sample_rate, q_range=list(args.q_range),
                                  spectrogram_shape=list(args.spectrogram_shape), target_shape=tuple(args.target_shape),
                                  n_detectors=args.n_detectors, channels=QTransformAdapter.TRAIN_CHANNELS)   # train.py:647-655
    logging.info("Q-Transform adapter ready.")
    encoder = mt.apply_lora(build_encoder(args), r=args.lora_rank, alpha=args.lora_alpha, use_dora=args.use_dora).to(device)
    logging.info("Whisper encoder (PEFT) ready.")
    network = mt.build_network(encoder, q_adapter, args.n_detectors, args.num_classes, device)
    os.makedirs(args.output_training, exist_ok=True)

    if args.pretrain_steps > 0:
        logging.info("Starting contrastive pretraining...")
        pre_ds = mt.PretrainDataset(train_data.noises, train_data.waveforms, snr_range=tuple(args.snr),
                                    noise_only_prob=args.noise_only_prob, device=device)
        pre_dl = mt.DeviceBatches(pre_ds, min(128, args.batch_size), shuffle=True, seed=args.seed + 3)
        pretrainer = mt.ContrastivePretrainer(network.adapter, network.encoder, network.adapter.n_detectors, device=device,
                                              proj_dim=256, lr=args.pretrain_lr, temperature=args.pretrain_temp)
        pretrainer.train(pre_dl, steps=args.pretrain_steps)
        pre_adapter_path = os.path.join(args.output_training, "q_adapter_pretrained.pt")
        pre_encoder_path = os.path.join(args.output_training, "encoder_pretrained.pt")
        torch.save(network.adapter.state_dict(), pre_adapter_path)
        torch.save(network.encoder.state_dict(), pre_encoder_path)
        logging.info("Saved pretraining weights.")
        network.adapter.load_state_dict(torch.load(pre_adapter_path, map_location=device))
        network.encoder.load_state_dict(torch.load(pre_encoder_path, map_location=device))
        logging.info("Reloaded pretraining weights.")

    trainer = mt.SupervisedTrainer(network, device=device, lr=args.learning_rate, clip_norm=args.clip_norm,
                                   loss_fn=mt.RegBCELoss(dim=args.num_classes))
    trainer.fit(train_dl, valid_dl, outdir=args.output_training, epochs=args.epochs, resume=args.resume, force=args.force,
                early_stop_patience=args.early_stop_patience)
    return 0


if __name__ == "__main__":
    sys.exit(main())
