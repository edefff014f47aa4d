#!/usr/bin/env python3
"""Counterpart of the reference's ``Signal_vs_Noise/run_train.py`` + ``src/train.py`` on the MI355X path.

Same flags (``run_train.py:9-25``), same construction sequence (``src/train.py:227-277``: encoder -> fnmatch target
search -> ``LoraConfig(use_dora=True)`` -> ``get_peft_model`` -> ``requires_grad = 'lora' in name`` ->
``two_channel_ligo_binary_classifier`` -> ``BCEWithLogitsLoss`` + ``AdamW(lr, betas=(0.9, 0.999), eps=1e-8)``), same
loop (``:139-211``: train epoch, validation loss + ROC AUC, best-by-val-loss checkpoint, early stopping with
patience 15) and the same artefacts (``<models-path>/[best_]lora_weights_<r>_<alpha>/adapter_config.json +
adapter_model.safetensors``, ``[best_]dense_layers_<r>_<alpha>.pth``).

Differences that come with the hardware path:
  * log-mel features are computed on the GPU per batch (``ops.logmel``) from the 16 kHz waveforms, not per item in
    DataLoader workers (``src/dataset.py:15-26``);
  * ``--data-path`` is a HuggingFace ``datasets`` directory with the reference's columns (``h1_timeseries``,
    ``l1_timeseries``, ``labels``, ``injection_snr``; ``utils/preprocess.py:111-132``) or, with ``--synthetic N``,
    N seeded noise segments of which half carry a chirp (there is no network for real data);
  * pretrained ``openai/whisper-*`` weights cannot be downloaded here: ``--encoder-weights`` takes a HF encoder
    ``state_dict`` (.pth / .safetensors), otherwise seeded random weights;
  * scalars go to ``<log-dir>/train_log.jsonl`` (TensorBoard is not installed);
  * under ``torchrun`` every rank trains on its shard of each epoch and the trainable gradients are all-reduced
    in ONE flat bucket (RCCL).
``--method DoRA`` (the reference default), ``--method LoRA`` and ``--method full_finetune`` have a HIP backward.
``--head cnn`` trains ``TwoChannelLIGOBinaryClassifierCNN`` (``src/model.py:57-85``) instead of the MLP head, for all three
methods; the ``[best_]dense_layers`` artefact is then the CNN's ``classifier.state_dict()``.
``full_finetune`` follows ``src/train.py:243-247``: no adapters, ``requires_grad = True`` on every encoder and head
parameter (``embed_positions`` included), AdamW over them, and the encoder saved by ``WhisperEncoder.save_pretrained``
(``config.json`` + ``model.safetensors``, HF key names) under the reference's ``[best_]lora_weights_<r>_<alpha>`` name;
``--encoder-weights <dir>/model.safetensors`` loads it back.
``--detectors 1`` is the reference's single-detector twin ``src/sd_train.py``: ``l1_timeseries`` only
(``one_channel_LigoBinaryData``, ``src/dataset.py:28-46``; with ``--synthetic`` the L1 half), the head of
``one_channel_ligo_binary_classifier`` (d -> 512 -> 256 -> 128 -> 64 -> 1, ``src/model.py:31-52``), the same loop, artefact
names and resume flags, for all three methods.  It has no CNN decoder: ``--detectors 1 --head cnn`` is refused.
``--head-step hip`` runs the MLP head's forward, ``BCEWithLogitsLoss`` and backward as one HIP step
(``gw_whisper_amd.binary.head_bce_with_logits``, csrc/binary_head.hip: exact fp32, four launches) and takes the host
synchronisations out of the loop: the step losses stay device tensors and are read once per epoch, validation goes through
``binary.head_logits`` + ``roc.BinaryEvalState`` with one host read per pass.  Its validation loss is the reference's (sum of
the batch means) / (number of batches) (``src/train.py:91,105``, ``sd_train.py:91,105``); the default ``--head-step torch``
branch weights every batch mean by its number of samples, so the two differ whenever the last validation batch is short.
``--head-step hip --head cnn`` is refused (the CNN decoder has its own HIP chain).
"""
import argparse
import fnmatch
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402


class EarlyStopper:   # src/train.py:27-43
    def __init__(self, patience=1, min_delta=0.0):
        self.patience, self.min_delta, self.counter, self.min_validation_loss = patience, min_delta, 0, float("inf")

    def early_stop(self, validation_loss):
        if validation_loss < self.min_validation_loss:
            self.min_validation_loss, self.counter = validation_loss, 0
        elif validation_loss > (self.min_validation_loss + self.min_delta):
            self.counter += 1
            if self.counter >= self.patience:
                return True
        return False


# the adapted modules of the reference (src/train.py:232; o_proj matches nothing in HF Whisper)
DEFAULT_LORA_TARGETS = ("layers.*.self_attn.q_proj", "layers.*.self_attn.k_proj", "layers.*.self_attn.v_proj",
                        "layers.*.self_attn.o_proj")


def synthetic_dataset(n, seed, rate=16000):
    """n two-detector 1 s segments at ``rate`` Hz (16 kHz by default), unit-variance noise; odd indices carry the same
    chirp in both."""
    from gw_whisper_amd import synth
    h1 = synth.strain_segments(n, seed=seed, n_samples=rate)
    l1 = synth.strain_segments(n, seed=seed + 1, n_samples=rate)
    t = np.arange(rate, dtype=np.float32) / np.float32(rate)
    labels = np.zeros(n, np.float32)
    rng = np.random.default_rng(seed + 2)
    for i in range(1, n, 2):
        f0, tc = 40.0 + 60.0 * rng.random(), 0.45 + 0.3 * rng.random()
        s = 4.0 * np.sin(2 * np.pi * (f0 + 220.0 * t) * t) * np.exp(-((t - tc) / 0.12) ** 2)
        h1[i] += s.astype(np.float32)
        l1[i] += s.astype(np.float32)
        labels[i] = 1.0
    return h1, l1, labels, np.where(labels > 0, 12.0, 0.0).astype(np.float32)


def load_arrays(args):
    """(h1, l1, labels, snr); h1 is None with --detectors 1 on a dataset directory (sd_train.py never reads it)."""
    if args.synthetic:
        return synthetic_dataset(args.synthetic, args.seed, getattr(args, "sampling_rate", 16000))
    from datasets import concatenate_datasets, load_from_disk
    path = args.data_path
    chunks = sorted(p for p in os.listdir(path) if p.startswith("chunk")) if os.path.isdir(path) else []
    ds = concatenate_datasets([load_from_disk(os.path.join(path, c)) for c in chunks]) if chunks else load_from_disk(path)
    cols = ds.with_format("numpy")
    single = getattr(args, "detectors", 2) == 1
    return (None if single else np.asarray(cols["h1_timeseries"], np.float32), np.asarray(cols["l1_timeseries"], np.float32),
            np.asarray(cols["labels"], np.float32), np.asarray(cols["injection_snr"], np.float32))


def check_args(args):
    """The flag combinations that name no model of the reference."""
    if args.detectors == 1 and args.head == "cnn":
        raise ValueError("--detectors 1 --head cnn: the single-detector trainer (src/sd_train.py) has the MLP head only; the "
                         "CNN decoder stacks the pooled tokens of two detectors")
    if args.head_step == "hip" and args.head == "cnn":
        raise ValueError("--head-step hip --head cnn: the HIP step is the MLP heads' (csrc/binary_head.hip); the CNN decoder "
                         "already runs its own HIP chain")


FRONTEND_DEFAULTS = {"sampling_rate": 16000, "n_fft": 400, "hop_length": 160, "chunk_length": 30, "mel_fmax": 8000.0}


def frontend_plan(args, n_mels=80):
    """(extractor keyword arguments, max_source_positions) of the front-end flags, or (None, 1500) when all of them are
    Whisper's: the run then builds, computes and writes exactly what it did before the flags existed.  The encoder's
    context is ``chunk_length * sampling_rate // hop_length // 2``; an odd frame count is refused (conv2 halves it), the
    rest of the supported set is the extractor's to check."""
    got = {k: getattr(args, k, v) for k, v in FRONTEND_DEFAULTS.items()}
    if all(float(got[k]) == float(v) for k, v in FRONTEND_DEFAULTS.items()):
        return None, 1500
    frames = got["chunk_length"] * got["sampling_rate"] // got["hop_length"] if got["hop_length"] > 0 else 0
    if frames % 2:
        raise ValueError(f"--chunk-length {got['chunk_length']} --sampling-rate {got['sampling_rate']} --hop-length "
                         f"{got['hop_length']}: {frames} frames, an odd count; the encoder's stride-2 conv needs an even one")
    kw = dict(feature_size=n_mels, sampling_rate=got["sampling_rate"], hop_length=got["hop_length"],
              chunk_length=got["chunk_length"], n_fft=got["n_fft"], min_frequency=0.0, max_frequency=float(got["mel_fmax"]))
    return kw, frames // 2


def main(args):
    check_args(args)
    from gw_whisper_amd import binary, dist as gdist, ops, roc, synth
    from gw_whisper_amd.encoder import WhisperConfig, WhisperEncoder
    from gw_whisper_amd.feature_extraction import WhisperFeatureExtractor
    from gw_whisper_amd.models import (TwoChannelLIGOBinaryClassifierCNN, one_channel_ligo_binary_classifier,
                                       two_channel_ligo_binary_classifier)
    from gw_whisper_amd.peft import LoraConfig, get_peft_model
    rank, world, local = gdist.init()
    assert torch.cuda.is_available(), "run_train.py needs an MI355X (gw_whisper_amd has no CPU path)"
    torch.cuda.set_device(local)
    device = torch.device("cuda", local)
    torch.manual_seed(args.seed)

    h1, l1, labels, snr = load_arrays(args)
    n = len(labels)
    perm = np.random.default_rng(args.seed).permutation(n)           # train_test_split(test_size, seed, shuffle=True)
    n_val = int(round(n * args.test_size))
    val_idx, train_idx = perm[:n_val], perm[n_val:]

    d, L, H, F = synth.ENCODER_SIZES[args.encoder]
    config = WhisperConfig.named(args.encoder)
    # src/dataset.py:12 -- the extractor of the same size: 128 mel bins for large-v3 / large-v3-turbo, 80 otherwise
    n_mels = WhisperFeatureExtractor.from_pretrained(f"openai/whisper-{args.encoder}").feature_size
    assert n_mels == config.num_mel_bins
    # the front-end flags: a configured extractor and an encoder of the matching context (a longer position table of
    # --encoder-weights, or of the seeded weights, is cut to its first rows by load_state_dict, as with_context does)
    fe_kw, context = frontend_plan(args, n_mels)
    extractor, fe_config = None, None
    if fe_kw is not None:
        import dataclasses
        extractor = WhisperFeatureExtractor(**fe_kw)
        fe_config = extractor.frontend_config
        config = dataclasses.replace(config, max_source_positions=context)
    encoder = WhisperEncoder(config, precision=args.precision)
    if args.encoder_weights:
        if args.encoder_weights.endswith(".safetensors"):
            from safetensors.torch import load_file
            encoder.load_state_dict(load_file(args.encoder_weights))
        else:
            encoder.load_state_dict(torch.load(args.encoder_weights, map_location="cpu"))
    else:
        sd = synth.encoder_state_dict(d, L, H, F, seed=args.seed, n_mels=n_mels)
        encoder.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    module_names = [name for name, _ in encoder.named_modules()]
    patterns = args.lora_targets
    matched = [m for p in patterns for m in fnmatch.filter(module_names, p)]
    if args.method not in ("DoRA", "LoRA", "full_finetune"):
        raise ValueError(f"--method {args.method}: expected DoRA, LoRA or full_finetune")
    if args.method == "full_finetune":
        # src/train.py:243-247: the bare encoder, every parameter trainable (embed_positions included); the HIP
        # base-weight backward is an explicit opt-in of the encoder
        if args.load_model_path:
            raise ValueError("--load_model_path resumes an adapter; a fully fine-tuned encoder is loaded with "
                             "--encoder-weights <dir>/model.safetensors")
        peft = encoder.enable_full_finetune().to(device)
    elif args.load_model_path:
        # resume (src/train.py:44-60): the saved adapter is loaded onto the BARE encoder -- PeftModel.from_pretrained
        # wraps the nn.Linear targets itself -- and stays trainable
        from gw_whisper_amd.peft import PeftModel
        adapter_dir = _resume_path(args.load_model_path, args.load_lora_weights)
        with open(os.path.join(adapter_dir, "adapter_config.json")) as f:
            saved_dora = bool(json.load(f).get("use_dora", False))
        if saved_dora != (args.method == "DoRA"):
            raise ValueError(f"--method {args.method} but the adapter in {adapter_dir} was saved with use_dora={saved_dora}: "
                             "resume with the method it was trained with")
        peft = PeftModel.from_pretrained(encoder, adapter_dir, is_trainable=True).to(device)
    else:
        peft = get_peft_model(encoder, LoraConfig(use_dora=args.method == "DoRA", r=args.lora_rank,   # src/train.py:253, :263
                                                  lora_alpha=args.lora_alpha, target_modules=matched)).to(device)
    if args.method != "full_finetune":
        for name, p in peft.named_parameters():
            p.requires_grad = "lora" in name
    # src/train.py:23 imports both decoders; --head cnn builds the second one (its HIP chain, forward and backward)
    if args.detectors == 1:        # sd_train.py:23, :275
        model = one_channel_ligo_binary_classifier(peft).to(device)
    else:
        model = (TwoChannelLIGOBinaryClassifierCNN(peft) if args.head == "cnn" else two_channel_ligo_binary_classifier(peft)).to(device)
    if args.method == "full_finetune":
        for p in model.parameters():   # src/train.py:246-247
            p.requires_grad = True
    if args.load_model_path:
        model.classifier.load_state_dict(torch.load(_resume_path(args.load_model_path, args.load_dense_weights),
                                                    map_location=device))
    params = [p for p in model.parameters() if p.requires_grad]
    optimizer = torch.optim.AdamW(params, lr=args.learning_rate, betas=(0.9, 0.999), eps=1e-08)
    bucket = gdist.FlatGradBucket(params)
    criterion = torch.nn.BCEWithLogitsLoss().to(device)
    tag = f"{args.lora_rank}_{args.lora_alpha}"
    os.makedirs(args.models_path, exist_ok=True)
    os.makedirs(args.log_dir, exist_ok=True)
    log = open(os.path.join(args.log_dir, "train_log.jsonl"), "a") if rank == 0 else None

    def features(idx):
        if args.detectors == 1:    # one_channel_LigoBinaryData: the L1 strain alone
            return (ops.logmel(torch.from_numpy(l1[idx]).to(device), n_mels=n_mels, config=fe_config),)
        w = torch.from_numpy(np.concatenate((h1[idx], l1[idx]))).to(device)
        mel = ops.logmel(w, n_mels=n_mels, config=fe_config)
        return mel[: len(idx)], mel[len(idx):]

    def evaluate_hip():
        """The validation pass without a host read per batch: the state lives on the device, ``read`` is the one copy."""
        model.eval()
        state = roc.BinaryEvalState(max(len(val_idx), 1), device, with_snr=False)
        with torch.no_grad():
            for i in range(0, len(val_idx), args.batch_size):
                idx = val_idx[i:i + args.batch_size]
                state.add(binary.head_logits(model.classifier, model.pooled(*features(idx))),
                          torch.from_numpy(labels[idx]).to(device))
        r = state.read()
        auc = float("nan")
        if len(set(r["labels"].tolist())) > 1:
            from sklearn.metrics import roc_auc_score
            auc = float(roc_auc_score(r["labels"], r["scores"]))
        return r["loss"], auc

    def evaluate():
        if args.head_step == "hip":
            return evaluate_hip()
        model.eval()
        tot, cnt, probs, ys = 0.0, 0, [], []
        with torch.no_grad():
            for i in range(0, len(val_idx), args.batch_size):
                idx = val_idx[i:i + args.batch_size]
                out = model(*features(idx))
                y = torch.from_numpy(labels[idx]).view(-1, 1).to(device)
                tot += criterion(out, y).item() * len(idx)
                cnt += len(idx)
                probs.append(torch.sigmoid(out).flatten().cpu().numpy())
                ys.append(labels[idx])
        auc = float("nan")
        if cnt and len(set(np.concatenate(ys).tolist())) > 1:
            from sklearn.metrics import roc_auc_score
            auc = float(roc_auc_score(np.concatenate(ys), np.concatenate(probs)))
        return tot / max(cnt, 1), auc

    def save(prefix):
        if rank != 0:
            return
        out_dir = os.path.join(args.models_path, f"{prefix}lora_weights_{tag}")
        model.encoder.save_pretrained(out_dir)
        if extractor is not None:
            # a non-default front end travels with the model: run_evaluation.py reads both files
            extractor.save_pretrained(out_dir)
            with open(os.path.join(out_dir, "config.json"), "w") as f:
                json.dump(encoder.config_dict(), f, indent=2, sort_keys=True)
        torch.save(model.classifier.state_dict(), os.path.join(args.models_path, f"{prefix}dense_layers_{tag}.pth"))

    stopper, best = EarlyStopper(patience=15), float("inf")
    for epoch in range(args.num_epochs):
        model.train()
        order = np.random.default_rng(args.seed + 1 + epoch).permutation(train_idx)
        t0, run, nb, seen, step_losses = time.time(), 0.0, 0, 0, []
        # every rank runs the SAME number of steps (one all-reduce each); the bucket takes the SAMPLE-weighted mean over
        # the ranks (a rank without a batch in the last step contributes zero samples), i.e. the gradient of the mean loss
        # over the whole global batch whatever the number of ranks
        for step in range(gdist.epoch_steps(len(order), world, args.batch_size)):
            sl = gdist.step_slice(len(order), step, rank, world, args.batch_size)
            bucket.zero()
            if sl is not None:
                idx = order[sl[0]:sl[1]]
                y = torch.from_numpy(labels[idx]).view(-1, 1).to(device)
                if args.head_step == "hip":
                    loss, _ = binary.head_bce_with_logits(model.classifier, model.pooled(*features(idx)), y)
                    loss.backward()
                    step_losses.append(loss.detach())
                else:
                    loss = criterion(model(*features(idx)), y)
                    loss.backward()
                    run += loss.item()
                nb += 1
                seen += len(idx)
            bucket.all_reduce_mean(world, n_local=0 if sl is None else sl[1] - sl[0])
            optimizer.step()
        if step_losses:            # the epoch's one read of the step losses (summed in fp64, as the host sum of .item()s is)
            run = float(torch.stack(step_losses).double().sum())
        train_loss = run / max(nb, 1)
        val_loss, val_auc = evaluate()
        val_loss = gdist.broadcast_scalar(val_loss, world, device)     # one decision for all ranks
        rec = {"epoch": epoch + 1, "train_loss": train_loss, "val_loss": val_loss, "val_auc": val_auc,
               "epoch_s": time.time() - t0, "segments_per_s": len(order) / max(time.time() - t0, 1e-9), "rank0_segments": seen}
        if rank == 0:
            print(f"Epoch {epoch + 1}/{args.num_epochs}, Train Loss: {train_loss:.4f}, Val Loss: {val_loss:.4f}, "
                  f"Val AUC: {val_auc:.4f}")
            log.write(json.dumps(rec) + "\n")
            log.flush()
        if val_loss < best:
            best = val_loss
            save("best_")
        if stopper.early_stop(val_loss):
            if rank == 0:
                print(f"Early stopping at epoch {epoch + 1}")
            break
    save("")
    if world > 1:
        torch.distributed.barrier()
        torch.distributed.destroy_process_group()


def _resume_path(base: str, name: str) -> str:
    """The reference builds resume paths by plain string concatenation, ``load_model_path + load_lora_weights``
    (Signal_vs_Noise/src/train.py:292): that form first, ``os.path.join`` (a base directory without the trailing
    separator) second; whichever exists."""
    for cand in (base + name, os.path.join(base, name)):
        if os.path.exists(cand):
            return cand
    raise FileNotFoundError(f"neither {base + name!r} nor {os.path.join(base, name)!r} exists")


def build_parser():
    parser = argparse.ArgumentParser(description="Training pipeline for the LIGO binary classification model (MI355X path)")
    parser.add_argument("--data-path", type=str, default="Detection/data/Whisper_train_mass-8to100_resampled_train")
    parser.add_argument("--models-path", type=str, default="Detection/results/Two_detectors/models")
    parser.add_argument("--figures-path", type=str, default="Detection/results/Two_detectors/figures")
    parser.add_argument("--log-dir", type=str, default="Detection/results/Two_detectors/logs")
    parser.add_argument("--load_model_path", type=str, default=None)
    parser.add_argument("--load_lora_weights", type=str, default=None)
    parser.add_argument("--load_dense_weights", type=str, default=None)
    parser.add_argument("--batch-size", type=int, default=32)
    parser.add_argument("--num-epochs", type=int, default=1)
    parser.add_argument("--learning-rate", type=float, default=1e-4)
    parser.add_argument("--test-size", type=float, default=0.2)
    parser.add_argument("--encoder", type=str, default="tiny")
    parser.add_argument("--seed", type=int, default=42)
    parser.add_argument("--num-workers", type=int, default=12, help="accepted for compatibility; features are computed on the GPU")
    parser.add_argument("--method", type=str, default="DoRA")
    parser.add_argument("--lora-rank", type=int, default=8)
    parser.add_argument("--lora-alpha", type=int, default=32)
    parser.add_argument("--lora-targets", type=str, nargs="+", default=list(DEFAULT_LORA_TARGETS), metavar="PATTERN",
                        help="fnmatch patterns of the encoder modules to adapt (e.g. 'layers.*.fc1'); a resumed adapter "
                             "keeps the targets it was saved with")
    parser.add_argument("--synthetic", type=int, default=0, help="use N seeded synthetic segments instead of --data-path")
    parser.add_argument("--encoder-weights", type=str, default=None, help="HF WhisperEncoder state_dict (.pth / .safetensors)")
    # the front end (defaults: Whisper's); any other value builds a WhisperFeatureExtractor of that configuration and an
    # encoder of max_source_positions = chunk_length * sampling_rate // hop_length // 2
    parser.add_argument("--sampling-rate", type=int, default=FRONTEND_DEFAULTS["sampling_rate"], help="Hz of the strain segments")
    parser.add_argument("--n-fft", type=int, default=FRONTEND_DEFAULTS["n_fft"])
    parser.add_argument("--hop-length", type=int, default=FRONTEND_DEFAULTS["hop_length"])
    parser.add_argument("--chunk-length", type=int, default=FRONTEND_DEFAULTS["chunk_length"], help="seconds a segment is padded to")
    parser.add_argument("--mel-fmax", type=float, default=FRONTEND_DEFAULTS["mel_fmax"],
                        help="upper edge of the mel filterbank in Hz (HF fixes 8000; pass sampling_rate / 2 for strain)")
    parser.add_argument("--precision", choices=("bf16", "fp32"), default="bf16",
                        help="encoder arithmetic: bf16 (default) or exact fp32, the reference's own training arithmetic "
                             "(DoRA / LoRA only: full fine-tuning is bf16)")
    parser.add_argument("--head", choices=("mlp", "cnn"), default="mlp",
                        help="the decoder: two_channel_ligo_binary_classifier's MLP (default) or "
                             "TwoChannelLIGOBinaryClassifierCNN, whose best_dense_layers artefact is the CNN's state_dict")
    parser.add_argument("--detectors", type=int, choices=(2, 1), default=2,
                        help="2: src/train.py (H1 + L1, two_channel_ligo_binary_classifier, the default); 1: src/sd_train.py "
                             "(L1 only, one_channel_ligo_binary_classifier)")
    parser.add_argument("--head-step", choices=("torch", "hip"), default="torch",
                        help="the MLP head's forward + BCEWithLogitsLoss + backward: torch.nn (default) or one HIP step with a "
                             "sync-free loop around it (validation loss: sum of batch means / batches)")
    return parser


if __name__ == "__main__":
    main(build_parser().parse_args())
