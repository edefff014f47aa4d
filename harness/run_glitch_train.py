#!/usr/bin/env python3
"""Counterpart of the reference's ``Glitch_classification/src/train.py`` (DoRA / LoRA) and
``src/train_full_finetune.py`` (``--method full_finetune``) on the MI355X path.

Same flags (``train.py:203-216``, underscores as there), same construction sequence (``train.py:144-189``: label
transformation -> label encoder fitted on train + test labels -> encoder -> fnmatch target search ->
``LoraConfig(use_dora=...)`` -> ``get_peft_model`` -> ``requires_grad = 'lora' in name`` -> the multi-class head ->
``CrossEntropyLoss`` + ``AdamW(model.parameters(), lr)`` with torch's default betas / eps / weight decay), same loop
(``:88-135``: shuffled training batches with the last partial batch kept, ``train_loss`` and ``val_loss`` the mean of the
per-batch mean losses, validation in dataset order, macro F1, best-by-``val_loss`` checkpoint, early stopping with
patience 60) and the same artefacts: ``<results_path>/<model_name>_best_lora_weights.pth``
(``torch.save(model.encoder.state_dict())``: the whole ``PeftModel`` state dict under peft's runtime key names),
``<model_name>_best_dense_weights.pth`` (keys ``0 3 6 9``); full fine-tuning: ``<model_name>_best_whisper_weights.pth``
(the bare encoder's HF-keyed state dict, ``train_full_finetune.py:123``).

Differences that come with the hardware path:
  * log-mel features are computed on the GPU per batch (``ops.logmel``) from the 16 kHz waveforms, not per item in
    DataLoader workers (``src/dataset.py:46``);
  * ``--head hip`` (default) runs the head, the loss and their backward as four HIP launches
    (``glitch.head_cross_entropy``) and reads the losses once per epoch; its dropout mask is a counter-based function of
    (``--seed``, step, layer, element), not torch's.  ``--head torch`` is the reference's ``nn.Sequential`` +
    ``CrossEntropyLoss`` with ``loss.item()`` per batch;
  * pretrained ``openai/whisper-*`` weights cannot be downloaded here: ``--encoder-weights`` takes a HF encoder
    ``state_dict`` (.pth / .safetensors), otherwise seeded random weights; ``--synthetic N`` replaces the two datasets
    by N seeded training segments (and N // 4 test segments) of ``--synthetic-classes`` burst classes;
  * scalars go to ``<log_dir>/train_log.jsonl`` (TensorBoard is not installed); in place of the confusion-matrix PNG:
    ``<model_name>_best_confusion_matrix.npy`` (int64 counts, rows = true class) and ``<model_name>_classes.json``;
  * under ``torchrun`` every rank trains on its shard of each epoch and the trainable gradients are all-reduced in ONE
    flat bucket (RCCL); every rank validates the whole test set, rank 0 writes.
Two deliberate differences from the reference's arithmetic:
  (a) the reference's ``evaluate`` (``train.py:56-62``) never calls ``model.eval()``, so after the first
      ``model.train()`` its validation runs with Dropout active; here validation runs in eval mode, so that ``val_loss``,
      the checkpoint choice and early stopping do not depend on a random mask;
  (b) ``train_full_finetune.py:169`` passes an undefined ``start_epoch``; here it is 0.
Full fine-tuning goes through ``WhisperEncoder.enable_full_finetune()`` and is bf16 only.
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402


class EarlyStopper:   # Glitch_classification/src/utils.py
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


def main(args):
    from gw_whisper_amd import dist as gdist, glitch, ops
    from gw_whisper_amd.feature_extraction import WhisperFeatureExtractor
    from gw_whisper_amd.models import _pooled
    rank, world, local = gdist.init()
    assert torch.cuda.is_available(), "run_glitch_train.py needs an MI355X (gw_whisper_amd has no CPU path)"
    torch.cuda.set_device(local)
    device = torch.device("cuda", local)
    torch.manual_seed(args.seed)

    if args.synthetic:
        train_x, train_raw, _ = glitch.synthetic_split(args.synthetic, args.synthetic_classes, args.seed)
        test_x, test_raw, _ = glitch.synthetic_split(args.synthetic, args.synthetic_classes, args.seed, test=True)
    else:
        if not (args.train_data_path and args.test_data_path):
            raise SystemExit("--train_data_path and --test_data_path are required (or --synthetic N)")
        train_x, train_raw, _ = glitch.load_split(args.train_data_path)
        test_x, test_raw, _ = glitch.load_split(args.test_data_path)
    classes = glitch.fit_classes(list(train_raw) + list(test_raw))        # train.py:144-148
    train_y, test_y = glitch.encode_labels(train_raw, classes), glitch.encode_labels(test_raw, classes)

    n_mels = WhisperFeatureExtractor.from_pretrained(f"openai/whisper-{args.encoder}").feature_size
    model = glitch.build_model(args.encoder, len(classes), args.method, args.lora_rank, args.lora_alpha, args.precision,
                               args.lora_targets, args.encoder_weights, args.seed, device)
    # train.py:189 hands AdamW model.parameters(); the frozen ones never get a gradient and are never touched
    params = [p for p in model.parameters() if p.requires_grad]
    optimizer = torch.optim.AdamW(params, lr=args.learning_rate)
    bucket = gdist.FlatGradBucket(params)
    criterion = torch.nn.CrossEntropyLoss().to(device)
    os.makedirs(args.results_path, exist_ok=True)
    os.makedirs(args.log_dir, exist_ok=True)
    log = open(os.path.join(args.log_dir, "train_log.jsonl"), "a") if rank == 0 else None
    name = os.path.join(args.results_path, args.model_name)
    body_path = name + ("_best_whisper_weights.pth" if args.method == "full_finetune" else "_best_lora_weights.pth")

    def save_best(cm):
        if rank != 0:
            return
        torch.save(model.encoder.state_dict(), body_path)                               # train.py:125
        torch.save(model.classifier.state_dict(), name + "_best_dense_weights.pth")    # train.py:126
        np.save(name + "_best_confusion_matrix.npy", cm)
        with open(name + "_classes.json", "w") as f:
            json.dump(classes, f, indent=1)

    stopper, best, step_no = EarlyStopper(patience=60), float("inf"), 0
    for epoch in range(0, args.num_epochs):
        model.train()
        order = np.random.default_rng(args.seed + 1 + epoch).permutation(len(train_y))   # DataLoader(shuffle=True)
        t0, losses, seen = time.time(), [], 0
        for step in range(gdist.epoch_steps(len(order), world, args.batch_size)):
            sl = gdist.step_slice(len(order), step, rank, world, args.batch_size)
            bucket.zero()
            if sl is not None:
                idx = order[sl[0]:sl[1]]
                mel = ops.logmel(torch.from_numpy(train_x[idx]).to(device), n_mels=n_mels)
                y = torch.from_numpy(train_y[idx]).to(device)
                if args.head == "hip":
                    loss, _ = glitch.head_cross_entropy(model.classifier, _pooled(model.encoder, mel), y, seed=args.seed,
                                                        offset=step_no)
                    loss.backward()
                    losses.append(loss.detach())          # read once per epoch
                else:
                    loss = criterion(model(mel).float(), y)
                    loss.backward()
                    losses.append(loss.item())            # train.py:108
                seen += len(idx)
            step_no += 1
            bucket.all_reduce_mean(world, n_local=0 if sl is None else sl[1] - sl[0])
            optimizer.step()
        if losses and torch.is_tensor(losses[0]):
            losses = torch.stack(losses).double().cpu().tolist()
        train_loss = float(np.sum(losses)) / max(len(losses), 1)                          # train.py:110
        train_s = time.time() - t0
        val_loss, cm = glitch.evaluate_model(model, test_x, test_y, args.batch_size, args.head, n_mels)
        val_f1 = glitch.macro_f1(cm)
        val_loss = gdist.broadcast_scalar(val_loss, world, device)     # one decision for all ranks
        rec = {"epoch": epoch + 1, "train_loss": train_loss, "val_loss": val_loss, "val_f1": val_f1, "train_s": train_s,
               "epoch_s": time.time() - t0, "segments_per_s": len(order) / max(train_s, 1e-9), "rank0_segments": seen,
               "head": args.head}
        if rank == 0:
            print(f"Epoch {epoch + 1}/{args.num_epochs}, Train Loss: {train_loss:.4f}, Val Loss: {val_loss:.4f}, "
                  f"Val F1: {val_f1:.4f}")
            log.write(json.dumps(rec) + "\n")
            log.flush()
        if val_loss < best:
            best = val_loss
            save_best(cm)
        if stopper.early_stop(val_loss):
            if rank == 0:
                print(f"Early stopping at epoch {epoch + 1}")
            break
    if world > 1:
        torch.distributed.barrier()
        torch.distributed.destroy_process_group()


def build_parser():
    from gw_whisper_amd.glitch import DEFAULT_LORA_TARGETS
    parser = argparse.ArgumentParser(description="Glitch-classification training (MI355X path)")
    parser.add_argument("--train_data_path", type=str, default=None, help="Path to the training dataset")
    parser.add_argument("--test_data_path", type=str, default=None, help="Path to the test dataset")
    parser.add_argument("--log_dir", type=str, default="Glitch_classification/results/generic/logs")
    parser.add_argument("--results_path", type=str, default="Glitch_classification/results/generic")
    parser.add_argument("--encoder", type=str, default="tiny", help="Whisper encoder size")
    parser.add_argument("--batch_size", type=int, default=32)
    parser.add_argument("--num_epochs", type=int, default=200)
    parser.add_argument("--learning_rate", type=float, default=8e-5)
    parser.add_argument("--num_workers", type=int, default=4, help="accepted for compatibility; features are computed on the GPU")
    parser.add_argument("--model_name", type=str, default="multi_class_model")
    parser.add_argument("--method", type=str, choices=["LoRA", "DoRA", "full_finetune"], required=True)
    parser.add_argument("--lora_rank", type=int, default=8)
    parser.add_argument("--lora_alpha", type=int, default=32)
    parser.add_argument("--synthetic", type=int, default=0, help="use N seeded synthetic training segments (N // 4 test)")
    parser.add_argument("--synthetic-classes", type=int, default=11, help="classes of the synthetic set")
    parser.add_argument("--seed", type=int, default=42)
    parser.add_argument("--encoder-weights", type=str, default=None, help="HF WhisperEncoder state_dict (.pth / .safetensors)")
    parser.add_argument("--precision", choices=("bf16", "fp32"), default="bf16",
                        help="encoder arithmetic (full fine-tuning is bf16 only)")
    parser.add_argument("--lora-targets", type=str, nargs="+", default=list(DEFAULT_LORA_TARGETS), metavar="PATTERN",
                        help="fnmatch patterns of the encoder modules to adapt")
    parser.add_argument("--head", choices=("hip", "torch"), default="hip",
                        help="classifier head + loss: the HIP head step (default) or torch.nn (profiles/glitch_train.md)")
    return parser


if __name__ == "__main__":
    main(build_parser().parse_args())
