#!/usr/bin/env python3
"""Counterpart of the reference's ``Glitch_classification/src/evaluate.py`` on the MI355X path.

Same flags (``evaluate.py:110-121``), same sequence: label encoder fitted on the TEST labels only (``:83-89``, as the
reference does -- the class order equals the training run's when the test set holds every class), the model rebuilt from
``--method / --lora_rank / --lora_alpha`` (``:16-36``), both ``.pth`` files loaded, eval mode, one pass in dataset order.
Writes ``<results_path>/<model_name>_test_classification_report.txt`` in the layout of sklearn's
``classification_report(..., zero_division=0)`` and, in place of the PNG, ``<model_name>_test_confusion_matrix.npy``
(int64 counts, rows = true class).

Differences that come with the hardware path: features by ``ops.logmel`` on the GPU per batch; ``--head hip`` (default)
keeps the confusion matrix on the device and reads it once, ``--head torch`` is the reference's per-batch
``argmax(...).cpu()`` loop; ``--method full_finetune`` takes the ``*_best_whisper_weights.pth`` of
``run_glitch_train.py --method full_finetune`` as ``--lora_weights_path``; ``--synthetic N`` evaluates the test split
``run_glitch_train.py --synthetic N`` validated on; ``--encoder-weights`` / seeded base weights as there.
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402


def main(args):
    from gw_whisper_amd import glitch
    from gw_whisper_amd.feature_extraction import WhisperFeatureExtractor
    assert torch.cuda.is_available(), "run_glitch_evaluate.py needs an MI355X (gw_whisper_amd has no CPU path)"
    device = torch.device("cuda", 0)
    if args.synthetic:
        test_x, test_raw, _ = glitch.synthetic_split(args.synthetic, args.synthetic_classes, args.seed, test=True)
    else:
        if not args.test_data_path:
            raise SystemExit("--test_data_path is required (or --synthetic N)")
        test_x, test_raw, _ = glitch.load_split(args.test_data_path, concatenated=False)
    classes = glitch.fit_classes(test_raw)                                   # evaluate.py:83-87
    test_y = glitch.encode_labels(test_raw, classes)
    n_mels = WhisperFeatureExtractor.from_pretrained(f"openai/whisper-{args.encoder}").feature_size
    model = glitch.build_model(args.encoder, len(classes), args.method, args.lora_rank, args.lora_alpha, args.precision,
                               args.lora_targets, args.encoder_weights, args.seed, device)
    model.encoder.load_state_dict(torch.load(args.lora_weights_path, map_location=device))       # evaluate.py:33
    model.classifier.load_state_dict(torch.load(args.dense_weights_path, map_location=device))   # evaluate.py:34
    print("Evaluating model on test dataset...")
    _loss, cm = glitch.evaluate_model(model, test_x, test_y, args.batch_size, args.head, n_mels)
    os.makedirs(args.results_path, exist_ok=True)
    name = os.path.join(args.results_path, args.model_name)
    report = glitch.classification_report(cm, classes)
    with open(name + "_test_classification_report.txt", "w") as f:
        f.write(report)
    print(f"Classification report saved to {name}_test_classification_report.txt")
    np.save(name + "_test_confusion_matrix.npy", cm)
    print(f"Confusion matrix saved to {name}_test_confusion_matrix.npy")


def build_parser():
    from gw_whisper_amd.glitch import DEFAULT_LORA_TARGETS
    parser = argparse.ArgumentParser(description="Glitch-classification test-set evaluation (MI355X path)")
    parser.add_argument("--test_data_path", type=str, default=None, help="Path to the test dataset")
    parser.add_argument("--results_path", type=str, default="Glitch_classification/results/generic")
    parser.add_argument("--encoder", type=str, default="tiny", help="Whisper encoder size")
    parser.add_argument("--batch_size", type=int, default=32)
    parser.add_argument("--num_workers", type=int, default=4, help="accepted for compatibility; features are computed on the GPU")
    parser.add_argument("--model_name", type=str, default="multi_class_model")
    parser.add_argument("--method", type=str, choices=["LoRA", "DoRA", "full_finetune"], required=True)
    parser.add_argument("--lora_weights_path", type=str, required=True, help="Path to the best LoRA weights file")
    parser.add_argument("--dense_weights_path", type=str, required=True, help="Path to the best dense weights file")
    parser.add_argument("--lora_rank", type=int, default=8)
    parser.add_argument("--lora_alpha", type=int, default=32)
    parser.add_argument("--synthetic", type=int, default=0, help="evaluate the synthetic test split of run_glitch_train.py")
    parser.add_argument("--synthetic-classes", type=int, default=11)
    parser.add_argument("--seed", type=int, default=42)
    parser.add_argument("--encoder-weights", type=str, default=None, help="HF WhisperEncoder state_dict (.pth / .safetensors)")
    parser.add_argument("--precision", choices=("bf16", "fp32"), default="bf16")
    parser.add_argument("--lora-targets", type=str, nargs="+", default=list(DEFAULT_LORA_TARGETS), metavar="PATTERN")
    parser.add_argument("--head", choices=("hip", "torch"), default="hip")
    return parser


if __name__ == "__main__":
    main(build_parser().parse_args())
