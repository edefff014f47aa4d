#!/usr/bin/env python3
"""Counterpart of the reference's ``Signal_vs_Noise/src/evaluation.py`` on the MI355X path.

Same sequence (``evaluation.py:91-160``): the encoder with the saved adapter (``PeftModel.from_pretrained``) under the
two- or one-detector head with its saved ``state_dict`` -- what ``run_train.py`` writes --, one no-grad pass per test set
in dataset order (loss, AUC, F1, classification report, ``:32-89``), then the ROC curve with its bootstrap band
(``bootstrap_roc_curve``, ``:110-122``: mean +- std of the TPR at 500 log-spaced FPRs over 1000 resamples).
``--lora_weights_path`` and ``--dense_layers_path`` are the two flags the reference's usage line names and its parser
forgot (``:154`` reads them).

Per test set i it writes into ``--out_dir``
  * ``ROC_curve_SNR_{i}_{model_type}.npz``: fpr, tpr, auc, grid, mean_tpr, std_tpr, all_labels, all_raw_preds, all_snr
    (the arrays behind the reference's figure; there is no plotting),
  * ``report_{i}.txt``: the classification report with the reference's ``target_names=['injection', 'noise']`` and the
    macro F1,
  * one line of ``eval_log.jsonl``: loss, auc, f1, n_valid.

Differences that come with the hardware path: features by ``ops.logmel`` on the GPU per batch; the probabilities, the
loss and the confusion matrix stay on the device and are read once (``roc.BinaryEvalState``); the ROC curve, the AUC and
the band are computed on the device (``roc.RocEvaluator``) from the resample indices of the host stream the reference
draws from, so ``--bootstrap_seed S`` gives what the reference gives after ``np.random.seed(S)``; ``--dataset_paths`` are
the HuggingFace ``datasets`` directories ``run_train.py`` reads, ``--synthetic N`` its seeded synthetic set;
``--encoder-weights`` / seeded base weights as there.  Where the adapter directory holds a ``preprocessor_config.json`` and
a ``config.json`` -- a ``run_train.py`` run with front-end flags writes them -- the features and the encoder's context are
theirs, ``--synthetic`` segments come at that sampling rate, and the line of ``eval_log.jsonl`` names the context and the
extractor it used; one of the two files without the other is an error (``saved_front_end``).
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402


def load_arrays(path):
    from datasets import concatenate_datasets, load_from_disk
    chunks = sorted(p for p in os.listdir(path) if p.startswith("chunk")) if os.path.isdir(path) else []
    ds = concatenate_datasets([load_from_disk(os.path.join(path, c)) for c in chunks]) if chunks else load_from_disk(path)
    cols = ds.with_format("numpy")
    h1 = np.asarray(cols["h1_timeseries"], np.float32) if "h1_timeseries" in ds.column_names else None
    return (h1, np.asarray(cols["l1_timeseries"], np.float32), np.asarray(cols["labels"], np.float32),
            np.asarray(cols["injection_snr"], np.float32))


def saved_front_end(model_dir, encoder_name):
    """(encoder configuration, ``ops.logmel``'s ``config``, sampling rate) of a saved model.  A ``run_train.py`` run with
    front-end flags left ``preprocessor_config.json`` and the encoder's ``config.json`` beside the adapter: the two are read
    together or not at all.  A directory that holds one without the other -- a copy that lost a file -- or two that do not
    fit each other is an error, never a run on Whisper's defaults.  Needs no GPU."""
    from gw_whisper_amd import synth
    from gw_whisper_amd.encoder import WhisperConfig
    from gw_whisper_amd.feature_extraction import WhisperFeatureExtractor
    config = WhisperConfig.named(encoder_name)
    pre, cfg_json = (os.path.join(model_dir, n) for n in ("preprocessor_config.json", "config.json"))
    saved = None
    if os.path.isfile(cfg_json):
        saved = WhisperConfig.from_json_file(cfg_json)
        if (saved.d_model, saved.encoder_layers, saved.encoder_attention_heads, saved.encoder_ffn_dim) != \
                tuple(synth.ENCODER_SIZES[encoder_name]):
            raise SystemExit(f"{cfg_json} describes another encoder than --encoder {encoder_name}")
    if not os.path.isfile(pre):
        # (a fully fine-tuned encoder of the default context has a config.json and no preprocessor_config.json)
        if saved is not None and saved.max_source_positions != config.max_source_positions:
            raise SystemExit(f"{cfg_json} has max_source_positions {saved.max_source_positions} but {pre} is missing: the "
                             "encoder's front end is unknown")
        return config, None, 16000
    if saved is None:
        raise SystemExit(f"{pre} is there but {cfg_json} is missing: the encoder's context is unknown")
    extractor = WhisperFeatureExtractor.from_pretrained(model_dir)
    if extractor.feature_size != saved.num_mel_bins or extractor.nb_max_frames != 2 * saved.max_source_positions:
        raise SystemExit(f"{pre} gives [{extractor.feature_size}, {extractor.nb_max_frames}] features, {cfg_json} an encoder "
                         f"of [{saved.num_mel_bins}, {2 * saved.max_source_positions}]")
    return saved, extractor.frontend_config, extractor.sampling_rate


def load_models(args, device):
    """evaluation.py:91-103."""
    from gw_whisper_amd import synth
    from gw_whisper_amd.encoder import WhisperEncoder
    from gw_whisper_amd.models import one_channel_ligo_binary_classifier, two_channel_ligo_binary_classifier
    from gw_whisper_amd.peft import PeftModel
    d, L, H, F = synth.ENCODER_SIZES[args.encoder]
    config, fe_config, rate = saved_front_end(args.lora_weights_path, args.encoder)
    encoder = WhisperEncoder(config, precision=args.precision)
    if args.encoder_weights:
        if args.encoder_weights.endswith(".safetensors"):
            from safetensors.torch import load_file
            encoder.load_state_dict(load_file(args.encoder_weights))
        else:
            encoder.load_state_dict(torch.load(args.encoder_weights, map_location="cpu"))
    else:
        sd = synth.encoder_state_dict(d, L, H, F, seed=args.seed, n_mels=config.num_mel_bins)
        encoder.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    peft = PeftModel.from_pretrained(encoder, args.lora_weights_path).to(device)
    head = two_channel_ligo_binary_classifier if args.model_type == "2D" else one_channel_ligo_binary_classifier
    model = head(peft, num_classes=1).to(device)
    model.classifier.load_state_dict(torch.load(args.dense_layers_path, map_location=device))
    return model.eval(), config, fe_config, rate


def evaluate(model, arrays, args, n_mels, device, fe_config=None):
    """One pass in dataset order (evaluation.py:32-64); nothing is read from the device before the pass is over."""
    from gw_whisper_amd import ops, roc
    h1, l1, labels, snr = arrays
    n = len(labels)
    state = roc.BinaryEvalState(n, device)
    with torch.no_grad():
        for i in range(0, n, args.batch_size):
            sl = slice(i, min(i + args.batch_size, n))
            if args.model_type == "2D":
                mel = ops.logmel(torch.from_numpy(np.concatenate((h1[sl], l1[sl]))).to(device), n_mels=n_mels,
                                 config=fe_config)
                b = sl.stop - sl.start
                logits = model(mel[:b], mel[b:])
            else:
                logits = model(ops.logmel(torch.from_numpy(l1[sl]).to(device), n_mels=n_mels, config=fe_config))
            state.add(logits.float(), torch.from_numpy(labels[sl]).to(device), torch.from_numpy(snr[sl]).to(device))
    return state


def main(args):
    from gw_whisper_amd import glitch, roc
    assert torch.cuda.is_available(), "run_evaluation.py needs an MI355X (gw_whisper_amd has no CPU path)"
    device = torch.device("cuda", 0)
    if not args.lora_weights_path or not args.dense_layers_path:
        raise SystemExit("--lora_weights_path and --dense_layers_path are required")
    if not args.synthetic and not args.dataset_paths:
        raise SystemExit("--dataset_paths P... is required (or --synthetic N)")
    model, config, fe_config, rate = load_models(args, device)
    n_mels = config.num_mel_bins
    if args.synthetic:
        from run_train import synthetic_dataset
        sets = [synthetic_dataset(args.synthetic, args.seed, rate)]
    else:
        sets = [load_arrays(p) for p in args.dataset_paths]
    os.makedirs(args.out_dir, exist_ok=True)
    ev = roc.RocEvaluator(num_bootstrap=args.num_bootstrap, seed=args.bootstrap_seed)
    with open(os.path.join(args.out_dir, "eval_log.jsonl"), "a") as log:
        for i, arrays in enumerate(sets):
            if args.model_type == "2D" and arrays[0] is None:
                raise SystemExit(f"test set {i} has no h1_timeseries column: --model_type 2D needs both detectors")
            state = evaluate(model, arrays, args, n_mels, device, fe_config)
            out = ev(state.scores[:state.filled], state.labels[:state.filled])
            res = state.read()
            np.savez(os.path.join(args.out_dir, f"ROC_curve_SNR_{i}_{args.model_type}.npz"), fpr=out["fpr"], tpr=out["tpr"],
                     auc=np.float64(out["auc"]), grid=out["grid"], mean_tpr=out["mean_tpr"], std_tpr=out["std_tpr"],
                     all_labels=res["labels"], all_raw_preds=res["scores"], all_snr=res["snr"])
            f1 = glitch.macro_f1(res["confusion"])
            with open(os.path.join(args.out_dir, f"report_{i}.txt"), "w") as f:
                f.write(glitch.classification_report(res["confusion"], ["injection", "noise"]))   # evaluation.py:69
                f.write(f"\nmacro F1: {f1:.6f}\n")
            rec = {"dataset": i, "n": state.filled, "loss": res["loss"], "auc": out["auc"], "f1": f1,
                   "n_valid": out["n_valid"], "num_bootstrap": args.num_bootstrap}
            if fe_config is not None:      # the saved front end this run computed its features with
                rec.update(max_source_positions=config.max_source_positions, sampling_rate=rate, n_fft=fe_config.n_fft,
                           hop_length=fe_config.hop_length, n_frames=fe_config.n_frames,
                           max_frequency=fe_config.max_frequency)
            log.write(json.dumps(rec) + "\n")
            log.flush()
            print(f"test set {i}: loss {res['loss']:.4f}, AUC {out['auc']:.4f}, macro F1 {f1:.4f}, "
                  f"{out['n_valid']}/{args.num_bootstrap} resamples in the band")


def build_parser():
    parser = argparse.ArgumentParser(description="Evaluate LIGO models with 1D or 2D data (MI355X path)")
    parser.add_argument("--model_type", type=str, choices=["1D", "2D"], required=True, help="Model type: 1D or 2D")
    parser.add_argument("--lora_weights_path", type=str, default=None, help="adapter directory run_train.py saved")
    parser.add_argument("--dense_layers_path", type=str, default=None, help="the head's state_dict (.pth) run_train.py saved")
    parser.add_argument("--dataset_paths", type=str, nargs="+", default=None, metavar="P",
                        help="HuggingFace datasets directories with l1_timeseries (and h1_timeseries), labels, injection_snr")
    parser.add_argument("--synthetic", type=int, default=0, help="evaluate N seeded synthetic segments instead of --dataset_paths")
    parser.add_argument("--seed", type=int, default=42, help="the synthetic set and the seeded base weights, as in run_train.py")
    parser.add_argument("--encoder", type=str, default="tiny")
    parser.add_argument("--batch_size", type=int, default=128)
    parser.add_argument("--num_bootstrap", type=int, default=1000)
    parser.add_argument("--bootstrap_seed", type=int, default=None,
                        help="np.random.seed of the resamples (default: unseeded, as the reference)")
    parser.add_argument("--out_dir", type=str, default="Detection/results/figures")
    parser.add_argument("--encoder-weights", type=str, default=None, help="HF WhisperEncoder state_dict (.pth / .safetensors)")
    parser.add_argument("--precision", choices=("bf16", "fp32"), default="bf16")
    return parser


if __name__ == "__main__":
    main(build_parser().parse_args())
