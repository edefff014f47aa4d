#!/usr/bin/env python3
"""Counterpart of the reference's ``Signal_vs_Noise/Real_events`` on the MI355X path: ``preprocess_real_events.py`` and
``evaluation_real_events.py`` in one program, without the ``datasets`` directories between them.

The reference cuts the H1 / L1 strain of every catalogue event (2048 Hz) into windows of 2048 samples every 204
(``preprocess_real_events.py:12-17``), resamples each to 16 kHz, saves 2 x 31 ``datasets`` directories per event, and
then runs the two-detector model on them at batch 1 and stores ``sigmoid(logit)`` (``evaluation_real_events.py:29-67``).
Here ``real_events.scan_events`` uploads the strain once and scores the windows of all events in batches.

Flags of ``preprocess_real_events.py``: ``--timeseries_data_test``, ``--event_name`` (zero or more; default: every event
of the file, in file order), ``--encoder``.  Flags of ``evaluation_real_events.py``: ``--output_path``,
``--lora_weights_file``, ``--dense_layers_file``.  New: ``--head {mlp,cnn}`` (the reference switches decoders by a
commented-out line, ``:19-20``), ``--encoder-weights``, ``--batch-size``, ``--first-window-only``, ``--precision``,
``--seed`` (the seeded base weights when no ``--encoder-weights`` are given, as in ``run_train.py``).

A model trained at the strain's own rate (``run_train.py --sampling-rate 2048 --n-fft 128 --hop-length 12 --chunk-length 1``)
leaves ``preprocessor_config.json`` and the encoder's ``config.json`` beside ``--lora_weights_file``: where they are there
the scan runs that front end and that context (``run_evaluation.saved_front_end``; one file without the other is an
error), windows of ``chunk_length * sampling_rate`` samples every ``--step-samples`` (the reference's 204), their features
through ``ops.logmel_windows`` -- no resampling, no window cut, an STFT frame that several windows of a batch share
computed once.  ``--sampling-rate --n-fft --hop-length --chunk-length --mel-fmax`` override what was saved, field by field.
Without the files and the flags the run is the reference's: resample to 16 kHz, Whisper's published log-mel.

Input: HDF5 with ``<event>/h1_strain`` and ``<event>/l1_strain`` when ``h5py`` imports, otherwise the ``.npz`` twin with
those names as array keys (given directly, or found as ``<path>.npz``).  Output: ``model_output`` [events, windows]
float32 and ``event_names`` (the key up to its first ``-``, the reference's ``split('-')[0]``), HDF5 or -- without
``h5py`` -- ``<output>.npz``.

Quirk of the reference, documented and not copied: it globs ``<event>/h1_segments/segment_0`` only (``:85-86``), so as
written it scores window 0 of every event, although its own comment expects ``(31,)``.  The default here is every
window; ``--first-window-only`` writes the ``[events, 1]`` the program as written produces.  (Its import of
``Detection.src.model``, a package the tree does not have, is noted in SURVEY.md C8.)
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402


def check_head_file(state, head, path):
    """A clear error when the saved head is not the chosen one: the MLP's first weight is a matrix, the CNN's a
    [64, 2, 3] conv kernel."""
    from gw_whisper_amd import GwwError
    w = state.get("0.weight")
    if w is None:
        raise GwwError(f"{path}: no '0.weight' -- not a classifier state_dict of a two-detector model")
    want = 3 if head == "cnn" else 2
    if w.dim() != want:
        other = "cnn" if head == "mlp" else "mlp"
        raise GwwError(f"{path}: '0.weight' has shape {tuple(w.shape)}, the head of --head {other}; --head {head} needs a "
                       f"rank-{want} first weight")


def front_end(args):
    """(encoder configuration, ``ops.FrontendConfig`` or None, window length in samples) of a run: what is saved beside
    ``--lora_weights_file`` (``run_evaluation.saved_front_end``), overridden field by field by the front-end flags; None and
    2048 samples -- the reference's resample + published log-mel -- when there is neither.  Needs no GPU."""
    import dataclasses
    from gw_whisper_amd import ops, real_events
    from run_evaluation import saved_front_end
    config, fe, _ = saved_front_end(args.lora_weights_file, args.encoder)
    flags = {k: getattr(args, k) for k in ("sampling_rate", "n_fft", "hop_length", "chunk_length", "mel_fmax")}
    if all(v is None for v in flags.values()):
        return config, fe, (real_events.WINDOW_SIZE if fe is None else fe.n_samples)
    if fe is None:
        missing = [k for k in ("sampling_rate", "n_fft", "hop_length") if flags[k] is None]
        if missing:
            raise SystemExit("a front end from flags alone needs --sampling-rate, --n-fft and --hop-length (missing: "
                             + ", ".join("--" + m.replace("_", "-") for m in missing) + ")")
        saved = dict(sampling_rate=None, n_fft=None, hop_length=None, chunk_length=1, mel_fmax=8000.0)
    else:
        saved = dict(sampling_rate=fe.sampling_rate, n_fft=fe.n_fft, hop_length=fe.hop_length,
                     chunk_length=fe.n_samples // fe.sampling_rate, mel_fmax=fe.max_frequency)
    got = {k: saved[k] if v is None else v for k, v in flags.items()}
    n_samples = got["chunk_length"] * got["sampling_rate"]
    frames = n_samples // got["hop_length"] if got["hop_length"] > 0 else 0
    if frames % 2:
        raise SystemExit(f"--chunk-length {got['chunk_length']} --sampling-rate {got['sampling_rate']} --hop-length "
                         f"{got['hop_length']}: {frames} frames, an odd count; the encoder's stride-2 conv needs an even one")
    fe = ops.FrontendConfig(config.num_mel_bins, got["sampling_rate"], got["n_fft"], got["hop_length"], n_samples, 0.0,
                            float(got["mel_fmax"]))
    ops.frontend_validate(fe)
    return dataclasses.replace(config, max_source_positions=frames // 2), fe, n_samples


def load_model(args, device, config=None):
    """``evaluation_real_events.py:15-22``."""
    from gw_whisper_amd import synth
    from gw_whisper_amd.encoder import WhisperConfig, WhisperEncoder
    from gw_whisper_amd.models import TwoChannelLIGOBinaryClassifierCNN, two_channel_ligo_binary_classifier
    from gw_whisper_amd.peft import PeftModel
    state = torch.load(args.dense_layers_file, map_location="cpu")
    check_head_file(state, args.head, args.dense_layers_file)
    d, L, H, F = synth.ENCODER_SIZES[args.encoder]
    config = WhisperConfig.named(args.encoder) if config is None else config
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
    peft = PeftModel.from_pretrained(encoder, args.lora_weights_file).to(device)
    cls = TwoChannelLIGOBinaryClassifierCNN if args.head == "cnn" else two_channel_ligo_binary_classifier
    model = cls(peft, num_classes=1).to(device)
    model.classifier.load_state_dict(state)
    return model.eval(), config.num_mel_bins


def write_result(path, model_output, names):
    from gw_whisper_amd import real_events
    path = real_events.output_path(path)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    if path.endswith(".npz"):
        np.savez(path, model_output=model_output, event_names=np.array(names))
        return path
    import h5py
    with h5py.File(path, "w") as f:                       # evaluation_real_events.py:24-27
        f.create_dataset("model_output", data=model_output)
        f.create_dataset("event_names", data=names)
    return path


def main(args):
    from gw_whisper_amd import real_events
    keys, strain = real_events.read_events(args.timeseries_data_test, args.event_name)
    assert torch.cuda.is_available(), "run_real_events.py needs an MI355X (gw_whisper_amd has no CPU path)"
    device = torch.device("cuda", 0)
    config, fe_config, window = front_end(args)
    model, n_mels = load_model(args, device, config)
    if args.first_window_only:
        strain = strain[:, :, :window]                    # window 0 alone: what the reference's glob scores
    out = real_events.scan_events(model, strain, batch_size=args.batch_size, window_size=window, step_size=args.step_samples,
                                  n_mels=n_mels, device=device, frontend=fe_config)
    names = [real_events.event_label(k) for k in keys]
    path = write_result(args.output_path, out, names)
    print(f"Saved model output {out.shape} of {len(names)} events to {path}")


def build_parser():
    p = argparse.ArgumentParser(description="Score catalogue events with the two-detector model (MI355X path)")
    p.add_argument("--timeseries_data_test", type=str, required=True,
                   help="HDF5 (or .npz twin) with <event>/h1_strain and <event>/l1_strain at 2048 Hz")
    p.add_argument("--event_name", type=str, nargs="*", default=None, help="events to score, in this order (default: all)")
    p.add_argument("--encoder", type=str, default="tiny", help="Whisper encoder size")
    p.add_argument("--output_path", type=str, default="Detection/Real_events/results/results_2_detectors_real_events.hdf")
    p.add_argument("--lora_weights_file", type=str, default="Detection/Real_events/results/models/best_lora_weights_8_32/")
    p.add_argument("--dense_layers_file", type=str, default="Detection/Real_events/results/models/best_dense_layers_8_32.pth")
    p.add_argument("--head", choices=("mlp", "cnn"), default="mlp",
                   help="two_channel_ligo_binary_classifier (default) or TwoChannelLIGOBinaryClassifierCNN")
    p.add_argument("--encoder-weights", type=str, default=None, help="HF WhisperEncoder state_dict (.pth / .safetensors)")
    p.add_argument("--batch-size", type=int, default=256, help="windows per pass, over all events")
    p.add_argument("--first-window-only", action="store_true",
                   help="score window 0 of every event only, as the reference program as written does")
    p.add_argument("--precision", choices=("bf16", "fp32"), default="bf16")
    p.add_argument("--seed", type=int, default=42, help="the seeded base weights when no --encoder-weights are given")
    # a native-rate front end: default, what is saved beside --lora_weights_file (else the reference's 16 kHz path)
    p.add_argument("--sampling-rate", type=int, default=None, help="Hz the model's front end takes the strain at")
    p.add_argument("--n-fft", type=int, default=None)
    p.add_argument("--hop-length", type=int, default=None)
    p.add_argument("--chunk-length", type=int, default=None, help="seconds per window: the window is chunk_length * sampling_rate samples")
    p.add_argument("--mel-fmax", type=float, default=None, help="upper edge of the mel filterbank in Hz")
    p.add_argument("--step-samples", type=int, default=204, help="samples between windows (preprocess_real_events.py:12)")
    return p


if __name__ == "__main__":
    main(build_parser().parse_args())
