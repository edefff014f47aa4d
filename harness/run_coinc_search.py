#!/usr/bin/env python3
"""The single-detector model on continuous data: a coincident two-detector search with a time-slide background, or the
events of one detector alone (``gw_whisper_amd/coinc.py``).

The reference trains a single-detector model (``Signal_vs_Noise/src/sd_train.py``, ``src/model.py:31-52``) and ships one,
but none of its programs runs it over a segment, and its search (``MLGWSC-1/inference.py``) carries ``--coinc-window`` as
a reserved flag.  This program is that missing search: every window of every detector is scored by the model
``run_train.py --detectors 1`` saves, each detector's scores are thresholded and clustered into events as
``run_inference.py`` clusters its triggers, and the device pairs the events of H1 and L1 at zero lag and under S
non-circular time slides.

    run_coinc_search.py IN.hdf OUT.hdf --lora-weights A [A_L1] --dense-weights H.pth [H_L1.pth]
        [--detectors H1 L1 | H1 | L1] [--white] [--encoder tiny] [--encoder-weights W]
        [-t T] [--step-size 0.1] [--cluster-threshold 0.35] [--coinc-window 0.15]
        [--time-slides S --slide-shift 2.0 --slides-output B.hdf]
        [--sampling-rate --n-fft --hop-length --chunk-length --mel-fmax] [--synthetic SECONDS] [--batch-size 256] [--force]

The input is ``run_inference.py``'s (its reader, the ``.npz`` twin included); one set of weights serves both detectors,
two sets give every detector its own model; without weights the parameters are seeded (there is no network for
checkpoints).  A model trained at the strain's own rate is run on its saved front end as ``run_real_events.py`` does it.
``OUT`` holds ``time``, ``stat``, ``var``: per coincidence the H1 event's time and the sum of the two logits -- with one
detector, that detector's events.  ``B`` holds ``time``, ``stat``, ``var``, ``slide``, ``slide_livetime`` [S] and
``livetime``, the layout of ``run_inference.py --slides-output``: ``run_search_evaluate.py --foreground-events OUT
--background-events B`` reads both.  One rank only.
"""
from __future__ import annotations

import argparse
import logging
import os
import sys
import time as t

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import run_inference as ri  # noqa: E402  (the reader, write_result and the detector order live there)

DETECTORS = ri.DETECTORS


def parse_args(argv=None):
    p = argparse.ArgumentParser(description="Single-detector model: coincident search with a slid background (MI355X).")
    p.add_argument("--verbose", action="store_true")
    p.add_argument("--force", action="store_true", help="Overwrite existing output files.")
    p.add_argument("inputfile", type=str, help="Input HDF5 / .npz (ignored with --synthetic).")
    p.add_argument("outputfile", type=str, help="Output HDF5 / .npz (must not exist unless --force).")
    p.add_argument("--detectors", type=str, nargs="+", default=list(DETECTORS), choices=DETECTORS,
                   help="The detectors to search: both (a coincident search) or one (its events alone).")
    p.add_argument("--white", action="store_true", help="Input is already whitened (otherwise every segment is whitened on the device first).")
    p.add_argument("--lora-weights", type=str, nargs="*", default=[], help="peft adapter directory: one, or one per detector.")
    p.add_argument("--dense-weights", type=str, nargs="*", default=[], help="Dense head weights (.pth): as many as --lora-weights.")
    p.add_argument("--encoder", type=str, default="tiny")
    p.add_argument("--encoder-weights", type=str, default=None, help="HF WhisperEncoder state_dict (.pth / .safetensors).")
    p.add_argument("--precision", choices=("bf16", "fp32"), default="bf16")
    p.add_argument("-t", "--trigger-threshold", type=float, default=-0.5, help="A window is a trigger when its logit exceeds this.")
    p.add_argument("--step-size", type=float, default=0.1)
    p.add_argument("--cluster-threshold", type=float, default=0.35)
    p.add_argument("--coinc-window", type=float, default=0.15,
                   help="Seconds two detectors' events may lie apart.  Default 0.15, one and a half steps: both detectors' "
                        "stamps come from one table, so two peak windows differ by whole steps; 0.15 takes in a neighbouring "
                        "window whatever the last bits of the running-sum stamps are and excludes the next one (0.1 would "
                        "sit on the boundary), and 2 * 0.15 < 0.35 keeps the matching one to one.")
    p.add_argument("--time-slides", type=int, default=0, help="Number of time slides of background per segment (0: none).")
    p.add_argument("--slide-shift", type=float, default=2.0, help="Seconds between two slides (a whole number of steps).")
    p.add_argument("--slides-output", type=str, default=None, help="Output file of the slid background events.")
    p.add_argument("--synthetic", type=float, default=None, help="Seconds of synthetic whitened noise instead of inputfile.")
    p.add_argument("--batch-size", type=int, default=256, help="Windows per pass (times the detectors, with one model).")
    p.add_argument("--seed", type=int, default=0)
    # a native-rate front end: default, what is saved beside --lora-weights (else resample to 16 kHz + the published log-mel)
    p.add_argument("--sampling-rate", type=int, default=None, help="Hz the model's front end takes the strain at")
    p.add_argument("--n-fft", type=int, default=None)
    p.add_argument("--hop-length", type=int, default=None)
    p.add_argument("--chunk-length", type=int, default=None, help="seconds per window")
    p.add_argument("--mel-fmax", type=float, default=None, help="upper edge of the mel filterbank in Hz")
    return p.parse_args(argv)


def check_args(args, world: int):
    """Everything that can be refused before a GPU is touched; returns the detector rows to search, in DETECTORS order."""
    if world > 1:
        raise SystemExit("run_coinc_search: runs on one rank only (WORLD_SIZE > 1 is not supported); segments are "
                         "independent, so split the input by segment instead")
    if len(set(args.detectors)) != len(args.detectors):
        raise SystemExit(f"run_coinc_search: --detectors {' '.join(args.detectors)} names a detector twice")
    rows = [i for i, d in enumerate(DETECTORS) if d in args.detectors]
    D = len(rows)
    if len(args.lora_weights) not in (0, 1, D):
        raise SystemExit(f"run_coinc_search: {len(args.lora_weights)} --lora-weights for {D} detector(s): one, or one per detector")
    if len(args.dense_weights) != len(args.lora_weights):
        raise SystemExit(f"run_coinc_search: {len(args.dense_weights)} --dense-weights but {len(args.lora_weights)} --lora-weights: "
                         "every adapter comes with its head")
    if args.time_slides < 0:
        raise SystemExit("run_coinc_search: --time-slides must be >= 0")
    if not args.coinc_window >= 0:
        raise SystemExit("run_coinc_search: --coinc-window must not be negative")
    if args.time_slides > 0:
        if D == 1:
            raise SystemExit(f"run_coinc_search: --time-slides needs two detectors: a slide pairs the events of H1 with shifted "
                             f"events of L1, and --detectors {args.detectors[0]} leaves nothing to slide against")
        if args.slides_output is None:
            raise SystemExit("run_coinc_search: --time-slides needs --slides-output FILE")
    if D == 2 and not 2 * args.coinc_window < args.cluster_threshold:
        raise SystemExit(f"run_coinc_search: 2 * --coinc-window = {2 * args.coinc_window} s must be less than --cluster-threshold "
                         f"= {args.cluster_threshold} s, or one event could pair with two events of the other detector")
    if os.path.isfile(args.outputfile) and not args.force:
        raise RuntimeError("Output file exists. Use --force to overwrite.")
    if args.time_slides > 0 and os.path.isfile(args.slides_output) and not args.force:
        raise RuntimeError("Slides file exists. Use --force to overwrite.")
    return rows


def front_end(args, lora_dir):
    """``run_real_events.front_end`` for one adapter directory (None: nothing is saved, the flags alone decide)."""
    import run_real_events as rre
    shim = argparse.Namespace(lora_weights_file=os.devnull if lora_dir is None else lora_dir, encoder=args.encoder,
                              **{k: getattr(args, k) for k in ("sampling_rate", "n_fft", "hop_length", "chunk_length", "mel_fmax")})
    return rre.front_end(shim)           # os.devnull: no file lies beneath it, so nothing is found saved


def load_model(args, device, config, lora_dir, dense_file):
    """What ``run_train.py --detectors 1`` saves: the adapter directory and the head's state_dict
    (``run_evaluation.load_models`` with ``--model_type 1D``); seeded DoRA adapters and head without them."""
    import torch
    from gw_whisper_amd import synth
    from gw_whisper_amd.encoder import WhisperEncoder
    from gw_whisper_amd.models import one_channel_ligo_binary_classifier
    from gw_whisper_amd.peft import LoraConfig, PeftModel, get_peft_model
    torch.manual_seed(args.seed)
    d, L, H, F = synth.ENCODER_SIZES[args.encoder]
    encoder = WhisperEncoder(config, precision=args.precision)
    if args.encoder_weights:
        if args.encoder_weights.endswith(".safetensors"):
            from safetensors.torch import load_file
            encoder.load_state_dict(load_file(args.encoder_weights))
        else:
            encoder.load_state_dict(torch.load(args.encoder_weights, map_location="cpu"))
    else:
        sd = synth.encoder_state_dict(d, L, H, F, seed=args.seed, n_mels=config.num_mel_bins)
        if sd["embed_positions.weight"].shape[0] != config.max_source_positions:
            sd["embed_positions.weight"] = sd["embed_positions.weight"][:config.max_source_positions].copy()
        encoder.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    if lora_dir is not None:
        peft = PeftModel.from_pretrained(encoder, lora_dir)
    else:
        targets = [n for n, _ in encoder.named_modules() if n.endswith(("q_proj", "k_proj", "v_proj"))]
        peft = get_peft_model(encoder, LoraConfig(use_dora=True, r=8, lora_alpha=32, target_modules=targets))
    model = one_channel_ligo_binary_classifier(peft.to(device), num_classes=1).to(device)
    if dense_file is not None:
        model.classifier.load_state_dict(torch.load(dense_file, map_location=device))
    return model.eval()


def background_dict(cols, slide_live):
    """The six datasets of a slides file, named and typed as ``run_inference.py --slides-output`` writes them."""
    return {"time": cols[0], "stat": cols[1], "var": cols[2], "slide": cols[3].astype(np.int32),
            "slide_livetime": slide_live, "livetime": np.float64(slide_live.sum())}


def search(args, device, rows):
    import torch  # noqa: F401
    from gw_whisper_amd import coinc
    from gw_whisper_amd import inference as inf
    D, S = len(rows), args.time_slides
    dirs = args.lora_weights or [None]
    heads = args.dense_weights or [None]
    configs = [front_end(args, d) for d in dirs]
    if any(c[1:] != configs[0][1:] for c in configs[1:]):
        raise SystemExit("run_coinc_search: the two models were saved with different front ends; one scan cuts one kind of window")
    _, fe, window_len = configs[0]
    models = [load_model(args, device, c[0], d, h) for c, d, h in zip(configs, dirs, heads)]
    model = models[0] if len(models) == 1 else models
    if args.synthetic is not None:
        rng = np.random.default_rng(args.seed)
        n = int(round(args.synthetic * 2048))
        segs = {"synthetic": (rng.standard_normal((len(DETECTORS), n)).astype(np.float32), 1.0e9, 1.0 / 2048)}
    else:
        segs = ri.read_segments(args.inputfile)
    fg, bg, slide_live = {}, {}, np.zeros((max(S, 0),), np.float64)
    for key in sorted(segs, key=lambda k: segs[k][0].shape[1], reverse=True):
        strain, start, dt = segs[key]
        slicer = inf.DeviceSegmentSlicer(strain[rows], start_time=start, delta_t=dt, step_size=args.step_size, key=key,
                                         device=device, white=args.white, slice_length=window_len)
        if len(slicer) < 1:
            logging.info("segment %s holds no window", key)
            continue
        plan = None
        if S > 0:
            plan = coinc.slide_shifts(len(slicer), args.step_size, args.slide_shift, S, slicer.slice_length * slicer.delta_t,
                                      slicer.time_step_size, window=args.coinc_window)
            slide_live += plan.livetime
        logging.info("segment %s: %d windows, %d slides", key, len(slicer), len(plan.slides) if plan else 0)
        scores = coinc.detector_scores(slicer, model, args.batch_size, fe)
        if args.verbose:                                 # what a threshold is chosen by (one extra copy of the scores)
            q = np.percentile(scores.cpu().numpy(), [50.0, 90.0, 99.0, 100.0], axis=1)
            for g, r in enumerate(rows):
                logging.info("segment %s %s logits: median %.4f, 90th percentile %.4f, 99th %.4f, max %.4f", key, DETECTORS[r],
                             *q[:, g])
        fg[key], bg[key] = coinc.search_segment(slicer, model, args.trigger_threshold, args.cluster_threshold, args.coinc_window,
                                                plan, scores=scores)
    keys = sorted(fg)
    cat = lambda parts, j, dtype: np.concatenate([p[j] for p in parts]) if parts else np.zeros((0,), dtype)  # noqa: E731
    foreground = {n: cat([fg[k] for k in keys], j, np.float64) for j, n in enumerate(("time", "stat", "var"))}
    background = None
    if S > 0:
        background = background_dict([cat([bg[k] for k in keys], j, np.int32 if j == 3 else np.float64) for j in range(4)],
                                     slide_live)
    return foreground, background


def main(argv=None) -> int:
    start = t.time()
    args = parse_args(argv)
    logging.basicConfig(level=logging.INFO if args.verbose else logging.WARN, format="%(levelname)s | %(asctime)s: %(message)s",
                        datefmt="%d.%m.%Y %H:%M:%S")
    rows = check_args(args, int(os.environ.get("WORLD_SIZE", "1")))
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("run_coinc_search: no GPU -- gw_whisper_amd has no CPU fallback")
    device = torch.device("cuda", int(os.environ.get("LOCAL_RANK", "0")))
    torch.cuda.set_device(device)
    foreground, background = search(args, device, rows)
    ri.write_result(args.outputfile, foreground)
    what = "coincidences" if len(rows) == 2 else f"{DETECTORS[rows[0]]} events"
    print(f"{len(foreground['time'])} {what} -> {args.outputfile}")
    if background is not None:
        ri.write_result(args.slides_output, background)
        print(f"{len(background['time'])} slid coincidences in {float(background['livetime']):.1f} s of live time -> "
              f"{args.slides_output}")
    print(f"Total execution time: {t.time() - start:.2f} seconds")
    sys.stdout.flush()
    return 0


if __name__ == "__main__":
    sys.exit(main())
