#!/usr/bin/env python3
"""Glitch scan of continuous strain: what a trained glitch model (``run_glitch_train.py``, or the reference's
``Glitch_classification/src/train.py``) finds in a stretch of detector data, when, and how confidently.  The reference
has no such program (its ``evaluate.py`` takes pre-cut, labelled 1 s segments); this is to the glitch model what
``run_inference.py`` is to the search and ``run_real_events.py`` to signal-vs-noise.

Input and output as ``run_inference.py`` (``inputfile outputfile``, its segment layout and ``write_result``: HDF5 when
``h5py`` is importable, the ``.npz`` twin otherwise); every detector of every segment is scanned as its own series, since
a glitch model is single-detector.  ``--white``: the data are already conditioned as the training data were; otherwise
``glitch_scan.condition`` runs first (whitening with 4 s segments and a 4 s filter, 30 Hz high-pass of order 512; parity
with PyCBC unpinned).  The model flags are those of ``run_glitch_evaluate.py``; ``--classes`` is the
``<model_name>_classes.json`` ``run_glitch_train.py`` writes (without it and without weights: seeded random parameters
and ``--synthetic-classes`` generic names, for dry runs).

Output datasets, one entry per event, segment after segment (longest first), detector after detector, by first window:
``segment`` (index into ``segment_keys``) ``detector`` ``class`` ``n_windows`` ``time_start`` ``time_end`` ``time_peak``
``prob``, plus ``class_names`` and ``segment_keys``.  ``--window-output FILE``: per segment ``<key>/window_class``,
``<key>/window_prob``, ``<key>/window_time`` ``[detectors, windows]``.  One rank; segments are independent, so split the
input to use more GPUs.
"""
from __future__ import annotations

import argparse
import json
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

from run_inference import DETECTORS, read_segments, write_result  # noqa: E402  (the segment layout and the writer)

EVENT_FIELDS = ("detector", "class", "n_windows", "time_start", "time_end", "time_peak", "prob")


def build_parser():
    from gw_whisper_amd.glitch import DEFAULT_LORA_TARGETS
    p = argparse.ArgumentParser(description="Glitch scan of continuous strain (MI355X path).")
    p.add_argument("inputfile", type=str, help="Input HDF5 / .npz (ignored with --synthetic).")
    p.add_argument("outputfile", type=str, help="Output HDF5 / .npz (must not exist unless --force).")
    p.add_argument("--verbose", action="store_true")
    p.add_argument("--force", action="store_true", help="Overwrite existing output files.")
    p.add_argument("--white", action="store_true", help="Input is already conditioned (otherwise glitch_scan.condition runs).")
    p.add_argument("--encoder", type=str, default="tiny", help="Whisper encoder size")
    p.add_argument("--method", type=str, choices=["LoRA", "DoRA", "full_finetune"], default="DoRA")
    p.add_argument("--lora_weights_path", type=str, default=None, help="Encoder weights of run_glitch_train.py (.pth)")
    p.add_argument("--dense_weights_path", type=str, default=None, help="Head weights of run_glitch_train.py (.pth)")
    p.add_argument("--lora_rank", type=int, default=8)
    p.add_argument("--lora_alpha", type=int, default=32)
    p.add_argument("--precision", choices=("bf16", "fp32"), default="bf16")
    p.add_argument("--encoder-weights", type=str, default=None, help="HF WhisperEncoder state_dict (.pth / .safetensors)")
    p.add_argument("--lora-targets", type=str, nargs="+", default=list(DEFAULT_LORA_TARGETS), metavar="PATTERN")
    p.add_argument("--classes", type=str, default=None, help="<model_name>_classes.json of run_glitch_train.py")
    p.add_argument("--ignore-class", type=str, nargs="+", default=[], metavar="NAME", help="Classes that never trigger.")
    p.add_argument("--prob-threshold", type=float, default=0.5)
    p.add_argument("--gap", type=float, default=0.35, help="Seconds without a trigger of a class that end its event.")
    p.add_argument("--step-size", type=float, default=0.1)
    p.add_argument("--batch-size", type=int, default=256)
    p.add_argument("--window-output", type=str, default=None, metavar="FILE", help="Also write every window's class, probability and time.")
    p.add_argument("--synthetic", type=float, default=None, metavar="SECONDS", help="Seconds of synthetic conditioned noise instead of inputfile.")
    p.add_argument("--synthetic-classes", type=int, default=11)
    p.add_argument("--seed", type=int, default=42)
    return p


def parse_args(argv=None):
    return build_parser().parse_args(argv)


def check_outputs(args):
    """Refuse to overwrite without ``--force`` (before any work, as ``run_inference.py`` does)."""
    if os.path.isfile(args.outputfile) and not args.force:
        raise RuntimeError("Output file exists. Use --force to overwrite.")
    if args.window_output is not None and os.path.isfile(args.window_output) and not args.force:
        raise RuntimeError("Window file exists. Use --force to overwrite.")


def load_classes(args):
    if args.classes:
        with open(args.classes) as f:
            classes = [str(c) for c in json.load(f)]
    else:
        from gw_whisper_amd import synth
        classes = list(synth.glitch_class_names(args.synthetic_classes))
    unknown = [c for c in args.ignore_class if c not in classes]
    if unknown:
        raise SystemExit(f"run_glitch_scan: --ignore-class {unknown} not among the classes {classes}")
    return classes


def name_array(names):
    """Names as fixed-width UTF-8 byte strings: the one string type both HDF5 and ``.npz`` store as they are."""
    return np.array([str(n).encode("utf-8") for n in names], dtype="S")


def pack_events(results, keys, classes):
    """The output arrays from the per-segment event dicts of ``GlitchScanner.scan`` (in the order of ``keys``)."""
    out = {"segment": np.concatenate([np.full((len(results[k]["class"]),), i, np.int32) for i, k in enumerate(keys)]
                                     or [np.zeros((0,), np.int32)])}
    for f in EVENT_FIELDS:
        parts = [results[k][f] for k in keys]
        out[f] = np.concatenate(parts) if parts else np.zeros((0,))
    out["class_names"] = name_array(classes)
    out["segment_keys"] = name_array(keys)
    return out


def main(argv=None) -> int:
    start = t.time()
    args = parse_args(argv)
    logging.basicConfig(level=logging.INFO if args.verbose else logging.WARN,
                        format="%(levelname)s | %(asctime)s: %(message)s", datefmt="%d.%m.%Y %H:%M:%S")
    check_outputs(args)
    if int(os.environ.get("WORLD_SIZE", "1")) > 1:
        raise SystemExit("run_glitch_scan: one rank only; segments are independent, so split the input by segment instead")
    classes = load_classes(args)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("run_glitch_scan: no GPU -- gw_whisper_amd has no CPU fallback")
    device = torch.device("cuda", 0)
    from gw_whisper_amd import glitch
    from gw_whisper_amd.glitch_scan import GlitchScanner
    model = glitch.build_model(args.encoder, len(classes), args.method, args.lora_rank, args.lora_alpha, args.precision,
                               args.lora_targets, args.encoder_weights, args.seed, device)
    if args.lora_weights_path:
        model.encoder.load_state_dict(torch.load(args.lora_weights_path, map_location=device))
    if args.dense_weights_path:
        model.classifier.load_state_dict(torch.load(args.dense_weights_path, map_location=device))
    scanner = GlitchScanner(model, classes)
    if args.synthetic is not None:
        rng = np.random.default_rng(args.seed)
        n = int(round(args.synthetic * 2048))
        segs = {"synthetic": (rng.standard_normal((len(DETECTORS), n)).astype(np.float32), 1.0e9, 1.0 / 2048)}
        white = True
    else:
        segs, white = read_segments(args.inputfile), args.white
    keys = sorted(segs, key=lambda k: segs[k][0].shape[1], reverse=True)
    results, windows = {}, {}
    for key in keys:
        strain, st, dt = segs[key]
        r = scanner.scan(strain, start_time=st, delta_t=dt, step_size=args.step_size, batch_size=args.batch_size,
                         prob_threshold=args.prob_threshold, gap=args.gap, ignore=args.ignore_class, conditioned=white,
                         return_windows=args.window_output is not None, device=device)
        logging.info("segment %s: %d events", key, len(r["class"]))
        results[key] = r
        if args.window_output is not None:
            for f in ("window_class", "window_prob", "window_time"):
                windows[f"{key}/{f}"] = r[f]
    write_result(args.outputfile, pack_events(results, keys, classes))
    if args.window_output is not None:
        windows["class_names"] = name_array(classes)
        write_result(args.window_output, windows)
    print(f"{sum(len(r['class']) for r in results.values())} events in {len(keys)} segment(s); "
          f"total execution time: {t.time() - start:.2f} seconds")
    sys.stdout.flush()
    return 0


if __name__ == "__main__":
    sys.exit(main())
