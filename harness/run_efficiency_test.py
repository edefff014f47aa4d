#!/usr/bin/env python3
"""Counterpart of the reference's ``Signal_vs_Noise/Efficiency_test/src/test_network.py`` on the MI355X path: the trained
network over long stretches of test data, one ``[n, 2]`` output per input file.

Same flags as the reference (``--input-dir --output-dir --log-file --batch-size --device --remove-softmax --verbose
--debug``); the two state-dict paths the reference hard-codes are ``--lora-weights`` (the adapter directory or file
``PeftModel.from_pretrained`` reads) and ``--dense-layers`` (the ``.pth`` of the head), and the encoder's size, weights and
arithmetic are given as in run_efficiency_estimate.py (``--encoder --encoder-weights --precision --seed``).

Per input file: ``H1/data`` [n, 2048] is read, uploaded once, resampled to 16 kHz (``inference.resample``), turned into
log-mel features on the device, run through the encoder's last token and the detection head
(``trigger_stats.score_windows``: the softmax pair, or ``(z0 - z1, z1 - z0)`` with ``--remove-softmax``), and the
``[n, 2]`` dataset ``data`` is written to the file of the same name in ``--output-dir``.  The reference's line
``Successfully saved output to <path>`` is appended to ``--log-file``, and files the log already names are skipped, so an
interrupted run resumes.  ``--batch-size`` 0 means a whole file at once, as in the reference.  Files are HDF5 when ``h5py``
is importable, otherwise the ``.npz`` twin (``<name>`` or ``<name>.npz`` with an array ``H1/data``; the output goes to
``<name>.npz``), as in run_search_evaluate.py.
"""
from __future__ import annotations

import argparse
import logging
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if p not in sys.path:
        sys.path.insert(0, p)

from run_search_evaluate import _have_h5py, output_path, write_result  # noqa: E402

SAVED = "Successfully saved output to"


def build_parser():
    p = argparse.ArgumentParser(description="The network over the efficiency study's test data (MI355X path)")
    p.add_argument("--input-dir", required=True, type=str, help="The directory from which the files will be read.")
    p.add_argument("--output-dir", required=True, type=str, help="The directory in which the output files will be stored.")
    p.add_argument("--log-file", required=True, type=str, help="The log file naming the successfully processed files.")
    p.add_argument("--verbose", action="store_true", help="Print status updates while loading.")
    p.add_argument("--debug", action="store_true", help="Print debugging info")
    p.add_argument("--batch-size", type=int, default=0, help="Batch size, 0 means entire data files. Default: 0")
    p.add_argument("--device", type=str, default="cuda", help="Device to use for calculation.")
    p.add_argument("--remove-softmax", action="store_true", help="Replace the final softmax layer by a 'mutual subtraction layer'.")
    p.add_argument("--lora-weights", type=str, default=None, help="adapter weights (PeftModel.from_pretrained)")
    p.add_argument("--dense-layers", type=str, default=None, help="state dict of the dense layers (.pth)")
    p.add_argument("--encoder", type=str, default="tiny", help="encoder size")
    p.add_argument("--encoder-weights", type=str, default=None, help="HF WhisperEncoder state_dict (.pth / .safetensors)")
    p.add_argument("--precision", choices=("bf16", "fp32"), default="bf16", help="encoder arithmetic")
    p.add_argument("--seed", type=int, default=0)
    return p


def get_already_processed_files(log_file_path):
    """The output paths the log names (test_network.py:55-61); a missing log names none."""
    if not os.path.isfile(log_file_path):
        return []
    with open(log_file_path, "r") as log_file:
        return [line.split(SAVED)[-1].strip() for line in log_file if SAVED in line]


def read_windows(path):
    """``H1/data`` [n, 2048] of one input file as float32."""
    if path.endswith(".npz") or not _have_h5py():
        twin = path if path.endswith(".npz") else path + ".npz"
        with np.load(twin) as z:
            data = z["H1/data"]
    else:
        import h5py
        with h5py.File(path, "r") as fp:
            data = fp["H1/data"][:]
    data = np.ascontiguousarray(data, np.float32)
    if data.ndim != 2:
        raise ValueError(f"{path}: H1/data has shape {data.shape}, expected [n, samples]")
    return data


def input_files(input_dir):
    """The input files by the name their output gets: without h5py ``x.hdf.npz`` stands for ``x.hdf``."""
    names = []
    for fn in sorted(os.listdir(input_dir)):
        if os.path.isfile(os.path.join(input_dir, fn)):
            names.append(fn[:-4] if fn.endswith(".npz") and not _have_h5py() else fn)
    return names


def run(model, args, device):
    """Every file of ``--input-dir`` the log does not name yet; returns the output paths written."""
    import torch
    from gw_whisper_amd import trigger_stats
    file_list = input_files(args.input_dir)
    logging.info(f"Found {len(file_list)} files in the input directory")
    processed = get_already_processed_files(args.log_file)
    logging.info(f"Skipping {len(processed)} files that are already processed.")
    os.makedirs(args.output_dir, exist_ok=True)
    written = []
    for fn in file_list:
        fout = os.path.join(args.output_dir, fn)
        if fout in processed:
            logging.info(f"Skipping already processed file: {fn}")
            continue
        windows = torch.from_numpy(read_windows(os.path.join(args.input_dir, fn))).to(device)
        out = trigger_stats.score_windows(model, windows, args.batch_size).cpu().numpy()
        write_result(fout, {"data": out})
        with open(args.log_file, "a") as log_file:
            log_file.write(f"{SAVED} {fout}\n")
        logging.info(f"{SAVED} {fout}")
        written.append(output_path(fout))
    logging.info("Finished processing all files")
    return written


def main(argv=None) -> int:
    args = build_parser().parse_args(argv)
    log_level = logging.DEBUG if args.debug else (logging.INFO if args.verbose else logging.WARN)
    logging.basicConfig(format="%(levelname)s | %(asctime)s: %(message)s", level=log_level, datefmt="%d-%m-%Y %H:%M:%S")
    import torch
    from gw_whisper_amd import efficiency
    device = torch.device(args.device)
    assert device.type == "cuda" and torch.cuda.is_available(), \
        "run_efficiency_test.py needs an MI355X (gw_whisper_amd has no CPU path)"
    logging.info(f"Initializing network on device {args.device}")
    model = efficiency.build_model(args.encoder, 2, precision=args.precision, encoder_weights=args.encoder_weights,
                                   seed=args.seed, device=device, adapter_path=args.lora_weights)
    if args.dense_layers:
        model.classifier.load_state_dict(torch.load(args.dense_layers, map_location=device))
    model.eval()
    if args.remove_softmax:
        logging.info("Removing the softmax layer")
        efficiency.remove_softmax(model)
    run(model, args, device)
    return 0


if __name__ == "__main__":
    sys.exit(main())
