#!/usr/bin/env python3
"""Counterpart of the reference's ``MLGWSC-1/evaluate.py`` command line on ``gw_whisper_amd``: the events of a search on
the foreground and the background data set plus the injection file in -> the false-alarm rate and the sensitive distance
out, with the sorting, matching, counting and the volumes on the device (``gw_whisper_amd/search_score.py``).

Same flags as the reference (``--injection-file --foreground-events --foreground-files --background-events --output-file
--verbose --force``), the same 30 s padding at both ends of every segment, the same "contains no injections" error, the
same refusal to overwrite without ``--force``, the same sixteen output datasets.  ``--background-duration SECONDS`` (or
the ``livetime`` dataset of a single background file, which ``run_inference.py --slides-output`` writes) counts ``far``
per that much background instead of the foreground's duration: a time-slide background is longer than the data.  ``chirp_distance`` weighting is on when
the injection file has the ``chirp_distance`` key.  Files as ``run_inference.py`` reads and writes them, so its event
files are accepted without conversion: HDF5 in the reference's layout when ``h5py`` is importable, otherwise the ``.npz``
twin of the same layout (foreground files: ``<detector>/<key>`` arrays plus ``<key>/start_time`` and ``<key>/delta_t``
scalars; every other file: one array per dataset).  The output file must end in ``.hdf`` as in the reference (or in
``.npz``); without ``h5py`` the datasets go to ``<output>.npz``.
"""
from __future__ import annotations

import argparse
import logging
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

PADDING_START, PADDING_END = 30, 30


def parse_args(argv=None):
    p = argparse.ArgumentParser(description="False-alarm rate and sensitive distance of a search (MI355X).")
    p.add_argument("--injection-file", type=str, required=True, help="The injections of the foreground data set.")
    p.add_argument("--foreground-events", type=str, nargs="+", required=True, help="Events of the search on the foreground.")
    p.add_argument("--foreground-files", type=str, nargs="+", required=True, help="The analysed foreground data files.")
    p.add_argument("--background-events", type=str, nargs="+", required=True, help="Events of the search on the background.")
    p.add_argument("--output-file", type=str, required=True, help="Output file (must end in .hdf, or .npz).")
    p.add_argument("--background-duration", type=float, default=None,
                   help="Seconds of background the background events were found in (default: the `livetime` dataset of a "
                        "single background file, as run_inference.py --slides-output writes it; otherwise the foreground's "
                        "duration, as in the reference).")
    p.add_argument("--verbose", action="store_true", help="Print update messages.")
    p.add_argument("--force", action="store_true", help="Overwrite existing files.")
    return p.parse_args(argv)


# ---------------------------------------------------------------------------------------------- files
def _have_h5py():
    try:
        import h5py  # noqa: F401
        return True
    except ImportError:
        return False


def resolve(path: str) -> str:
    """The file to open for ``path``: itself, or -- without h5py -- the ``.npz`` twin ``run_inference.py`` wrote beside it."""
    if path.endswith(".npz") or _have_h5py():
        return path
    if os.path.isfile(path + ".npz"):
        return path + ".npz"
    raise IOError(f"{path}: h5py is not importable and there is no {path}.npz beside it")


def output_path(path: str) -> str:
    return path if path.endswith(".npz") or _have_h5py() else path + ".npz"


def read_arrays(path: str) -> dict:
    """Every top-level dataset of a flat file (events, injections) as numpy arrays."""
    path = resolve(path)
    if path.endswith(".npz"):
        with np.load(path) as z:
            return {k: z[k] for k in z.files}
    import h5py
    with h5py.File(path, "r") as fp:
        return {k: fp[k][()] for k in fp.keys() if isinstance(fp[k], h5py.Dataset)}


def read_segment_list(path: str):
    """[(start_time, n_samples, delta_t)] of the segments of the first detector of a foreground file."""
    path = resolve(path)
    segs = []
    if path.endswith(".npz"):
        with np.load(path) as z:
            names = [k for k in z.files if not k.endswith(("/start_time", "/delta_t"))]
            det = names[0].split("/", 1)[0]
            for k in names:
                d, key = k.split("/", 1)
                if d == det:
                    segs.append((float(z[f"{key}/start_time"]), int(z[k].shape[-1]), float(z[f"{key}/delta_t"])))
        return segs
    import h5py
    with h5py.File(path, "r") as fp:
        det = list(fp.keys())[0]
        for key in fp[det].keys():
            ds = fp[f"{det}/{key}"]
            segs.append((ds.attrs["start_time"], len(ds), ds.attrs["delta_t"]))
    return segs


def read_events(paths):
    """[3, n] (time, stat, var) of one or more event files (evaluate.py:356-362)."""
    parts = []
    for path in paths:
        a = read_arrays(path)
        parts.append(np.vstack([a["time"], a["stat"], a["var"][:len(a["time"])]]).astype(np.float64))
    return np.concatenate(parts, axis=-1)


def write_result(path: str, arrays: dict):
    path = output_path(path)
    if path.endswith(".npz"):
        np.savez(path, **arrays)
        return
    import h5py
    with h5py.File(path, "w") as fp:
        for k, v in arrays.items():
            fp.create_dataset(k, data=np.array(v))


# ---------------------------------------------------------------------------------------------- main
def main(argv=None) -> int:
    args = parse_args(argv)
    logging.basicConfig(format="%(levelname)s | %(asctime)s: %(message)s", level=logging.INFO if args.verbose else logging.WARN,
                        datefmt="%d-%m-%Y %H:%M:%S")
    if os.path.splitext(args.output_file)[1] not in (".hdf", ".npz"):
        raise ValueError("The output file must have the extension `.hdf` (or `.npz`).")
    if os.path.isfile(output_path(args.output_file)) and not args.force:
        raise IOError(f"The file {output_path(args.output_file)} already exists. Set the flag `force` to overwrite it.")

    from gw_whisper_amd import search_score
    logging.info("Finding injections contained in data")
    inj = read_arrays(args.injection_file)
    segments = [s for path in args.foreground_files for s in read_segment_list(path)]
    dur, idxs = search_score.find_injection_times(segments, inj["tc"], padding_start=PADDING_START, padding_end=PADDING_END)
    if np.sum(idxs) == 0:
        raise RuntimeError("The foreground data contains no injections! Probably a too small section of data was generated. "
                           f"Please make sure to generate at least {PADDING_START + PADDING_END + 24} seconds of data. "
                           "Otherwise a sensitive distance cannot be calculated.")
    injparams = {k: np.asarray(inj[k])[idxs] for k in ("tc", "distance", "mass1", "mass2")}
    use_chirp_distance = "chirp_distance" in inj

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("run_search_evaluate: no GPU -- gw_whisper_amd has no CPU fallback")
    logging.info("Reading foreground events from %s", args.foreground_events)
    fg_events = read_events(args.foreground_events)
    logging.info("Reading background events from %s", args.background_events)
    bg_events = read_events(args.background_events)
    bg_dur = args.background_duration
    if bg_dur is None and len(args.background_events) == 1:
        live = read_arrays(args.background_events[0]).get("livetime")
        if live is not None:
            bg_dur = float(np.asarray(live).reshape(-1)[0])
            logging.info("Background duration %.1f s from the livetime dataset of %s", bg_dur, args.background_events[0])
    stats = search_score.get_stats(fg_events, bg_events, injparams, duration=dur, chirp_distance=use_chirp_distance,
                                   background_duration=bg_dur)
    logging.info("Writing output to %s", output_path(args.output_file))
    write_result(args.output_file, stats)
    return 0


if __name__ == "__main__":
    sys.exit(main())
