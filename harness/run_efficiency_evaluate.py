#!/usr/bin/env python3
"""Counterpart of the reference's ``Signal_vs_Noise/Efficiency_test/src/evaluate_test_data.py`` on ``gw_whisper_amd``: the
outputs ``run_efficiency_test.py`` wrote per file in -> triggers, clustered events, the false-alarm rate per month and the
sensitive distance out, with thresholding, clustering, matching, sorting and the ranking steps on the device
(``gw_whisper_amd/trigger_stats.py``).

Same flags and defaults as the reference (``--trigger-threshold 0.1 --cluster-tolerance 0.2 --event-tolerance 0.3
--injection-file --data-dir --force --delta-t 0.1 --start-time-offset 0.75 --duration --test-data-activation
--ranking-statistic --verbose --trigger-file-name --event-file-name --stats-file-name --load-triggers --load-events``), the
same errors (no overwriting without ``--force``, a ``linear`` ranking statistic on ``softmax`` data, a missing
``--duration`` when triggers or events are loaded) and the same datasets: ``data`` / ``trigger_values`` in the trigger
file, ``times`` / ``values`` in the event file, ``ranking`` / ``far`` / ``sens-frac`` / ``sens-dist`` / ``sens-vol`` /
``sens-vol-err`` in the statistics file.  Files are HDF5 when ``h5py`` is importable, otherwise the ``.npz`` twin of the
same layout (``<name>.npz``), as in run_search_evaluate.py.

File bookkeeping stays host Python (the reference's ``load_data`` and ``assemble_time_series``, :323-387), by this rule:
  * every regular file of ``--data-dir`` whose name parses and that holds a ``data`` dataset [n, 2] is one stretch; a file
    that does not (the trigger, event and statistics files of an earlier run among them) is skipped, as the reference's
    bare ``except`` skips it;
  * its start is ``int(fn.split('-')[1])``, plus 0.1 unless that is zero, plus ``--start-time-offset``;
  * its ranking statistic comes from the reference's own numpy expressions in the file's dtype: softmax of a linear pair
    ``exp0 / (exp0 + exp1)``, linear ``data.T[0] - data.T[1]``, softmax data ``data.T[0]``;
  * the long series is zero-filled fp64 with ``int((end - start) / dt) + 1`` samples, and the files are written into it in
    ascending start order, later files over earlier ones where they overlap: on the device one ordered copy per file on
    one stream;
  * epochs are integer nanoseconds (``trigger_stats.TimeSeries``, the project's stand-in for PyCBC's container).
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

from run_search_evaluate import output_path, read_arrays, write_result  # noqa: E402


def build_parser():
    p = argparse.ArgumentParser(description="Triggers, events, false-alarm rate and sensitivity of the test data (MI355X).")
    p.add_argument("--trigger-threshold", type=float, default=0.1, help="The threshold value to determine triggers.")
    p.add_argument("--cluster-tolerance", type=float, default=0.2,
                   help="The maximum distance (in seconds) between a trigger and the cluster boundaries.")
    p.add_argument("--event-tolerance", type=float, default=0.3,
                   help="The maximum time (in seconds) between an event and an injection of the same origin.")
    p.add_argument("--injection-file", required=True, type=str, help="The file containing the injections for this data.")
    p.add_argument("--data-dir", type=str, help="The directory containing the output of the network.")
    p.add_argument("--force", action="store_true", help="Overwrite existing output files.")
    p.add_argument("--delta-t", type=float, default=0.1, help="The time (in seconds) between two slices.")
    p.add_argument("--start-time-offset", type=float, default=0.75,
                   help="The time from the start of each window to the centre of the merger-time interval.")
    p.add_argument("--duration", type=float, help="The duration of the analysed data; required if triggers or events are loaded.")
    p.add_argument("--test-data-activation", choices=["linear", "softmax"], default="linear")
    p.add_argument("--ranking-statistic", choices=["softmax", "linear"], default="softmax")
    p.add_argument("--verbose", action="store_true", help="Print status updates.")
    p.add_argument("--trigger-file-name", type=str, default="triggers.hdf")
    p.add_argument("--event-file-name", type=str, default="events.hdf")
    p.add_argument("--stats-file-name", type=str, default="statistics.hdf")
    p.add_argument("--load-triggers", type=str, help="Start the analysis from the given trigger file.")
    p.add_argument("--load-events", type=str, help="Start the analysis from the given event file.")
    return p


# ---------------------------------------------------------------------------------------------- file bookkeeping
def get_start_time(fn):
    start = int(fn.split("-")[1])
    return start if start == 0 else start + 0.1


def ranking_statistic(data, data_activation="linear", target_activation="softmax"):
    """The series of one file from its [n, 2] outputs, in the reference's own expressions (evaluate_test_data.py:341-364)."""
    if data_activation == "linear":
        if target_activation == "linear":
            return data.T[0] - data.T[1]
        if target_activation == "softmax":
            exp0 = np.exp(data.T[0])
            exp1 = np.exp(data.T[1])
            return exp0 / (exp0 + exp1)
        raise RuntimeError(f"Unrecognized target_activation {target_activation}.")
    if data_activation == "softmax":
        if target_activation == "softmax":
            return data.T[0]
        if target_activation == "linear":
            raise ValueError("Cannot use target activation `linear` if data was generated with a softmax activation.")
        raise RuntimeError(f"Unrecognized target_activation {target_activation}.")
    raise RuntimeError(f"Unrecognized data_activation {data_activation}.")


def load_data(path, epoch_offset=0., delta_t=0.1, data_activation="linear", target_activation="softmax"):
    """The per-file series of ``path`` as ``trigger_stats.TimeSeries``, sorted by start time."""
    from gw_whisper_amd.trigger_stats import TimeSeries
    if not os.path.isdir(path):
        raise ValueError("Path {} for loading data not found.".format(path))
    out = []
    for fn in sorted(os.listdir(path)):
        full = os.path.join(path, fn)
        if not os.path.isfile(full):
            continue
        try:
            epoch = get_start_time(fn) + epoch_offset
            data = read_arrays(full)["data"]
        except Exception:                       # not a data file of this layout: skipped, as in the reference
            continue
        if data.ndim != 2 or data.shape[1] != 2:
            continue
        out.append(TimeSeries(ranking_statistic(data, data_activation, target_activation), delta_t=delta_t, epoch=epoch))
    return sorted(out, key=lambda ts: ts.start_time)


def _refuse_overwrite(path, what, force):
    if os.path.isfile(output_path(path)) and not force:
        raise IOError("Cannot overwrite {} file at {}. Set the flag --force if you want to overwrite the file anyways."
                      .format(what, output_path(path)))


def check_args(args):
    """The reference's flag errors (evaluate_test_data.py:456-478), before anything touches the device."""
    if args.ranking_statistic == "linear" and args.test_data_activation != "linear":
        raise ValueError("Can only use a linear ranking statistic if the test data was produced from a linear activation.")
    if args.load_triggers is None and args.load_events is None:
        if args.data_dir is None:
            raise ValueError("Must provide a directory from which to load the data when no triggers or events are loaded.")
    else:
        if args.data_dir is None:
            args.data_dir = "."
        if args.duration is None:
            raise ValueError("Duration required if data is not loaded.")
    return args


# ---------------------------------------------------------------------------------------------- main
def main(argv=None) -> int:
    args = check_args(build_parser().parse_args(argv))
    logging.basicConfig(format="%(levelname)s | %(asctime)s: %(message)s", level=logging.INFO if args.verbose else logging.WARN,
                        datefmt="%d-%m-%Y %H:%M:%S")
    trigger_path = os.path.join(args.data_dir, args.trigger_file_name)
    event_path = os.path.join(args.data_dir, args.event_file_name)
    stat_path = os.path.join(args.data_dir, args.stats_file_name)
    from_data = args.load_triggers is None and args.load_events is None
    if from_data:
        _refuse_overwrite(trigger_path, "trigger", args.force)
    if args.load_events is None:
        _refuse_overwrite(event_path, "event", args.force)
    _refuse_overwrite(stat_path, "statistics", args.force)
    inj = read_arrays(args.injection_file)
    inj_times, dist = np.asarray(inj["tc"], np.float64), np.asarray(inj["distance"], np.float64)

    import torch
    from gw_whisper_amd import trigger_stats as ts
    assert torch.cuda.is_available(), "run_efficiency_evaluate.py needs an MI355X (gw_whisper_amd has no CPU path)"

    def write_triggers(t, v):
        write_result(trigger_path, {"data": t, "trigger_values": v})
        logging.info("Wrote %d triggers to %s.", len(t), output_path(trigger_path))

    def write_events(t, v):
        write_result(event_path, {"times": t, "values": v})
        logging.info("Wrote %d events to %s.", len(t), output_path(event_path))

    if from_data:
        data = load_data(args.data_dir, epoch_offset=args.start_time_offset, delta_t=args.delta_t,
                         data_activation=args.test_data_activation, target_activation=args.ranking_statistic)
        logging.info("Loading complete. Loaded %d files.", len(data))
        series, dt, epoch = ts.assemble_time_series(data)
        duration = series.numel() * dt if args.duration is None else args.duration
        try:
            res = ts.evaluate(series, dt, epoch, inj_times, dist, args.trigger_threshold, args.cluster_tolerance,
                              args.event_tolerance, duration=duration)
        except ts.NoTruePositive as e:          # the reference has written both files when it dies
            if e.partial:
                write_triggers(*e.partial["triggers"])
                write_events(*e.partial["events"])
            raise
        write_triggers(*res["triggers"])
        write_events(*res["events"])
        stats = res["statistics"]
    else:
        if args.load_events is None:
            a = read_arrays(args.load_triggers)
            logging.info("Loaded %d triggers from %s", len(a["data"]), args.load_triggers)
            ev_t, ev_v = ts.events(a["data"], a["trigger_values"], args.cluster_tolerance)
            write_events(ev_t, ev_v)
        else:
            a = read_arrays(args.load_events)
            ev_t, ev_v = a["times"], a["values"]
        stats = ts.statistics(ev_t, ev_v, inj_times, dist, args.duration, args.event_tolerance)
    write_result(stat_path, {k: stats[k] for k in ts.STAT_KEYS})
    logging.info("Wrote statistics to %s.", output_path(stat_path))
    logging.info("Finished")
    return 0


if __name__ == "__main__":
    sys.exit(main())
