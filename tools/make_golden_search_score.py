#!/usr/bin/env python3
"""Write tests/golden/search_score.npz by running the REFERENCE's own code: ``find_closest_index``, ``mchirp`` and
``get_stats`` are taken out of ``MLGWSC-1/evaluate.py`` with ``ast`` where the file lies and executed; the module itself is
never imported (it imports ``h5py``, which this project does without), and nothing of its text is stored: only the
OUTPUTS the reference computes plus numpy's version.  The inputs are regenerated from seeds by
tests/search_score_helpers.py.

Per case and mode (plain / chirp-weighted) the file holds the reference's sixteen keys as ``c<case>_<mode>_<key>``; for the
largest case the three keys that are gathers of the inputs by stored indices (``fg-events``, ``true-positives``,
``false-positives``) are left out to keep the file under 1 MB.  For every case the tool asserts that the foreground event
times are pairwise distinct (the reference's argsort is not stable) and that at least one true positive exists.

usage: make_golden_search_score.py [--reference DIR] [--out FILE]"""
import argparse
import ast
import logging
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import search_score_helpers as sh  # noqa: E402

WANTED = ("find_closest_index", "mchirp", "get_stats")


def reference_functions(path):
    """The namespace holding the reference's three functions."""
    from tqdm import tqdm
    tree = ast.parse(open(path).read(), filename=path)
    funcs = {n.name: n for n in tree.body if isinstance(n, ast.FunctionDef)}
    missing = [n for n in WANTED if n not in funcs]
    assert not missing, f"{path} no longer defines {missing}"
    ns = {"np": np, "logging": logging, "tqdm": tqdm}
    exec(compile(ast.fix_missing_locations(ast.Module(body=[funcs[n] for n in WANTED], type_ignores=[])), path, "exec"), ns)
    return ns


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reference", default=os.path.join(os.path.dirname(ROOT), "reference"),
                    help="the reference checkout (default: the directory `reference` beside this repository)")
    ap.add_argument("--out", default=sh.GOLD)
    args = ap.parse_args()
    ns = reference_functions(os.path.join(args.reference, "MLGWSC-1", "evaluate.py"))
    out = {"numpy_version": np.asarray(np.__version__), "cases": np.asarray(sh.CASES, np.int64)}
    for ci in range(sh.HAND + 1):
        fg, bg, inj, duration = sh.case(ci)
        assert np.unique(fg[0]).size == fg.shape[1], f"case {ci}: foreground event times are not pairwise distinct"
        for mode in sh.MODES:
            res = ns["get_stats"](fg.copy(), bg.copy(), {k: v.copy() for k, v in inj.items()}, duration=duration,
                                  chirp_distance=mode == "chirp")
            assert len(res) == 16, sorted(res)
            assert len(res["true-positive-event-indices"]) >= 1, f"case {ci}: no true positive"
            for k, v in res.items():
                if ci == len(sh.CASES) - 1 and k in sh.BIG_KEYS:
                    continue
                out[f"c{ci}_{mode}_{k}"] = np.asarray(v)
            print(f"case {ci} [{mode}]: E={fg.shape[1]} B={bg.shape[1]} N={len(inj['tc'])} true positives "
                  f"{len(res['true-positive-event-indices'])} missed {len(res['missed-indices'])} "
                  f"max distance {float(np.max(res['sensitive-distance'])):.1f}")
    np.savez_compressed(args.out, **out)
    size = os.path.getsize(args.out)
    print(f"wrote {args.out}: {size} bytes")
    assert size <= 1 << 20, "the golden file exceeds 1 MiB"


if __name__ == "__main__":
    main()
