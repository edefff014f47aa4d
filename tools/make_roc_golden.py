#!/usr/bin/env python3
"""Write tests/golden/roc_bootstrap.npz by running the REFERENCE's own code on scikit-learn: the metric statements of
``evaluate`` (``roc_auc_score``, ``roc_curve``) and ``bootstrap_roc_curve`` are taken out of
``Signal_vs_Noise/src/evaluation.py`` with ``ast`` where the file lies and executed; the module itself is never imported
(its imports need packages and a display this project does not), and nothing of its text is stored: only the INPUTS this
tool draws and the OUTPUTS the reference computes.

Per case (N, R) the file holds the scores, the labels, the seed, R, ``mean_tpr`` / ``std_tpr`` of the band, an XOR and a
sum checksum of the [R, N] matrix of resample indices (the tests regenerate the matrix from the seed), ``roc_curve``'s
fpr / tpr with and without ``drop_intermediate`` and ``roc_auc_score``.  Every warning is an error: a degenerate resample
(one class only) would stop the tool.

usage: make_roc_golden.py [--reference DIR] [--out FILE]"""
import argparse
import ast
import os
import sys
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import roc_helpers as rh  # noqa: E402

SEPS = (1.0, 2.0, 3.0, 4.0)
SEEDS = (1001, 1002, 1003, 1004)


def reference_code(path):
    """(namespace holding the reference's bootstrap_roc_curve, code object of evaluate's two metric statements)."""
    import sklearn.metrics as skm
    from sklearn.utils import resample
    tree = ast.parse(open(path).read(), filename=path)
    funcs = {n.name: n for n in tree.body if isinstance(n, ast.FunctionDef)}
    ns = {"np": np, "resample": resample, "roc_curve": skm.roc_curve, "roc_auc_score": skm.roc_auc_score}
    exec(compile(ast.fix_missing_locations(ast.Module(body=[funcs["bootstrap_roc_curve"]], type_ignores=[])), path, "exec"), ns)

    def is_metric(stmt):
        return isinstance(stmt, ast.Assign) and isinstance(stmt.value, ast.Call) and \
            getattr(stmt.value.func, "id", "") in ("roc_auc_score", "roc_curve")
    metric = [s for s in funcs["evaluate"].body if is_metric(s)]
    assert len(metric) == 2, "evaluate() no longer has one roc_auc_score and one roc_curve statement"
    return ns, compile(ast.fix_missing_locations(ast.Module(body=metric, type_ignores=[])), path, "exec")


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reference", default="/root/reference")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "roc_bootstrap.npz"))
    args = ap.parse_args()
    import sklearn
    import sklearn.metrics as skm
    from sklearn.utils import resample
    ns, metric = reference_code(os.path.join(args.reference, "Signal_vs_Noise", "src", "evaluation.py"))
    warnings.simplefilter("error")
    out = {"cases": np.asarray(rh.CASES, np.int64), "sklearn_version": np.asarray(sklearn.__version__),
           "numpy_version": np.asarray(np.__version__)}
    for ci, ((n, R), sep, seed) in enumerate(zip(rh.CASES, SEPS, SEEDS)):
        scores, labels = rh.saturating_scores(n, sep, seed)
        drawn = []

        def recording_resample(*arrays):
            # the reference's draw, then the same draw again on arange(n): the indices it used
            state = np.random.get_state()
            res = resample(*arrays)
            after = np.random.get_state()
            np.random.set_state(state)
            drawn.append(resample(np.arange(n)))
            np.random.set_state(after)
            return res
        ns["resample"] = recording_resample
        np.random.seed(seed)
        grid, mean_tpr, std_tpr = ns["bootstrap_roc_curve"](labels, scores, num_bootstrap=R)
        assert np.array_equal(grid, rh.GRID)
        idx = np.stack(drawn).astype(np.int64)
        assert np.array_equal(idx, rh.draw_indices(seed, R, n)), "resample() does not draw randint(0, n, size=n) per replicate"
        env = {"all_labels": labels, "all_raw_preds": scores, "roc_curve": skm.roc_curve, "roc_auc_score": skm.roc_auc_score}
        exec(metric, env)
        fpr_all, tpr_all, _ = skm.roc_curve(labels, scores, drop_intermediate=False)
        xor, total = rh.checksums(idx)
        out.update({f"c{ci}_scores": scores, f"c{ci}_labels": labels.astype(np.uint8), f"c{ci}_seed": np.int64(seed),
                    f"c{ci}_R": np.int64(R), f"c{ci}_mean_tpr": mean_tpr, f"c{ci}_std_tpr": std_tpr,
                    f"c{ci}_idx_xor": np.int64(xor), f"c{ci}_idx_sum": np.int64(total),
                    f"c{ci}_fpr_drop": env["fpr"], f"c{ci}_tpr_drop": env["tpr"], f"c{ci}_fpr_all": fpr_all,
                    f"c{ci}_tpr_all": tpr_all, f"c{ci}_auc": np.float64(env["auc"])})
        print(f"case {ci}: N={n} R={R} auc={float(env['auc']):.6f} vertices {len(fpr_all)} / {len(env['fpr'])} "
              f"ties at 0/1: {int((scores == 0).sum())}/{int((scores == 1).sum())}")
    np.savez_compressed(args.out, **out)
    print(f"wrote {args.out}: {os.path.getsize(args.out)} bytes")


if __name__ == "__main__":
    main()
