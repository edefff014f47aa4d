"""The bf16 backward reductions on exact-integer operands, bit for bit (tests/exact_int.py holds the operand rules, the
integer references and the table of cases; tests/test_exact_int_host.py proves on the CPU that every case is exact, free
of the summation order, and that the comparison catches a lost or doubled row, a lost 16-byte chunk, swapped rows, a
shifted column scale, a missing accumulate and a doubled alpha).  ``gemm_wgrad`` (k_wgrad_bf16, k_wgrad_reduce),
``dora_grads`` on every route of launch_dora_grads (k_dora_grads at d 128 / 1024 / 1280, k_dora_grads_mfma + k_dora_reduce
at 384 / 512 / 768), ``dora_grads_multi``, ``adapter_grads`` (k_adapter_uv / _outer / _reduce) and the dbeta of
``layernorm_param_grads`` (k_ln_gb_partial / _reduce).  Every assertion is ``np.array_equal`` on the uint32 view against the
reference cast to fp32; every case runs twice and the two runs must be equal too.  No tolerance anywhere: a mismatch is a
kernel or launch-plan bug, and the message names the tiles it falls in.  Needs an MI355X."""

import numpy as np
import pytest

from tests import exact_int as xi

pytestmark = pytest.mark.gpu

# tile edges of the launch plans along each axis of an output, for the mismatch report
BLOCKS = {"dw": (128, 128), "db": (128,), "dA": (32, 128), "dB": (128, 32), "dm": (128,), "dbeta": (128,)}


@pytest.fixture(scope="module")
def T():
    import torch
    assert torch.cuda.is_available()
    return torch


def _bf(T, a):
    return T.from_numpy(np.ascontiguousarray(a)).cuda().to(T.bfloat16)


def _f(T, a):
    return T.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def _np(outs):
    return {k: v.cpu().numpy() for k, v in outs.items()}


def _check(case, label, runs, ref, note=""):
    """runs: the outputs {name: fp32 array} of two identical calls."""
    lines = []
    for name, want in ref.items():
        for i, run in enumerate(runs):
            msg = xi.report(f"{name} (run {i})", run[name], want, BLOCKS[name])
            if msg:
                lines.append(msg)
        a, b = (np.ascontiguousarray(r[name]).view(np.uint32) for r in runs)
        if not np.array_equal(a, b):
            lines.append(f"{name}: two identical calls differ in {int((a != b).sum())} elements")
    assert not lines, f"{case.id} {label} {note}\n" + "\n".join(lines)


def _view(T, flat, lay):
    off, ld, rows, width = lay
    return flat.as_strided((rows, width), (ld, 1), off)


@pytest.mark.parametrize("case", xi.cases("wgrad"), ids=[c.id for c in xi.cases("wgrad")])
def test_gemm_wgrad_exact(T, gww, case):
    from gw_whisper_amd import ops
    o = xi.wgrad_operands(case)
    ref = xi.reference("wgrad", xi.wgrad_effective(o))
    dy, x = _view(T, _bf(T, o["dy_flat"]), o["dy_lay"]), _view(T, _bf(T, o["x_flat"]), o["x_lay"])
    kw = {}
    if o["dy_lay"][2] != o["M"]:
        kw["rows"] = o["M"]
    if o["x_lay"][1] < o["x_lay"][3]:          # overlapping im2col rows
        kw["k"] = o["x_lay"][3]
    runs = []
    for _ in range(2):
        dw = None if o["dw0"] is None else _f(T, o["dw0"])
        db = _f(T, o["db0"]) if o["db0"] is not None else (True if o["want_db"] else None)
        dw, db = ops.gemm_wgrad(dy, x, dw=dw, db=db, alpha=o["alpha"], **kw)
        assert (db is None) == (not o["want_db"])
        runs.append(_np({"dw": dw, **({"db": db} if db is not None else {})}))
    tn, tk, slices, rows = xi.wgrad_plan(o["M"], case.N, case.K)
    _check(case, "", runs, ref, f"plan: {tn} x {tk} tiles, {slices} slices of {rows} rows")


def _proj_args(T, pr):
    return dict(bias_st=_f(T, pr["bias"]), yscale=pr["yscale"], scaling=pr["scaling"], A=_f(T, pr["A"]), B=_f(T, pr["B"]),
                mag=_f(T, pr["mag"]), nrm=_f(T, pr["nrm"]))


def _names(out):
    return dict(zip(("dA", "dB", "dm"), out))


@pytest.mark.parametrize("case", xi.cases("dora"), ids=[c.id for c in xi.cases("dora")])
def test_dora_grads_exact(T, gww, case):
    """r = 8 on [d, d]: plain [M, d] buffers and the q / k / v sections of a packed [M, 3 d] pair."""
    from gw_whisper_amd import ops
    o = xi.adapter_operands(case)
    ref = xi.reference("dora", xi.adapter_effective(o))
    x, dy, y = _bf(T, o["x_buf"]), _bf(T, o["dy_buf"]), _bf(T, o["y_buf"])
    a = _proj_args(T, o)
    runs = [_np(_names(ops.dora_grads(x, dy, y, a["bias_st"], a["yscale"], a["scaling"], a["A"], a["B"], a["mag"], a["nrm"],
                                      col_off=o["col_off"]))) for _ in range(2)]
    rt = 32 if case.d_in <= 768 else (16 if case.d_in <= 1024 else 8)
    _check(case, "", runs, ref, f"row tiles of {rt}: {-(-case.M // rt)}, the last one {case.M - (case.M - 1) // rt * rt} rows")


@pytest.mark.parametrize("case", xi.cases("dora_multi"), ids=[c.id for c in xi.cases("dora_multi")])
def test_dora_grads_multi_exact(T, gww, case):
    """Up to three projections that share x, in either order of their sections, each with its own factors; and each
    projection equal, bit for bit, to the single-projection call on the same section."""
    from gw_whisper_amd import ops
    o = xi.multi_operands(case)
    x, dy, y = _bf(T, o["x_buf"]), _bf(T, o["dy_buf"]), _bf(T, o["y_buf"])
    args = [_proj_args(T, pr) for pr in o["proj"]]
    lists = [[a[k] for a in args] for k in ("bias_st", "yscale", "scaling", "A", "B", "mag", "nrm")]
    both = [ops.dora_grads_multi(x, dy, y, o["col_off"], *lists) for _ in range(2)]
    for p, a in enumerate(args):
        ref = xi.reference("dora", xi.adapter_effective(o, p))
        runs = [_np(_names(run[p])) for run in both]
        _check(case, f"projection {p} at column {o['col_off'][p]}", runs, ref)
        single = _np(_names(ops.dora_grads(x, dy, y, a["bias_st"], a["yscale"], a["scaling"], a["A"], a["B"], a["mag"], a["nrm"],
                                           col_off=o["col_off"][p])))
        for name in ref:
            assert np.array_equal(single[name].view(np.uint32), runs[0][name].view(np.uint32)), (case.id, p, name)


@pytest.mark.parametrize("case", xi.cases("adapter"), ids=[c.id for c in xi.cases("adapter")])
def test_adapter_grads_exact(T, gww, case):
    """Square, fc1 and fc2 shapes, ranks on both sides of RP = 32 / 64 and of the zero-padded ranks, strided rows, plain
    LoRA (mag = nrm = 1) and DoRA factors."""
    from gw_whisper_amd import ops
    o = xi.adapter_operands(case)
    ref = xi.reference("adapter", xi.adapter_effective(o))
    x = _bf(T, o["x_buf"])[:, o["x_off"]:o["x_off"] + case.d_in]
    sl = slice(o["col_off"], o["col_off"] + case.d_out)
    dy, y = _bf(T, o["dy_buf"])[:, sl], _bf(T, o["y_buf"])[:, sl]
    a = _proj_args(T, o)
    runs = [_np(_names(ops.adapter_grads(x, dy, y, a["bias_st"], a["yscale"], a["scaling"], a["A"], a["B"], a["mag"], a["nrm"])))
            for _ in range(2)]
    tiles = -(-case.M // 32)
    n_rs = max(1, min(-(-1024 // ((case.d_in + case.d_out) // 128)), tiles, 128))
    _check(case, "", runs, ref, f"{tiles} row tiles of 32 over {n_rs} row splits, RP {32 if case.r <= 32 else 64}")


@pytest.mark.parametrize("case", xi.cases("ln"), ids=[c.id for c in xi.cases("ln")])
def test_layernorm_dbeta_exact(T, gww, case):
    """dbeta = dbeta0 + sum_m dy on integer dy (fp32 and bf16); dgamma keeps its own test and is only held to be
    reproducible here."""
    from gw_whisper_amd import ops
    o = xi.ln_operands(case)
    ref = xi.reference("ln", xi.ln_effective(o))
    x = T.from_numpy(o["x"]).cuda().float()
    dy = T.from_numpy(o["dy"]).cuda().float()
    if case.dy == "bf16":
        dy = dy.bfloat16()
    runs, gammas = [], []
    for _ in range(2):
        dgamma, dbeta = ops.layernorm_param_grads(x, dy, dbeta=_f(T, o["dbeta0"]))
        runs.append(_np({"dbeta": dbeta}))
        gammas.append(dgamma)
    P = min(max(-(-case.M // 64), 1), 512)
    _check(case, "", runs, ref, f"{P} workgroups of 4 rows, {-(-case.M // (4 * P))} trips")
    assert T.equal(gammas[0], gammas[1])
