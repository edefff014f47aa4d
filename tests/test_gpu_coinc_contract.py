"""Memory contract of ``ops.coinc_slides`` and the three entry points of csrc/coinc.hip behind it (the pattern of
tests/test_gpu_time_slides_contract.py): the event lists, the shifts, the partner table, the per-workgroup counts, the
offsets and the ragged result are allocated under tests/guard.py's guard-band allocator; each case runs under the three fill
bytes and unguarded, must leave every band intact, write every element its contract says it writes -- all of ``offsets``,
the first ``min(total, cap_total)`` entries of the ragged buffers -- and give the same bits whatever lies outside."""

import numpy as np
import pytest

from gw_whisper_amd import coinc
from tests.guard import run_contract

from . import coinc_helpers as ch

pytestmark = pytest.mark.gpu

MODULES = ("gw_whisper_amd.ops",)
RAGGED = ("time", "stat", "dt", "idx0", "idx1")


@pytest.fixture(scope="module")
def T():
    import torch
    assert torch.cuda.is_available()
    return torch


@pytest.mark.parametrize("N,q,step", [(40, 70.0, 0.1), (600, 85.0, 204.0 / 2048.0)])
def test_coinc_slides_contract(T, gww, N, q, step):
    from gw_whisper_amd import ops
    c = ch.make_case(N, q, step)
    ref = coinc.coinc_host(c["t0"], c["v0"], c["t1"], c["v1"], c["shifts"], ch.WINDOW)
    total = int(ref["offsets"][-1])
    cut = max(1, total // 2)
    assert 0 < cut < total
    dev = {k: T.from_numpy(np.array(c[k])).cuda() for k in ("t0", "v0", "t1", "v1", "shifts")}
    n0, n1 = len(c["t0"]), len(c["t1"])
    n1_dev = T.tensor([n1 - 1], dtype=T.int32).cuda()

    def case(g):
        ev = [g.place(dev[k]) for k in ("t0", "v0")], [g.place(dev[k]) for k in ("t1", "v1")]
        full = ops.coinc_slides(*ev[0], n0, *ev[1], n1, g.place(dev["shifts"]), ch.WINDOW)
        short = ops.coinc_slides(*ev[0], n0, *ev[1], n1, g.place(dev["shifts"]), ch.WINDOW, cap_total=cut)
        roomy = ops.coinc_slides(*ev[0], n0, *ev[1], g.place(n1_dev), g.place(dev["shifts"]), ch.WINDOW, cap_total=total + 5)
        out = {"offsets": full["offsets"], "cut_offsets": short["offsets"], "roomy_offsets": roomy["offsets"]}
        n_roomy = min(int(roomy["offsets"][-1]), total + 5)
        for k in RAGGED:
            assert full[k].shape == (total,) and short[k].shape == (cut,) and roomy[k].shape == (total + 5,)
            out[k], out["cut_" + k], out["roomy_" + k] = full[k], short[k], roomy[k][:n_roomy]
        return out
    r = run_contract(case, modules=MODULES)
    # ... and what came out under the guard is what the tests of the values check
    got = {k: r[k].cpu().numpy() for k in RAGGED + ("offsets",)}
    ch.check_equal(got, ref)
    assert T.equal(r["cut_offsets"], r["offsets"])
    for k in RAGGED:
        assert np.array_equal(r["cut_" + k].cpu().numpy(), ref[k][:cut]), k
    less = coinc.coinc_host(c["t0"], c["v0"], c["t1"][:n1 - 1], c["v1"][:n1 - 1], c["shifts"], ch.WINDOW)
    assert np.array_equal(r["roomy_offsets"].cpu().numpy(), less["offsets"])
    for k in RAGGED:
        assert np.array_equal(r["roomy_" + k].cpu().numpy(), less[k]), k
