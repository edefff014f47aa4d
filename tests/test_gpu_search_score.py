"""The search score on the device (csrc/score.hip, gw_whisper_amd/search_score.py) against the golden file the
reference's own ``get_stats`` wrote and, for shapes beyond it, against the numpy restatement the host tests hold to that
file.  Bit for bit on every key; in chirp-weighted mode the volume keys within the derived bounds of
``search_score_helpers.compare``."""

import numpy as np
import pytest

from . import search_score_helpers as sh

pytestmark = pytest.mark.gpu

CHUNK = 4096
SORT_SIZES = (1, 255, 256, 257, CHUNK - 1, CHUNK, CHUNK + 1, 3 * CHUNK + 17)


@pytest.fixture(scope="module")
def T():
    import torch
    assert torch.cuda.is_available()
    return torch


@pytest.fixture(scope="module")
def ss(gww):
    from gw_whisper_amd import search_score
    return search_score


@pytest.fixture(scope="module")
def gold():
    return np.load(sh.GOLD, allow_pickle=False)


def _gold(gold, ci, mode):
    pre = f"c{ci}_{mode}_"
    return {k[len(pre):]: gold[k] for k in gold.files if k.startswith(pre)}


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("mode", sh.MODES)
@pytest.mark.parametrize("ci", range(sh.HAND + 1))
def test_device_equals_the_reference(ss, gold, ci, mode):
    fg, bg, inj, duration = sh.case(ci)
    chirp = mode == "chirp"
    got = ss.get_stats(fg, bg, inj, duration=duration, chirp_distance=chirp)
    assert tuple(got) == ss.KEYS
    g = _gold(gold, ci, mode)
    aux = sh.restate(fg, bg, inj, duration, chirp)      # _F, _S1, _S2 for the bounds; the keys the golden leaves out
    sh.compare(got, {**aux, **g}, chirp, "device vs reference")


def sort_keys(n, seed):
    """negatives, +-0, denormals, +-inf, GPS-sized values that differ in the last bit, heavy ties"""
    rng = np.random.default_rng(seed)
    gps = np.float64(sh.GPS0) + rng.integers(0, 4, n) * np.spacing(np.float64(sh.GPS0))
    pool = np.array([0.0, -0.0, 5e-324, -5e-324, 2.2e-308, -1e-310, np.inf, -np.inf, 1.5, -1.5, 6.1, 6.1, -6.1])
    k = np.where(rng.random(n) < 0.4, gps, pool[rng.integers(0, len(pool), n)])
    some = rng.random(n) < 0.2
    k[some] = np.round(rng.normal(0, 3, int(some.sum())), 1)
    return k


@pytest.mark.parametrize("n", SORT_SIZES)
def test_sort_is_numpys_stable_argsort(T, gww, n):
    from gw_whisper_amd import ops
    keys = sort_keys(n, 7000 + n)
    order, out, n_nan = ops.score_sort(T.from_numpy(keys).cuda())
    ref = np.argsort(keys, kind="stable")              # -0.0 == +0.0: a tie, kept in index order
    assert int(n_nan.item()) == 0
    assert np.array_equal(order.cpu().numpy(), ref)
    assert _same_bits(out.cpu().numpy(), keys[ref])     # the keys' own bits, signed zeros included


def test_sort_counts_nans_and_honours_a_device_count(T, gww):
    from gw_whisper_amd import ops
    n, m = CHUNK + 300, CHUNK + 3
    keys = sort_keys(n, 7777)
    keys[[5, 300, CHUNK + 1]] = np.nan
    order, out, n_nan = ops.score_sort(T.from_numpy(keys).cuda())
    assert int(n_nan.item()) == 3
    assert np.array_equal(order.cpu().numpy(), np.argsort(keys, kind="stable"))          # NaNs last, in index order
    cnt = T.tensor([m], dtype=T.int32, device="cuda")
    order, out, n_nan = ops.score_sort(T.from_numpy(keys).cuda(), n_dev=cnt)
    ref = np.argsort(keys[:m], kind="stable")
    assert int(n_nan.item()) == 3
    assert np.array_equal(order[:m].cpu().numpy(), ref) and _same_bits(out[:m].cpu().numpy(), keys[:m][ref])


def test_closest_index_tie_rule(ss):
    tc = np.array([100.0, 130.0, 160.0])
    below = np.nextafter(115.0, 0.0)
    t = np.array([115.0, below, 145.0, np.nextafter(145.0, 0.0), 100.0, 90.0, 170.0, 130.0, 160.0])
    assert ss.find_closest_index(tc, t).tolist() == [1, 0, 2, 1, 0, 0, 2, 1, 2]
    assert ss.find_closest_index(np.array([7.0]), np.array([[1.0, 9.0]])).tolist() == [[0, 0]]
    rng = np.random.default_rng(5)
    tc = np.sort(rng.uniform(0, 1000, 513))
    t = np.concatenate([rng.uniform(-10, 1010, 5000), tc, (tc[1:] + tc[:-1]) / 2])
    assert np.array_equal(ss.find_closest_index(tc, t), sh.closest(tc, t)[0])


def test_equality_counts_as_a_true_positive(ss):
    fg, bg, inj, duration = sh.hand_case()
    col = int(np.flatnonzero(fg[0] == 100.25)[0])
    assert fg[2, col] == 0.25
    assert ss.get_stats(fg, bg, inj, duration)["true-positive-event-indices"].tolist() == [1, 3]
    fg[2, col] = np.nextafter(0.25, 0.0)                 # one ulp less: a false positive
    got = ss.get_stats(fg, bg, inj, duration)
    assert got["true-positive-event-indices"].tolist() == [3]
    assert got["false-positive-event-indices"].tolist() == [0, 1, 2, 4]
    sh.compare(got, sh.restate(fg, bg, inj, duration), False, "device vs restatement")


BEYOND = {"one run": (3 * CHUNK + 17, 700, 1, 4101), "two runs": (3 * CHUNK + 17, 700, 2, 4102),
          "most missed": (3 * CHUNK + 17, CHUNK + 1, 8 * CHUNK + 3, 4103)}


@pytest.mark.parametrize("mode", sh.MODES)
@pytest.mark.parametrize("name", sorted(BEYOND))
def test_device_equals_the_restatement_beyond_the_goldens(ss, name, mode):
    E, B, N, seed = BEYOND[name]
    fg, bg, inj, duration = sh.make_case(E, B, N, seed)
    duration = duration if N == 1 else None             # None: the span of the injection times
    chirp = mode == "chirp"
    ref = sh.restate(fg, bg, inj, duration, chirp)
    if name == "most missed":
        assert len(ref["missed-indices"]) > N // 2
    got = ss.get_stats(fg, bg, inj, duration=duration, chirp_distance=chirp)
    sh.compare(got, ref, chirp, "device vs restatement")


def test_empty_background_and_no_false_positive(ss):
    fg, bg, inj, duration = sh.hand_case()
    got = ss.get_stats(fg, bg[:, :0], inj, duration)
    for k in ("far",) + sh.VOLUME_KEYS:
        assert got[k].shape == (0,) and got[k].dtype == np.float64
    assert got["found-indices"].tolist() == [0, 0, 1, 1, 2]
    only_tp = fg[:, np.isin(fg[0], (100.25, 130.125))]
    got = ss.get_stats(only_tp, bg, inj, duration)
    assert got["fg-far"].shape == (0,) and got["false-positives"].shape == (3, 0)
    assert got["missed-indices"].tolist() == [2]
    sh.compare(got, sh.restate(only_tp, bg, inj, duration), False, "device vs restatement")


def test_refusals(T, ss, gww):
    fg, bg, inj, duration = sh.hand_case()
    E = gww.GwwError

    def inj_with(**kw):
        return {**inj, **kw}
    with pytest.raises(E, match="not ascending"):
        ss.get_stats(fg, bg, inj_with(tc=np.array([100.0, 160.0, 130.0])), duration)
    with pytest.raises(E, match="NaN"):
        ss.get_stats(fg, bg, inj_with(tc=np.array([100.0, np.nan, 160.0])), duration)
    for row in (0, 1):
        bad = fg.copy()
        bad[row, 2] = np.nan
        with pytest.raises(E, match="NaN"):
            ss.get_stats(bad, bg, inj, duration)
    bad = bg.copy()
    bad[1, 0] = np.nan
    with pytest.raises(E, match="NaN"):
        ss.get_stats(fg, bad, inj, duration)
    with pytest.raises(E, match="no foreground events"):
        ss.get_stats(fg[:, :0], bg, inj, duration)
    with pytest.raises(E, match="no true positive"):
        ss.get_stats(fg[:, np.isin(fg[0], (90.0, 115.0, 170.0))], bg, inj, duration)
    with pytest.raises(E, match="CPU tensor"):
        ss.get_stats(T.from_numpy(fg), bg, inj, duration)
    with pytest.raises(E, match="CPU tensor"):
        ss.get_stats(fg, T.from_numpy(bg), inj, duration)
    huge = np.broadcast_to(np.zeros((3, 1)), (3, (1 << 27) + 1))     # a view: no memory behind it
    with pytest.raises(E, match="more than 2\\^27"):
        ss.get_stats(huge, bg, inj, duration)
    with pytest.raises(E, match="more than 2\\^27"):
        ss.get_stats(fg, huge, inj, duration)


def test_harness_end_to_end(ss, tmp_path):
    """harness/run_search_evaluate.py in this process: event files of run_inference.py's shape, one foreground segment
    around all injections, an injection file with the ``chirp_distance`` key -> the sixteen datasets of the weighted mode."""
    import importlib.util
    import os
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "harness", "run_search_evaluate.py")
    spec = importlib.util.spec_from_file_location("run_search_evaluate", path)
    harness = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(harness)
    fg, bg, inj, _ = sh.case(1)
    start = float(np.floor(inj["tc"][0])) - 40.0
    n = (int(np.ceil(inj["tc"][-1] - start)) + 40) * 16
    np.savez(tmp_path / "fgdata.npz", **{"H1/seg": np.zeros(n, np.float32), "L1/seg": np.zeros(n, np.float32),
                                         "seg/start_time": np.float64(start), "seg/delta_t": np.float64(1.0 / 16)})
    np.savez(tmp_path / "inj.npz", chirp_distance=np.ones(len(inj["tc"])), **inj)
    half = fg.shape[1] // 2
    np.savez(tmp_path / "fg0.npz", time=fg[0, :half], stat=fg[1, :half], var=fg[2, :half], all_vals=np.zeros(3, np.float32))
    np.savez(tmp_path / "fg1.npz", time=fg[0, half:], stat=fg[1, half:], var=fg[2, half:], all_vals=np.zeros(3, np.float32))
    np.savez(tmp_path / "bg.npz", time=bg[0], stat=bg[1], var=bg[2], all_vals=np.zeros(3, np.float32))
    out = str(tmp_path / "out.hdf")
    assert harness.main(["--injection-file", str(tmp_path / "inj.npz"), "--foreground-events", str(tmp_path / "fg0.npz"),
                         str(tmp_path / "fg1.npz"), "--foreground-files", str(tmp_path / "fgdata.npz"), "--background-events",
                         str(tmp_path / "bg.npz"), "--output-file", out]) == 0
    got = harness.read_arrays(out)
    assert sorted(got) == sorted(ss.KEYS)
    sh.compare(got, sh.restate(fg, bg, inj, n / 16.0, True), True, "harness vs restatement")
    with pytest.raises(IOError, match="already exists"):
        harness.main(["--injection-file", "x", "--foreground-events", "x", "--foreground-files", "x", "--background-events", "x",
                      "--output-file", out])


@pytest.mark.parametrize("mode", sh.MODES)
def test_identical_calls_and_tensor_inputs_give_identical_bits(T, ss, mode):
    fg, bg, inj, duration = sh.case(2)
    chirp = mode == "chirp"
    a = ss.get_stats(fg, bg, inj, duration, chirp)
    b = ss.get_stats(fg, bg, inj, duration, chirp)
    c = ss.get_stats(T.from_numpy(fg).cuda(), T.from_numpy(bg).cuda(), inj, duration, chirp)
    for k in ss.KEYS:
        assert _same_bits(a[k], b[k]), f"{k}: two identical calls differ"
        assert _same_bits(a[k], c[k]), f"{k}: GPU-tensor inputs differ from numpy inputs"
