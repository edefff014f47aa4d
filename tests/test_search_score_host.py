"""CPU pins of the search score: the numpy restatement of csrc/score.hip's algorithm against the golden file the
reference's own ``get_stats`` wrote (tools/make_golden_search_score.py), the host-side bookkeeping of
``gw_whisper_amd/search_score.py`` and the file handling of harness/run_search_evaluate.py."""

import importlib.util
import os

import numpy as np
import pytest

from . import search_score_helpers as sh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def gold():
    return np.load(sh.GOLD, allow_pickle=False)


@pytest.fixture(scope="module")
def harness():
    spec = importlib.util.spec_from_file_location("run_search_evaluate", os.path.join(ROOT, "harness", "run_search_evaluate.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def golden_case(gold, ci, mode):
    pre = f"c{ci}_{mode}_"
    return {k[len(pre):]: gold[k] for k in gold.files if k.startswith(pre)}


@pytest.mark.parametrize("mode", sh.MODES)
@pytest.mark.parametrize("ci", range(sh.HAND + 1))
def test_restatement_equals_the_reference(gold, ci, mode):
    fg, bg, inj, duration = sh.case(ci)
    r = sh.restate(fg, bg, inj, duration, mode == "chirp")
    g = golden_case(gold, ci, mode)
    assert len(g) == (16 - len(sh.BIG_KEYS) if ci == len(sh.CASES) - 1 else 16)
    sh.compare(r, {**r, **g}, mode == "chirp", "restatement vs reference", [k for k in sh.EXACT_KEYS if k in g])


def test_hand_case_is_what_the_reference_gives(gold):
    g = golden_case(gold, sh.HAND, "plain")
    assert g["found-indices"].tolist() == [0, 0, 1, 1, 2]
    assert g["true-positive-event-indices"].tolist() == [1, 3]
    assert g["true-positive-diffs"].tolist() == [0.25, 0.125]          # |dt| == var counts
    assert g["false-positive-diffs"].tolist() == [10.0, 15.0, 10.0]     # the midpoint went right: 130 - 115


def test_find_injection_times_padding():
    from gw_whisper_amd import search_score as ss
    tc = np.array([1029.0, 1030.0, 1031.0, 1070.0, 1071.0, 2040.0, 5000.0])
    # [1000, 1100) -> [1030, 1070]; a 50 s segment vanishes under the padding but still counts for the duration
    segs = [(1000.0, 204800, 1.0 / 2048), (2000.0, 50 * 2048, 1.0 / 2048)]
    dur, mask = ss.find_injection_times(segs, tc, padding_start=30, padding_end=30)
    assert dur == 150.0
    assert mask.tolist() == [False, True, True, True, False, False, False]
    dur, mask = ss.find_injection_times(segs, tc)
    assert dur == 150.0 and mask.tolist() == [True, True, True, True, True, True, False]
    dur, mask = ss.find_injection_times([], tc, 30, 30)
    assert dur == 0 and mask.shape == (7,) and not mask.any()


def test_mchirp_is_the_reference_expression():
    from gw_whisper_amd import search_score as ss
    m1, m2 = np.array([10.0, 30.0, 50.0]), np.array([12.0, 25.0, 40.0])
    assert np.array_equal(ss.mchirp(m1, m2), (m1 * m2) ** (3. / 5.) / (m1 + m2) ** (1. / 5.))


def _write_inputs(tmp_path, seconds):
    """One foreground file with one ``seconds`` long segment, an injection file, two event files as run_inference.py writes."""
    fg, bg, inj, _ = sh.case(1)
    start = float(np.floor(inj["tc"][0])) - 40.0
    n = int(seconds * 16)
    np.savez(tmp_path / "fgdata.npz", **{"H1/seg": np.zeros(n, np.float32), "L1/seg": np.zeros(n, np.float32),
                                         "seg/start_time": np.float64(start), "seg/delta_t": np.float64(1.0 / 16)})
    np.savez(tmp_path / "inj.npz", **inj)
    for name, ev in (("fgev", fg), ("bgev", bg)):
        np.savez(tmp_path / f"{name}.hdf.npz", time=ev[0], stat=ev[1], var=ev[2], all_vals=np.zeros(3, np.float32))
    return ["--injection-file", str(tmp_path / "inj.npz"), "--foreground-events", str(tmp_path / "fgev.hdf.npz"),
            "--foreground-files", str(tmp_path / "fgdata.npz"), "--background-events", str(tmp_path / "bgev.hdf.npz")]


def test_harness_argument_errors_and_force(harness, tmp_path):
    base = _write_inputs(tmp_path, seconds=45)          # shorter than the two paddings: no injection can lie inside
    with pytest.raises(SystemExit):
        harness.main(base)                                # --output-file is required
    with pytest.raises(ValueError, match="extension"):
        harness.main(base + ["--output-file", str(tmp_path / "out.txt")])
    out = tmp_path / "out.hdf"
    written = harness.output_path(str(out))
    open(written, "w").close()
    with pytest.raises(IOError, match="already exists"):
        harness.main(base + ["--output-file", str(out)])
    # --force passes the overwrite check; the next check is the reference's
    with pytest.raises(RuntimeError, match="contains no injections"):
        harness.main(base + ["--output-file", str(out), "--force"])
    assert os.path.getsize(written) == 0


def test_event_file_round_trip(harness, tmp_path):
    """An events file of run_inference.py's shape (time, stat, var, all_vals) reads back as the [3, n] it was written from,
    through the name without the ``.npz`` suffix too when h5py is absent; the result file holds every key."""
    _write_inputs(tmp_path, seconds=45)
    fg, _, _, _ = sh.case(1)
    assert np.array_equal(harness.read_events([str(tmp_path / "fgev.hdf.npz")]), fg)
    if not harness._have_h5py():
        assert np.array_equal(harness.read_events([str(tmp_path / "fgev.hdf")]), fg)
    two = harness.read_events([str(tmp_path / "fgev.hdf.npz"), str(tmp_path / "bgev.hdf.npz")])
    assert two.shape == (3, 257 + 255) and two.dtype == np.float64
    assert harness.read_segment_list(str(tmp_path / "fgdata.npz")) == [(float(np.floor(sh.case(1)[2]["tc"][0])) - 40.0, 45 * 16, 1.0 / 16)]
    r = sh.restate(*sh.case(1)[:3], sh.case(1)[3])
    stats = {k: r[k] for k in r if not k.startswith("_")}
    harness.write_result(str(tmp_path / "res.npz"), stats)
    back = harness.read_arrays(str(tmp_path / "res.npz"))
    assert sorted(back) == sorted(stats) and len(back) == 16
    assert all(np.array_equal(back[k], stats[k]) for k in stats)
