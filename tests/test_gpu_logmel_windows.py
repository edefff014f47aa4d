"""``ops.logmel_windows`` (csrc/logmel_windows.hip): the log-mel features of the overlapping windows of a series, each STFT
frame computed once per call, against ``ops.logmel`` of the materialised windows -- bit for bit, so no tolerance: the
per-window kernels are held to HF's output and to the fp64 oracle by tests/test_gpu_frontend_config.py, and one case here is a
configuration of tests/frontend_any.py.  Both routes, both output layouts, 1 - 3 rows at a non-contiguous stride, first
windows 0 and 3, 1 / 2 / 5 / all windows; batch independence; the refusals; the memory contract under tests/guard.py.

The series: seeded white noise; a transient 1e3 x the noise, three samples long, at L + 1.5 steps, which enters at window 2
and has left ceil(L / step) + 2 windows later -- the maximum and the clamp floor differ between neighbours --; and exact
zeros over the last L + step samples, whose two windows must come out as the constant (-10 + 4) / 4."""

import ctypes as C

import numpy as np
import pytest

from tests import frontend_any as fa
from tests.guard import run_contract

pytestmark = pytest.mark.gpu

PITCH_EXTRA = 37              # the rows of a series lie N + 37 apart: a non-contiguous row stride
R_MAX = 3

# name -> (n_fft, hop, L, step): the shared-route cases of the issue
SHARED = {
    "n16_h4": (16, 4, 128, 8),
    "n18_h6": (18, 6, 132, 12),          # n_fft / 2 is no multiple of the hop
    "hop_is_nfft": (16, 16, 256, 32),    # no edge frame at the end
    "workload": (128, 12, 2048, 204),    # 6 + 160 + 4 frames
    "step_is_hop": (16, 4, 128, 4),
}
PER_WINDOW = {
    "step_10_hop_4": (16, 4, 128, 10),   # step is no multiple of the hop
    "step_is_L": (16, 4, 128, 128),      # nothing is shared
    "all_edges": (64, 8, 40, 8),         # n_fft / 2 = 32: every frame of a 40-sample window sees the padding
}
_CASES = {}


@pytest.fixture(scope="module")
def T():
    import torch
    assert torch.cuda.is_available()
    return torch


def config_of(name):
    from gw_whisper_amd import ops
    if name == "golden6":
        c = fa.cfg(6)                       # (80, 2048 Hz, hop 8, 1 s, n_fft 64, fmax 1024): tests/frontend_any.py
        return ops.FrontendConfig(c.n_mels, c.rate, c.n_fft, c.hop, c.n_samples, c.fmin, c.fmax), 200
    n_fft, hop, L, step = {**SHARED, **PER_WINDOW}[name]
    return ops.FrontendConfig(80, 2048, n_fft, hop, L, 0.0, 1024.0), step


class Case:
    """One configuration: the series [3, N] on the device at a pitch of N + 37, the count of windows, and the reference
    ``ops.logmel`` of every materialised window [n_all, 3, n_mels, n_frames], computed once."""

    def __init__(self, T, name, seed):
        from gw_whisper_amd import ops
        self.cfg, self.step = config_of(name)
        L, step = self.cfg.n_samples, self.step
        self.n_all = -(-L // step) + 8
        extra = min(5, step - 1)               # samples behind the last window: not enough for another one
        self.N = N = L + (self.n_all - 1) * step + extra
        rng = np.random.default_rng(seed)
        x = rng.standard_normal((R_MAX, N)).astype(np.float32)
        p = L + step + step // 2
        x[:, p:p + 3] += np.float32(1e3) * np.array([[1.0, -1.0, 1.0], [-1.0, 1.0, 0.5], [0.5, 1.0, -1.0]], np.float32)
        x[:, N - (L + step + extra):] = 0.0
        self.host = x
        buf = T.zeros((R_MAX, N + PITCH_EXTRA), dtype=T.float32, device="cuda")
        buf[:, :N] = T.from_numpy(x).cuda()
        self.series = buf[:, :N]
        assert not self.series.is_contiguous()
        win = self.series.as_strided((self.n_all, R_MAX, L), (step, N + PITCH_EXTRA, 1))
        flat = ops.logmel(win.contiguous().reshape(self.n_all * R_MAX, L), config=self.cfg)
        self.ref = flat.reshape(self.n_all, R_MAX, self.cfg.n_mels, self.cfg.n_frames)
        self.enter = 2
        self.leave = (p + 2) // step + 1       # the first window behind the transient

    def want(self, R, w0, n, rows_major):
        r = self.ref[w0:w0 + n, :R]
        return r.transpose(0, 1).contiguous() if rows_major else r


def case(T, name):
    if name not in _CASES:
        _CASES[name] = Case(T, name, 300 + len(_CASES))
    return _CASES[name]


def check_all(T, name, route, want_route):
    from gw_whisper_amd import ops
    c = case(T, name)
    for R in (1, 2, 3):
        for w0 in (0, 3):
            for n in (1, 2, 5, None):
                for rows_major in (False, True):
                    got = ops.logmel_windows(c.series[:R], c.cfg, c.step, w0=w0, n_windows=n, rows_major=rows_major, route=route)
                    nn = c.n_all - w0 if n is None else n
                    plan = ops.logmel_windows_plan(c.cfg, c.step, nn)["route"]
                    ran = "per_window" if route == "per_window" else plan
                    assert ops.last_logmel_windows_route() == ran
                    assert nn == 1 or want_route is None or ran == want_route
                    want = c.want(R, w0, nn, rows_major)
                    assert got.shape == want.shape and got.is_contiguous()
                    assert T.equal(got, want), (f"{name}: R {R} w0 {w0} n {n} rows_major {rows_major} route {ran}: "
                                                f"{int((got != want).sum())} of {got.numel()} elements differ, max "
                                                f"{float((got - want).abs().max()):.3e}")
    return c


@pytest.mark.parametrize("name", list(SHARED) + ["golden6"])
def test_shared_route_equals_the_materialised_windows(T, gww, name):
    from gw_whisper_amd import ops
    c = check_all(T, name, None, "shared")
    assert ops.logmel_windows_plan(c.cfg, c.step, c.n_all)["route"] == "shared"
    # the series does what it is built for: the transient moves the maximum of the windows it is in, the zero windows are
    # the constant of -10
    top = c.ref[:, 0].amax(dim=(1, 2)).cpu().numpy()
    assert c.leave < c.n_all - 2
    quiet, loud = max(top[:c.enter].max(), top[c.leave:c.n_all - 2].max()), top[c.enter:c.leave].min()
    assert loud > quiet + 0.5, "the transient must lift the windows it is in by more than two decades"
    assert T.equal(c.ref[-2:], T.full_like(c.ref[-2:], -1.5))


@pytest.mark.parametrize("name", list(SHARED) + ["golden6"])
def test_forced_per_window_route_equals_the_materialised_windows(T, gww, name):
    check_all(T, name, "per_window", "per_window")


@pytest.mark.parametrize("name", list(PER_WINDOW))
def test_the_plan_s_per_window_route_equals_the_materialised_windows(T, gww, name):
    from gw_whisper_amd import GwwError, ops
    c = check_all(T, name, None, "per_window")
    with pytest.raises(GwwError, match="route='shared' is refused"):
        ops.logmel_windows(c.series, c.cfg, c.step, route="shared")


def test_refusals(T, gww):
    from gw_whisper_amd import GwwError, _lib, ops
    c = case(T, "n16_h4")
    with pytest.raises(GwwError, match="route='shared' is refused"):      # one window shares nothing
        ops.logmel_windows(c.series, c.cfg, c.step, n_windows=1, route="shared")
    with pytest.raises(GwwError, match="n_windows=99"):
        ops.logmel_windows(c.series, c.cfg, c.step, n_windows=99)
    with pytest.raises(GwwError, match="n_windows"):
        ops.logmel_windows(c.series, c.cfg, c.step, w0=c.n_all)
    with pytest.raises(GwwError, match="step=0"):
        ops.logmel_windows(c.series, c.cfg, 0)
    with pytest.raises(GwwError, match="route="):
        ops.logmel_windows(c.series, c.cfg, c.step, route="fast")
    # the C entry refuses on its own, before any launch: a series too short, a workspace too small, a forced shared route
    lib, fe = _lib.lib(), ops._fe(c.series.device, 80, c.cfg)
    out = T.empty((4, 1, 80, c.cfg.n_frames), device="cuda")
    ws = T.empty((1 << 16,), device="cuda")
    args = lambda n_series, ws_bytes, force: (fe, c.series.data_ptr(), 1, n_series, c.N, c.step, 0, 4, out.data_ptr(), 0,  # noqa: E731
                                              ws.data_ptr(), ws_bytes, force, None)
    assert lib.gww_logmel_windows_f32(*args(c.cfg.n_samples + 3 * c.step - 1, ws.numel() * 4, -1)) == -1
    assert b"n_series" in lib.gww_last_error()
    assert lib.gww_logmel_windows_f32(*args(c.N, 64, -1)) == -3
    assert b"workspace_bytes" in lib.gww_last_error()
    step10 = (fe, c.series.data_ptr(), 1, c.N, c.N, 10, 0, 4, out.data_ptr(), 0, ws.data_ptr(), ws.numel() * 4, 1, None)
    assert lib.gww_logmel_windows_f32(*step10) == -1 and b"force_route" in lib.gww_last_error()
    assert lib.gww_logmel_windows_f32(*args(c.N, ws.numel() * 4, -1)) == 0
    T.cuda.synchronize()
    assert T.equal(out, c.ref[:4, :1])


@pytest.mark.parametrize("name", ["n16_h4", "workload"])
def test_a_window_does_not_depend_on_its_batch(T, gww, name):
    """Windows 0 .. 7 in one call against 0 .. 3 and 4 .. 7 in two: the stream tiles, the edge tiles and the seam differ,
    the bits do not."""
    from gw_whisper_amd import ops
    c = case(T, name)
    whole = ops.logmel_windows(c.series, c.cfg, c.step, w0=0, n_windows=8)
    a = ops.logmel_windows(c.series, c.cfg, c.step, w0=0, n_windows=4)
    b = ops.logmel_windows(c.series, c.cfg, c.step, w0=4, n_windows=4)
    assert ops.last_logmel_windows_route() == "shared"
    assert T.equal(whole, T.cat((a, b))) and T.equal(whole, c.ref[:8])


@pytest.mark.parametrize("rows_major", [False, True])
@pytest.mark.parametrize("name,route", [("n16_h4", None), ("workload", None), ("n18_h6", "per_window"), ("step_10_hop_4", None)])
def test_the_memory_contract(T, gww, name, route, rows_major):
    """Series rows N + 37 apart with the fill between them, output and workspace from the guard: nothing is written outside
    them, no output element is left unwritten, and the bits do not depend on what the workspace -- or the memory around
    the series -- held before."""
    from gw_whisper_amd import ops
    c = case(T, name)
    series = T.from_numpy(c.host).cuda()

    def run(g):
        return {"mel": ops.logmel_windows(g.place(series, pitch=c.N + PITCH_EXTRA), c.cfg, c.step, w0=1, n_windows=7,
                                          rows_major=rows_major, route=route)}
    got = run_contract(run)["mel"]
    assert T.equal(got, c.want(R_MAX, 1, 7, rows_major))


def test_plan_struct_matches_the_header(gww):
    """ctypes' layout of gww_windows_plan is the C one: a plan read through it reproduces the issue's counts."""
    from gw_whisper_amd import _lib, ops
    cfg, step = config_of("workload")
    plan = _lib.WindowsPlan()
    assert _lib.lib().gww_logmel_windows_plan(C.byref(cfg.c_struct()), step, 256, C.byref(plan)) == 0
    assert (plan.route, plan.edge_lo, plan.edge_hi, plan.interior, plan.stream_frames) == (1, 6, 4, 160, 17 * 255 + 160)
    assert ops.logmel_windows_plan(cfg, step, 256)["workspace_bytes"] == 4 * 80 * (17 * 255 + 160 + 10 * 256)
