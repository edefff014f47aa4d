"""The general log-mel kernels (csrc/logmel_any.hip) per element, on the seven configurations of tests/frontend_any.py:
every element the fp64 restatement leaves unclamped is held to LIMIT x GAMMA x e_model of its own, the clamped ones to
the floor the kernel's own segment maximum implies, the dead frames to one bitwise constant; the published configuration
through the general kernels (a test-only handle flag) under the same model, next to the kernels written for it; batch
independence; and the new entry points under the guard-band allocator of tests/guard.py."""

import numpy as np
import pytest

from tests import frontend_any as fa
from tests.guard import run_contract

pytestmark = pytest.mark.gpu

IDS = list(range(len(fa.CONFIGS)))
_OUT = {}


@pytest.fixture(scope="module")
def T():
    import torch
    assert torch.cuda.is_available()
    return torch


def config(i, n_mels=None):
    from gw_whisper_amd import ops
    c = fa.cfg(i)
    return ops.FrontendConfig(n_mels or c.n_mels, c.rate, c.n_fft, c.hop, c.n_samples, c.fmin, c.fmax)


def device_out(T, i):
    """The general kernels' output for configuration i, computed once."""
    from gw_whisper_amd import ops
    if i not in _OUT:
        c = fa.cfg(i)
        out = ops.logmel(T.from_numpy(fa.waves(i)).cuda(), config=config(i), general=(i == "default")).cpu().numpy()
        assert out.shape == (fa.N_SEG, c.n_mels, c.n_frames) and out.dtype == np.float32
        out.setflags(write=False)
        _OUT[i] = out
    return _OUT[i]


@pytest.mark.parametrize("i", IDS + ["default"])
def test_every_unclamped_element_within_its_own_bound(T, gww, i):
    c, out = fa.case(i), device_out(T, i)
    assert c.unclamped.any()
    assert int(c.near.sum()) == 0, "an element within NEAR of the floor: a failure for these seeds, not a tolerance"
    worst = float(c.ratio(out)[c.unclamped].max())
    print(f"config {i!r}: worst |err| / e_model = {worst:.3f} = {worst / fa.GAMMA[i]:.3f} x GAMMA (limit {fa.LIMIT:g} x GAMMA)")
    assert worst <= fa.LIMIT * fa.GAMMA[i]


@pytest.mark.parametrize("i", IDS + ["default"])
def test_clamped_and_dead_elements(T, gww, i):
    """Clamped elements equal the floor the kernel's own maximum implies: with mx the fp32 raw maximum the kernel took --
    recovered from its largest output, (mx + 4) / 4, over the few fp32 values that map there -- every element the oracle
    puts NEAR under the floor is (max(mx, -10 if dead frames) - 8 + 4) / 4 in fp32, bit for bit; the dead frames are
    (max(-10, floor) + 4) / 4, one bitwise constant, and the tail of every row is that constant."""
    f32 = np.float32
    c, out = fa.case(i), device_out(T, i)
    cfg, live = c.cfg, c.live
    for s in range(fa.N_SEG):
        top = out[s, :, :live].max()
        mx0 = f32(top) * f32(4.0) - f32(4.0)
        near = [mx0]
        for _ in range(4):                                  # (mx + 4 loses up to two bits of mx: a few values share an image)
            near = [np.nextafter(near[0], f32(-np.inf))] + near + [np.nextafter(near[-1], f32(np.inf))]
        cand = [m for m in near if (f32(m) + f32(4.0)) * f32(0.25) == top]
        assert cand, "the largest output is no image of an fp32 maximum"
        assert abs(float(top) - float(c.out[s].max())) <= fa.LIMIT * fa.GAMMA[i] * c.e_max[s]
        floors = [f32(max(m, f32(-10.0)) if live < cfg.n_frames else m) - f32(8.0) for m in cand]
        floor_out = {f32((fl + f32(4.0)) * f32(0.25)) for fl in floors}
        dead_out = {f32((max(f32(-10.0), fl) + f32(4.0)) * f32(0.25)) for fl in floors}
        far = c.clamped[s]
        if far.any():
            v = out[s, :, :live][far]
            assert (v == v[0]).all() and v[0] in floor_out
        dead = out[s, :, live:]
        if dead.size:
            assert (dead.view(np.uint32) == dead.view(np.uint32)[0, 0]).all(), "dead frames must be one bitwise constant"
            assert dead[0, 0] in dead_out
            assert abs(float(dead[0, 0]) - c.pad[s]) <= fa.LIMIT * fa.GAMMA[i] * c.e_max[s]
    assert i not in (0, 6) or c.clamped.any()        # the configurations with empty filters do clamp


def test_published_configuration_by_both_kernels(T, gww):
    """Whisper's configuration through the general kernels and through the kernels written for it: both within the model
    of the same oracle, the same dead-frame constant; a handle from gww_frontend_create_cfg runs the latter, bit for bit."""
    from gw_whisper_amd import ops
    c, gen = fa.case("default"), device_out(T, "default")
    w = T.from_numpy(fa.waves("default")).cuda()
    fixed = ops.logmel(w).cpu().numpy()
    via_cfg = ops.logmel(w, config=ops.FrontendConfig()).cpu().numpy()
    assert np.array_equal(fixed.view(np.uint32), via_cfg.view(np.uint32))
    for out in (gen, fixed):
        assert float(c.ratio(out)[c.unclamped].max()) <= fa.LIMIT * fa.GAMMA["default"]
    lim = fa.LIMIT * fa.GAMMA["default"] * (c.e_model + c.e_model)
    assert (np.abs(gen[:, :, :c.live].astype(np.float64) - fixed[:, :, :c.live])[c.unclamped] <= lim[c.unclamped]).all()
    for s in range(fa.N_SEG):
        assert abs(float(gen[s, 0, -1]) - float(fixed[s, 0, -1])) <= 2 * fa.LIMIT * fa.GAMMA["default"] * c.e_max[s]
        assert (gen[s, :, c.live:] == gen[s, 0, -1]).all()


@pytest.mark.parametrize("i", [0, 4, 5])
def test_a_segment_does_not_depend_on_its_batch(T, gww, i):
    """Each segment alone, and in a batch of five behind a loud and a silent neighbour, is bit-identical to the pair's."""
    from gw_whisper_amd import ops
    w, out = fa.waves(i), device_out(T, i)
    for s in range(fa.N_SEG):
        alone = ops.logmel(T.from_numpy(w[s:s + 1].copy()).cuda(), config=config(i)).cpu().numpy()
        assert np.array_equal(alone[0].view(np.uint32), out[s].view(np.uint32))
    big = np.stack([w[0] * np.float32(1e3), np.zeros_like(w[0]), w[1], w[0], w[1] * np.float32(1e-4)])
    got = ops.logmel(T.from_numpy(big).cuda(), config=config(i)).cpu().numpy()
    assert np.array_equal(got[2].view(np.uint32), out[1].view(np.uint32))
    assert np.array_equal(got[3].view(np.uint32), out[0].view(np.uint32))
    assert np.isfinite(got).all()


@pytest.mark.parametrize("n", [0, 1, 777, 9999])
def test_ragged_and_overlong_inputs(T, gww, n):
    """Input lengths from empty to beyond the chunk (truncated) on the 1 s / n_fft 64 configuration against the host twin,
    which tests/test_frontend_config_host.py holds to HF."""
    from gw_whisper_amd import ops
    w = np.random.default_rng(50 + n).standard_normal((2, max(n, 1))).astype(np.float32)
    dev = ops.logmel(T.from_numpy(w).cuda(), n_samples=n, config=config(6)).cpu().numpy()
    host = ops.logmel_host(w, n_samples=n, config=config(6)).numpy()
    np.testing.assert_allclose(dev, host, atol=2e-5, rtol=0)         # test_gpu_kernels.py's bound between the twins
    assert dev.shape == (2, 80, 256)


def test_device_filterbank_is_the_host_s(T, gww):
    from gw_whisper_amd import ops
    for i in IDS:
        np.testing.assert_array_equal(ops.mel_filters(config(i), device="cuda"), ops.mel_filters(config(i)))
        np.testing.assert_array_equal(ops.mel_filters(config(i)).T, fa.cfg(i).filters())


@pytest.mark.parametrize("i", [1, 4, 5])
def test_general_kernels_keep_the_memory_contract(T, gww, i):
    """gww_logmel_f32 on a general handle with wave_stride > n_samples, the gap holding the fill: no stray store, no
    unwritten output element, and bits that do not depend on what lies outside the contract."""
    from gw_whisper_amd import ops
    c = fa.cfg(i)
    wd = T.from_numpy(fa.waves(i)).cuda()
    n = c.n_in

    def case(g):
        pw = g.place(wd, pitch=n + 1000)
        full = T.as_strided(pw, (fa.N_SEG, n + 1000), (n + 1000, 1), storage_offset=pw.storage_offset())
        return {"mel": ops.logmel(full, n_samples=n, config=config(i))}
    got = run_contract(case)["mel"].cpu().numpy()
    assert np.array_equal(got.view(np.uint32), device_out(T, i).view(np.uint32))


def test_extractor_on_the_device(T, gww):
    from gw_whisper_amd.feature_extraction import WhisperFeatureExtractor
    c = fa.cfg(1)
    fe = WhisperFeatureExtractor(**c.extractor_kwargs(), device="cuda")
    x = fe(list(fa.waves(1)), sampling_rate=c.rate, return_tensors="pt", return_device="cuda").input_features
    assert x.is_cuda and np.array_equal(x.cpu().numpy().view(np.uint32), device_out(T, 1).view(np.uint32))
