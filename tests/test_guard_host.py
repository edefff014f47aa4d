"""Self-tests of the guard-band allocator (tests/guard.py) on the CPU: small Python stand-in "ops" that allocate through
a proxied dummy module and misbehave in exactly one way each -- a store one element past the output, one element before
it, an output element left unwritten, a result that depends on a band value -- must each be reported, with the right
offset; a well-behaved one must pass.  This is what shows that tests/test_gpu_memory_contract.py can fail: the library
itself is never broken or under-sized to show it.  Then the one host entry point of the library, ``ops.logmel_host``,
under the guard.  CPU only: nothing here may touch a GPU."""

import re
import types

import numpy as np
import pytest
import torch

from tests.guard import FILLS, MIN_BAND, Guard, GuardError, NoGuard, run_contract

N = 37      # output elements of the stand-ins (fp32)


def _standin_module():
    """A dummy module with a module-level name ``torch``, like the package modules the guard patches."""
    m = types.ModuleType("standin_ops")
    m.torch = torch
    return m


M = _standin_module()


def _beyond(t, index):
    """Element ``index`` of the storage ``t`` lives in, counted from t's first element (negative / >= numel: outside t,
    inside the block the guard -- or, unguarded, the padded test buffer -- owns)."""
    return torch.as_strided(t, (1,), (1,), storage_offset=t.storage_offset() + index)


def op_good(x):
    out = M.torch.empty((N,), dtype=torch.float32)
    out.copy_(2 * x)
    return out


def op_writes_one_past(x):
    out = op_good(x)
    _beyond(out, N)[0] = 1.5
    return out


def op_writes_one_before(x):
    out = op_good(x)
    _beyond(out, -1)[0] = 1.5
    return out


def op_leaves_one_unwritten(x, k=11):
    out = M.torch.empty((N,), dtype=torch.float32)
    out[:k] = 2 * x[:k]
    out[k + 1:] = 2 * x[k + 1:]
    return out


def op_depends_on_band(x):
    """A reduction that runs one element too far: reads the first band element behind a zeros buffer."""
    acc = M.torch.zeros((N,), dtype=torch.float32)
    acc.copy_(x)
    out = M.torch.empty((1,), dtype=torch.float32)
    out[0] = torch.as_strided(acc, (N + 1,), (1,), storage_offset=acc.storage_offset()).sum()
    return out


@pytest.fixture
def x():
    return torch.arange(1, N + 1, dtype=torch.float32)


def _guard(fill):
    return Guard(fill, modules=[M], cpu=True)


@pytest.mark.parametrize("fill", FILLS)
def test_well_behaved_standin_passes(x, fill):
    with _guard(fill) as g:
        out = op_good(g.place(x))
        g.check()
        assert g.owns(out) and g.owns(out[3:]) and not g.owns(x) and g.n_alloc == 1
        assert g.unwritten(out) == 0
        assert out.data_ptr() % 512 == 0 and out.is_contiguous()
        assert torch.equal(out, 2 * x)
    assert M.torch is torch, "the proxy must be gone after the with block"


def test_run_contract_passes_the_well_behaved_standin(x):
    r = run_contract(lambda g: {"out": op_good(g.place(x))}, modules=[M], cpu=True)
    assert torch.equal(r["out"], 2 * x)


@pytest.mark.parametrize("fill", FILLS)
def test_store_one_element_past_the_end_is_reported(x, fill):
    with _guard(fill) as g:
        op_writes_one_past(x)
        with pytest.raises(GuardError) as e:
            g.check()
    msg = str(e.value)
    # fp32 element N: bytes 4 N .. 4 N + 3 from the interior's first byte; 1.5 = 0x3FC00000 (two zero bytes under fill 0)
    first, last = (4 * N, 4 * N + 3) if fill else (4 * N + 2, 4 * N + 3)
    assert "back band damaged" in msg and f"offsets {first} .. {last} relative" in msg
    assert f"extent {last - first + 1} bytes" in msg
    assert f"({N},) torch.float32" in msg and "test_guard_host.py" in msg and "op_good" in msg


@pytest.mark.parametrize("fill", FILLS)
def test_store_one_element_before_the_start_is_reported(x, fill):
    with _guard(fill) as g:
        op_writes_one_before(x)
        with pytest.raises(GuardError) as e:
            g.check()
    msg = str(e.value)
    first = -4 if fill else -2
    assert "front band damaged" in msg and f"offsets {first} .. -1 relative" in msg and f"extent {-first} bytes" in msg


@pytest.mark.parametrize("fill", [0xFF, 0x7F])
def test_unwritten_output_element_is_reported(x, fill):
    with _guard(fill) as g:
        out = op_leaves_one_unwritten(x)
        g.check()                                     # no band is touched: only the missing write
        assert g.unwritten(out) == 1
        assert g.unwritten_mask(out).nonzero().flatten().tolist() == [11]
    with pytest.raises(AssertionError, match=re.escape("'out': 1 element(s)") + ".*flat index 11"):
        run_contract(lambda g: {"out": op_leaves_one_unwritten(g.place(x))}, modules=[M], cpu=True)


def test_result_that_depends_on_a_band_value_is_reported(x):
    vals = {}
    for fill in FILLS:
        with _guard(fill) as g:
            vals[fill] = float(op_depends_on_band(x)[0])
            g.check()                                 # a stray READ damages nothing ...
    assert vals[0x00] == float(x.sum())               # ... and the benign fill hides it
    assert np.isnan(vals[0xFF]) and vals[0x7F] > 1e38


def op_sums_padded_scratch(x):
    """A reduction over the padded rows of an ``empty`` scratch: right only while the padding happens to hold zeros."""
    scratch = M.torch.empty((N + 3,), dtype=torch.float32)
    scratch[:N] = x
    out = M.torch.empty((1,), dtype=torch.float32)
    out[0] = scratch.sum()
    return out


def test_result_that_depends_on_uninitialised_scratch_is_reported(x, monkeypatch):
    # unguarded, the ordinary allocator's leftovers stand in for the padding: make them the benign zeros
    monkeypatch.setattr(M, "torch", types.SimpleNamespace(empty=lambda *a, **k: torch.zeros(*a, **k)))
    r0 = op_sums_padded_scratch(x)
    monkeypatch.setattr(M, "torch", torch)
    assert float(r0[0]) == float(x.sum())
    for fill, bad in ((0xFF, np.isnan), (0x7F, lambda v: v > 1e38)):
        with _guard(fill) as g:
            out = op_sums_padded_scratch(x)
            g.check()
            assert bad(float(out[0])) and not torch.equal(out, r0)
    with _guard(0x00) as g:
        assert torch.equal(op_sums_padded_scratch(x), r0)      # the benign fill hides it


def test_case_without_guarded_allocation_fails(x):
    with _guard(0xFF) as g:
        g.place(x)
        with pytest.raises(GuardError, match="tests nothing"):
            g.check()


def test_zeros_interior_is_zero_and_bands_are_sized_from_the_pitch():
    with Guard(0x7F, arena_row_bytes=4 * 6144, modules=[M], cpu=True) as g:
        z = M.torch.zeros((3, 5), dtype=torch.float32)
        zl = M.torch.zeros_like(z)
        e = M.torch.empty_like(z, dtype=torch.bfloat16)
        arena = M.torch.empty((1000,), dtype=torch.uint8)
        wide = M.torch.empty((2, 4096), dtype=torch.float32)
        assert not z.any() and not zl.any() and g.unwritten(e) == e.numel() and e.dtype == torch.bfloat16
        band = {r.shape: r.band for r in g.records}
        assert band[(3, 5)] == MIN_BAND                       # 512 rows of 20 bytes: the 1 MiB floor
        assert band[(1000,)] == 512 * 4 * 6144                # a byte arena: 512 of the widest rows carved from it
        assert band[(2, 4096)] == 512 * 4 * 4096              # 512 rows of the buffer's own pitch
        assert float(e.float().abs().max()) == pytest.approx(3.39e38, rel=1e-2)
        g.check()


def test_place_with_pitch_fills_the_gap(x):
    t = x[:36].reshape(4, 9)
    with _guard(0xFF) as g:
        M.torch.empty((1,))
        v = g.place(t, pitch=16)
        assert v.shape == (4, 9) and v.stride() == (16, 1) and torch.equal(v, t) and g.owns(v)
        full = torch.as_strided(v, (4, 16), (16, 1), storage_offset=v.storage_offset())
        assert torch.isnan(full[:, 9:]).all()
        g.repoison(v, 0x00)
        assert not full.any()
        g.check()
    v0 = NoGuard().place(t, pitch=16)
    assert v0.stride() == (16, 1) and torch.equal(v0, t)


# ---------------------------------------------------------------- the library's host entry point under the guard
@pytest.mark.parametrize("n_mels", [80, 128])
@pytest.mark.parametrize("n", [1, 159, 12345])
def test_logmel_host_under_the_guard(n_mels, n):
    """``gww_logmel_host_nmel_f32`` with wave_stride > n_samples and the gap holding 0xFF (NaN): the first n_samples of
    each row are the samples (include/gww.h), so the bands stay intact, every output element is written, and the result
    is bit-identical to the unguarded call on the bare samples."""
    from gw_whisper_amd import ops, synth
    w = synth.strain_segments(2, seed=300 + n, n_samples=n)
    ref = ops.logmel_host(w, n_mels=n_mels)
    stride = n + 1000
    padded = torch.from_numpy(w).new_empty((2, stride))
    padded.view(torch.uint8).fill_(0xFF)
    padded[:, :n] = torch.from_numpy(w)
    assert torch.isnan(padded[:, n:]).all()
    for fill in FILLS:
        with Guard(fill, cpu=True) as g:
            out = ops.logmel_host(g.place(padded), n_samples=n, n_mels=n_mels)
            g.check()
            assert g.owns(out) and g.n_alloc == 1
            if fill:
                assert g.unwritten(out) == 0
            assert out.shape == (2, n_mels, 3000) and torch.isfinite(out).all()
            assert torch.equal(out, ref), f"fill 0x{fill:02X}"
