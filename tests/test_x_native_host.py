"""The accumulator-order layout of the residual stream (``x_native_offset``, csrc/common.h) on the host: the C entry point
``gww_x_native_offset`` against a numpy restatement of the formula, and the properties the fused block relies on -- every
element of an [M, 384] stream has a slot of its own inside the whole panels the buffer spans, a lane's 16 bytes are
contiguous, a wave instruction's 64 lanes cover one KiB, a 32-row slice keeps the byte range it has in row order (so x_next
can come back in place), and a row past M lands on the slot of row M - 1."""

import numpy as np
import pytest

import gw_whisper_amd

D = 384
SIZES = [1, 31, 32, 127, 128, 129, 1500, 4500]


def _offsets_numpy(M, rows=None):
    """Byte offset of every (row, column), rows clamped to M - 1: ((4 P + w) 48 + 4 t + cc) 1024 + (r + 32 hh) 16 + 4 k."""
    g = np.arange(M, dtype=np.int64) if rows is None else np.asarray(rows, dtype=np.int64)
    g = np.minimum(g, M - 1)[:, None]
    c = np.arange(D, dtype=np.int64)[None, :]
    P, w, r = g >> 7, (g >> 5) & 3, g & 31
    t, cc, hh, k = c >> 5, (c >> 3) & 3, (c >> 2) & 1, c & 3
    return ((4 * P + w) * 48 + 4 * t + cc) * 1024 + (r + 32 * hh) * 16 + 4 * k


def _offsets_lib(M, rows):
    lib = gw_whisper_amd.lib()
    return np.array([[lib.gww_x_native_offset(int(g), c, M) for c in range(D)] for g in rows], dtype=np.int64)


@pytest.fixture(scope="module", params=SIZES)
def layout(request):
    M = request.param
    return M, _offsets_numpy(M)


def test_bijection_into_the_padded_buffer(layout):
    M, off = layout
    nbytes = gw_whisper_amd.lib().gww_x_native_bytes(M)
    assert nbytes == (M + 127) // 128 * 128 * D * 4
    assert off.min() >= 0 and off.max() + 4 <= nbytes
    assert (off % 4 == 0).all()
    assert np.unique(off).size == M * D            # one slot per element


def test_library_matches_numpy(layout):
    M, off = layout
    # every row of a small stream; of a large one the first and last panel, the rows around every slice boundary of a few
    # panels in between, and rows past M
    rows = set(range(min(M, 130))) | set(range(max(0, M - 130), M))
    rows |= {g for base in (128 * 5, 128 * 11, 128 * 34) for g in range(base - 2, base + 34) if g < M}
    rows = sorted(rows)
    assert np.array_equal(_offsets_lib(M, rows), off[rows])
    past = [M, M + 1, M + 31, M + 127]
    got = _offsets_lib(M, past)
    assert np.array_equal(got, np.broadcast_to(off[M - 1], got.shape))          # clamped rows: the slot of row M - 1
    assert np.array_equal(_offsets_numpy(M, past), got)


def test_pieces_lines_and_slices(layout):
    M, off = layout
    # a lane's four values of a piece are 16 contiguous bytes
    q = off.reshape(M, D // 4, 4)
    assert (q[:, :, 0] % 16 == 0).all() and (np.diff(q, axis=2) == 4).all()
    # a 32-row slice keeps the 48 KiB it has in row order: block l + 1 reads what block l wrote, in place
    g = np.arange(M)[:, None]
    assert (off // (32 * D * 4) == g // 32).all()
    # piece 4 t + cc of a full slice: the 64 lanes (r, hh) in order cover exactly one KiB
    for s in range(M // 32):
        sl = off[32 * s:32 * s + 32] - s * 32 * D * 4
        for t in (0, 5, 11):
            for cc in range(4):
                lanes = np.stack([sl[:, 32 * t + 8 * cc + 4 * hh] for hh in (0, 1)])          # [hh, r]
                assert np.array_equal(lanes.reshape(-1), (4 * t + cc) * 1024 + 16 * np.arange(64))
        if s >= 2:
            break


def test_bad_arguments():
    lib = gw_whisper_amd.lib()
    bad = (1 << 64) - 1
    assert lib.gww_x_native_offset(-1, 0, 10) == bad
    assert lib.gww_x_native_offset(0, 384, 10) == bad
    assert lib.gww_x_native_offset(0, 0, 0) == bad
    assert lib.gww_x_native_bytes(0) == 0
