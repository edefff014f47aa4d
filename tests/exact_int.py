"""Exact-integer operands for the bf16 backward reductions, their integer references, and the one table of cases.

Numpy only, no test functions.  The bf16 backward sums over the M = B T token rows in ``gemm_wgrad`` (wgrad.hip),
``dora_grads`` / ``dora_grads_multi`` / ``adapter_grads`` (train_ops.hip, dora_grads.hip) and ``layernorm_param_grads``
(train_ops.hip).  On Gaussian floats the bf16 rounding noise keeps every tolerance of their tests so wide that a lost row,
a lost 16-byte chunk or a stale slab passes.  On the operands below nothing is rounded anywhere, so the result does not
depend on the summation order, the slice plan, the MFMA shape or the order of the float atomics, and a correct kernel returns
the integer reference BIT FOR BIT.

Operand rules (``check_ranges`` enforces them, tests/test_exact_int_host.py runs it on every case):
  * row operands x, dy are integers in [-3, 3] WITHOUT zero (every 8-column chunk of every row changes the result when it
    is lost), y is an integer in [-8, 8] without zero; the only zero rows are the junk rows of the conv im2col views, which
    carry zero gradient in the encoder too;
  * projection factors A [r, d_in] and B [d_out, r] have entries in {-1, 0, 1}, at most 8 of them non-zero per rank row of A
    and per rank column of B: u = x A^T and v = dy (g . B) are then integers times a power of two with at most 8
    significant bits, exact where the kernels store them as bf16 (Us / Vs, U / V, Wu / Wv);
  * scale factors are powers of two that vary per column (a column shift of g = yscale mag / nrm is visible):
    mag in {0.5, 1, 2, 4}, nrm in {1, 2}, yscale in {1, 0.125}, scaling in {4, 0.5}, alpha in {1, 0.25, -2};
  * bias_st is an integer in [-4, 4]; pre-loaded dw0 / db0 / dbeta0 are integers in [-1000, 1000];
  * in the units of its power-of-two scale every intermediate -- every sum of absolute values of the terms of a result, so
    every partial sum in any order -- and every result stays below 2^24: exact in fp32.

References: the integer sums (dy^T x, sum dy, v^T x, dy^T u, sum dy y) are formed as int64 (``imatmul``: a float64 BLAS product
of integers below 2^53 is exact and is converted back), the power-of-two factors are applied in float64, which is exact for
these values; the host test re-derives sampled elements with ``fractions.Fraction``.
    dW = dw0 + alpha dy^T x          db = db0 + alpha sum_m dy
    dA = s (v^T x)                   dB = s g (dy^T u)              dm = (sum_m dy y - b sum_m dy) / mag
    dbeta = dbeta0 + sum_m dy
"""

from __future__ import annotations

import zlib

import numpy as np

LIMIT = 1 << 24                       # integers below it are exact in fp32
ALPHAS = (1.0, 0.25, -2.0)
MAGS = (0.5, 1.0, 2.0, 4.0)
NRMS = (1.0, 2.0)
YSCALES = (1.0, 0.125)
SCALINGS = (4.0, 0.5)
MUTATIONS = ("row_dropped", "row_doubled", "x_chunk_zeroed", "dy_chunk_zeroed", "x_rows_swapped", "dy_rows_swapped",
             "g_from_neighbour", "dw0_not_added", "alpha_twice")


# ------------------------------------------------------------------------------------------------------ small tools
def bf16_round(a):
    """fp32 values rounded to bf16, round to nearest even (returned as fp32): what a bf16 store keeps."""
    u = np.ascontiguousarray(a, np.float32).view(np.uint32)
    return ((u + np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1))) & np.uint32(0xFFFF0000)).view(np.float32)


def imatmul(a, b):
    """a @ b of integer arrays as int64.  Formed in float64 (BLAS): exact while the sum of absolute values stays below 2^53,
    which the bound checked here guarantees."""
    a, b = np.asarray(a), np.asarray(b)
    assert float(np.abs(a).max(initial=0)) * float(np.abs(b).max(initial=0)) * a.shape[-1] < 2.0 ** 53
    return np.rint(a.astype(np.float64) @ b.astype(np.float64)).astype(np.int64)


def significant_bits(n):
    """Largest number of significant bits (leading one to trailing one) among the integers n."""
    n = np.abs(np.asarray(n, np.int64)).ravel()
    n = n[n != 0]
    if n.size == 0:
        return 0
    return int(np.max(n // (n & -n))).bit_length()


def as_f32(ref):
    """The float64 reference as the fp32 the kernel must return (exact by the operand rules; -0 folded into +0)."""
    r = np.asarray(ref, np.float64)
    f = (r + 0.0).astype(np.float32)
    assert np.array_equal(f.astype(np.float64), r), "the reference itself is not exact in fp32"
    return f + np.float32(0.0)


def mismatch(got, want):
    """None when ``got`` (fp32) holds the reference bit for bit (uint32 views), else the flat indices that differ."""
    got = np.ascontiguousarray(got, np.float32)
    want = as_f32(want)
    assert got.shape == want.shape, (got.shape, want.shape)
    if np.array_equal(got.view(np.uint32), want.view(np.uint32)):
        return None
    return np.flatnonzero(got.view(np.uint32).ravel() != want.view(np.uint32).ravel())


def report(name, got, want, blocks):
    """What a mismatch looks like: how many elements, the first few (index, got, want), and the tiles they fall in.
    ``blocks``: per axis, the tile edge of the launch plan along it (1: the axis is not tiled)."""
    bad = mismatch(got, want)
    if bad is None:
        return None
    got, want = np.asarray(got, np.float32), as_f32(want)
    idx = np.stack(np.unravel_index(bad, got.shape), 1)
    tiles = sorted({tuple(int(i) // b for i, b in zip(ix, blocks)) for ix in idx})
    first = [(tuple(int(i) for i in ix), float(got[tuple(ix)]), float(want[tuple(ix)])) for ix in idx[:6]]
    return (f"{name}: {bad.size} of {got.size} elements differ; first (index, got, want) {first}; tiles of edge {blocks} hit: "
            f"{tiles[:12]}{' ...' if len(tiles) > 12 else ''}")


def wgrad_plan(M, N, K):
    """wgrad.hip's launch plan restated (for the mismatch report): (tiles_n, tiles_k, slices, rows_per_slice)."""
    cdiv = lambda a, b: -(-a // b)
    tiles_n, tiles_k = cdiv(N, 128), cdiv(K, 128)
    s = max(1, min(cdiv(512, tiles_n * tiles_k), cdiv(max(M, 1), 256), 64))
    rows = cdiv(cdiv(max(M, 1), s), 64) * 64
    return tiles_n, tiles_k, cdiv(max(M, 1), rows), rows


# ------------------------------------------------------------------------------------------------------ generators
def _rng(case, salt=0):
    return np.random.default_rng(zlib.crc32(case.id.encode()) + 7919 * salt)


def ints(rng, shape, hi=3):
    """Integers in [-hi, hi] without zero (int8)."""
    v = rng.integers(0, 2 * hi, size=shape, dtype=np.int8) - np.int8(hi)
    v[v >= 0] += 1
    return v


def pick(rng, values, n):
    return np.asarray(values, np.float64)[rng.integers(0, len(values), size=n)]


def factor_A(rng, r, d_in):
    """A [r, d_in] in {-1, 0, 1}, 8 non-zeros per rank row."""
    A = np.zeros((r, d_in), np.int8)
    for j in range(r):
        cols = rng.choice(d_in, size=8, replace=False)
        A[j, cols] = rng.choice(np.array([-1, 1], np.int8), size=8)
    return A


def factor_B(rng, d_out, r, g):
    """B [d_out, r] in {-1, 0, 1}, at most 8 non-zeros per rank column, thinned until v = dy (g . B) keeps 8 significant
    bits for every dy in [-3, 3]: 3 sum_c g[c] |B[c, j]| <= 255 in units of the smallest g of the column's non-zeros."""
    B = np.zeros((d_out, r), np.int8)
    for j in range(r):
        rows = list(rng.choice(d_out, size=8, replace=False))
        while 3 * sum(g[c] for c in rows) / min(g[c] for c in rows) > 255:
            rows.remove(max(rows, key=lambda c: g[c]))
        B[rows, j] = rng.choice(np.array([-1, 1], np.int8), size=len(rows))
    return B


class Case:
    """One row of the table: ``kernel`` in {"wgrad", "dora", "dora_multi", "adapter", "ln"}, the pytest id, the parameters."""

    def __init__(self, kernel, **p):
        self.kernel, self.p = kernel, p
        self.id = kernel + "-" + "-".join(f"{k}{v}" for k, v in p.items()).replace(" ", "").replace("(", "").replace(")", "") \
            .replace(",", "x").replace("[", "").replace("]", "").replace("'", "")

    def __getattr__(self, k):
        try:
            return self.__dict__["p"][k]
        except KeyError:
            raise AttributeError(k) from None

    def get(self, k, default=None):
        return self.p.get(k, default)

    def __repr__(self):
        return self.id


def _strided(flat, off, ld, rows, width):
    """rows x width view of a flat buffer with row stride ld (elements), starting at element off; rows may overlap."""
    assert off + (rows - 1) * ld + width <= flat.size
    return np.lib.stride_tricks.as_strided(flat[off:], (rows, width), (ld * flat.itemsize, flat.itemsize), writeable=False)


def wgrad_operands(c):
    """Buffers and layout of a gemm_wgrad case.  Returns a dict:
    dy_flat / x_flat (int8, 1-D), dy_lay / x_lay = (offset, row stride, rows of the view, width), M (rows summed), alpha,
    dw0 / db0 (int64 or None), want_db."""
    rng = _rng(c)
    M, N, K = c.M, c.N, c.K
    view = c.get("view", "plain")
    o = dict(M=M, alpha=float(c.get("alpha", 1.0)), want_db=c.get("db", True))
    if view == "plain":
        o["dy_flat"], o["dy_lay"] = ints(rng, M * N), (0, N, M, N)
        o["x_flat"], o["x_lay"] = ints(rng, M * K), (0, K, M, K)
    elif view == "sections":         # dy: the middle section of [M, 3 N]; x: columns 8 .. 8 + K of [M, K + 24]
        o["dy_flat"], o["dy_lay"] = ints(rng, M * 3 * N), (N, 3 * N, M, N)
        o["x_flat"], o["x_lay"] = ints(rng, M * (K + 24)), (8, K + 24, M, K)
    elif view == "rows":             # 37 more rows in the tensors than ``rows=`` asks for
        o["dy_flat"], o["dy_lay"] = ints(rng, (M + 37) * N), (0, N, M + 37, N)
        o["x_flat"], o["x_lay"] = ints(rng, (M + 37) * K), (0, K, M + 37, K)
    elif view == "conv2":            # row b (T + 1) + t reads c1 rows 2 t .. 2 t + 2; row T of a segment is junk
        B, Tn, d = c.B, c.Tn, N
        assert M == B * (Tn + 1) and K == 3 * d
        dz = ints(rng, (B, Tn + 1, d))
        dz[:, Tn] = 0
        o["dy_flat"], o["dy_lay"] = dz.ravel(), (0, d, M, d)
        o["x_flat"], o["x_lay"] = ints(rng, (2 * M + 2) * d), (0, 2 * d, M, K)
    elif view == "conv1":            # row m reads melT[m .. m + 3) (80 channels each) + 16 padding columns
        B, Tin, C = c.B, c.Tin, 80
        assert M == B * (Tin + 2) and K == 256
        dz = ints(rng, (B, Tin + 2, N))
        dz[:, Tin:] = 0
        o["dy_flat"], o["dy_lay"] = dz.ravel(), (0, N, M, N)
        o["x_flat"], o["x_lay"] = ints(rng, M * C + 256), (0, C, M, K)
    else:
        raise ValueError(view)
    acc = c.get("acc", False)
    o["dw0"] = rng.integers(-1000, 1001, size=(N, K)) if acc else None
    o["db0"] = rng.integers(-1000, 1001, size=N) if acc and o["want_db"] else None
    return o


def wgrad_effective(o):
    """The [M, N] / [M, K] integer matrices the kernel sums over, and the scalars: what the reference takes."""
    dy = _strided(o["dy_flat"], *o["dy_lay"])[:o["M"]].astype(np.int64)
    x = _strided(o["x_flat"], *o["x_lay"])[:o["M"]].astype(np.int64)
    return dict(dy=dy, x=x, alpha=o["alpha"], dw0=o["dw0"], db0=o["db0"], want_db=o["want_db"])


def _projection(rng, d_in, d_out, r, lora, yscale, scaling):
    mag = np.ones(d_out) if lora else pick(rng, MAGS, d_out)
    nrm = np.ones(d_out) if lora else pick(rng, NRMS, d_out)
    g = yscale * mag / nrm
    return dict(A=factor_A(rng, r, d_in), B=factor_B(rng, d_out, r, g), mag=mag, nrm=nrm,
                bias=rng.integers(-4, 5, size=d_out).astype(np.int64), yscale=float(yscale), scaling=float(scaling))


def _live_last_row(rng, x, dy, pr, g):
    """The last row is the one the mutations act on (and the ragged one of the last tile): redraw it until neither its u nor
    its v vanishes, so that losing a piece of it always shows."""
    for _ in range(64):
        if (x[-1].astype(np.int64) @ pr["A"].T.astype(np.int64)).any() and \
                ((dy[-1] * g) @ pr["B"].astype(np.float64)).any():
            return
        x[-1], dy[-1] = ints(rng, x.shape[1]), ints(rng, dy.shape[1])
    raise AssertionError("no live last row")


def adapter_operands(c):
    """Buffers of a dora_grads (r = 8, square) or adapter_grads case: x_buf [M, Wx], dy_buf / y_buf [M, Wy] (int8), the
    column offsets x_off / col_off of the operands inside them, and the projection (A, B, mag, nrm, bias, yscale,
    scaling)."""
    rng = _rng(c)
    M, d_in, d_out, r = c.M, c.d_in, c.d_out, c.r
    lay = c.get("layout", "plain")
    if lay == "plain":
        Wx, x_off, Wy, col_off = d_in, 0, d_out, 0
    elif lay == "strided":           # both operands sections of wider buffers
        Wx, x_off, Wy, col_off = d_in + 24, 8, d_out + 40, 16
    else:                            # "q" / "k" / "v": sections 0, d, 2 d of a packed [M, 3 d] pair
        Wx, x_off, Wy, col_off = d_in, 0, 3 * d_out, "qkv".index(lay) * d_out
    o = dict(M=M, x_off=x_off, col_off=col_off, x_buf=ints(rng, (M, Wx)), dy_buf=ints(rng, (M, Wy)), y_buf=ints(rng, (M, Wy), 8))
    o.update(_projection(rng, d_in, d_out, r, c.get("lora", False), c.get("yscale", 1.0), c.get("scaling", 4.0)))
    g = o["yscale"] * o["mag"] / o["nrm"]
    _live_last_row(rng, o["x_buf"][:, x_off:x_off + d_in], o["dy_buf"][:, col_off:col_off + d_out], o, g)
    return o


def adapter_effective(o, p=None):
    """x [M, d_in], dy, y [M, d_out] (int64) and the projection: what the reference takes.  ``p``: the projection of a
    dora_grads_multi case."""
    pr = o if p is None else o["proj"][p]
    d_out, d_in = pr["B"].shape[0], pr["A"].shape[1]
    co = o["col_off"] if p is None else o["col_off"][p]
    sl = slice(co, co + d_out)
    return dict(x=o["x_buf"][:, o["x_off"]:o["x_off"] + d_in].astype(np.int64), dy=o["dy_buf"][:, sl].astype(np.int64),
                y=o["y_buf"][:, sl].astype(np.int64), **{k: pr[k] for k in ("A", "B", "mag", "nrm", "bias", "yscale", "scaling")})


def multi_operands(c):
    """Buffers of a dora_grads_multi case: np projections in the sections ``order`` of a packed [M, 3 d] pair, each with its
    own A, B, mag, nrm, bias, yscale, scaling."""
    rng = _rng(c)
    M, d = c.M, c.d
    o = dict(M=M, x_off=0, col_off=[s * d for s in c.order], x_buf=ints(rng, (M, d)), dy_buf=ints(rng, (M, 3 * d)),
             y_buf=ints(rng, (M, 3 * d), 8), proj=[])
    for i, s in enumerate(c.order):
        pr = _projection(rng, d, d, 8, False, YSCALES[(s + i) % 2], SCALINGS[(s + M) % 2])
        _live_last_row(rng, o["x_buf"], o["dy_buf"][:, s * d:(s + 1) * d], pr, pr["yscale"] * pr["mag"] / pr["nrm"])
        o["proj"].append(pr)
    return o


def ln_operands(c):
    """x fp32 [M, d] (any finite rows: dgamma is not compared), integer dy, integer dbeta0."""
    rng = _rng(c)
    return dict(x=ints(rng, (c.M, c.d), 8), dy=ints(rng, (c.M, c.d)), dbeta0=rng.integers(-1000, 1001, size=c.d))


def ln_effective(o):
    return dict(dy=o["dy"].astype(np.int64), dbeta0=o["dbeta0"])


def effective(c):
    """[(label, effective operands)] of a case: one entry, or one per projection of a dora_grads_multi case."""
    if c.kernel == "wgrad":
        return [("", wgrad_effective(wgrad_operands(c)))]
    if c.kernel == "ln":
        return [("", ln_effective(ln_operands(c)))]
    if c.kernel == "dora_multi":
        o = multi_operands(c)
        return [(f"p{p}", adapter_effective(o, p)) for p in range(len(c.order))]
    return [("", adapter_effective(adapter_operands(c)))]


# ------------------------------------------------------------------------------------------------------ references
def _g(e):
    return e["yscale"] * e["mag"] / e["nrm"]


def _g_units(e):
    g = _g(e)
    gmin = float(g.min())
    gi = np.rint(g / gmin).astype(np.int64)
    assert np.array_equal(gi * gmin, g)
    return gmin, gi


def reference(kernel, e):
    """{name: float64 array}, exact.  ``e``: the effective operands."""
    if kernel == "wgrad":
        out = {"dw": (0 if e["dw0"] is None else e["dw0"]) + e["alpha"] * imatmul(e["dy"].T, e["x"])}
        if e["want_db"]:
            out["db"] = (0 if e["db0"] is None else e["db0"]) + e["alpha"] * e["dy"].sum(0)
        return {k: np.asarray(v, np.float64) for k, v in out.items()}
    if kernel == "ln":
        return {"dbeta": (e["dbeta0"] + e["dy"].sum(0)).astype(np.float64)}
    gmin, gi = _g_units(e)
    A, B = e["A"].astype(np.int64), e["B"].astype(np.int64)
    u = imatmul(e["x"], A.T)                                    # [M, r]
    vi = imatmul(e["dy"], gi[:, None] * B)                      # [M, r], units of gmin
    dA = e["scaling"] * gmin * imatmul(vi.T, e["x"])
    dB = e["scaling"] * _g(e)[:, None] * imatmul(e["dy"].T, u)
    dm = ((e["dy"] * e["y"]).sum(0) - e["bias"] * e["dy"].sum(0)) / e["mag"]
    return {"dA": dA.astype(np.float64), "dB": dB.astype(np.float64), "dm": dm.astype(np.float64)}


def check_ranges(kernel, e):
    """The operand rules and the exact range, on the effective operands of one case.  Raises AssertionError."""
    def below(v, what):
        assert float(np.max(v, initial=0)) < LIMIT, f"{what}: {float(np.max(v))} >= 2^24"

    dy = e["dy"]
    assert np.abs(dy).max() <= 3
    if kernel == "wgrad":
        x, a = e["x"], abs(e["alpha"])
        assert e["alpha"] in ALPHAS and np.abs(x).max() <= 3 and (x != 0).all()
        assert (dy.any(1) == (dy != 0).all(1)).all(), "dy rows are zero-free or all zero (junk rows)"
        unit = min(a, 1.0)            # everything is a multiple of it
        base = 0 if e["dw0"] is None else np.abs(e["dw0"])
        assert np.max(base, initial=0) <= 1000
        below(imatmul(np.abs(dy).T, np.abs(x)), "sum |dy| |x|")
        below((base + a * imatmul(np.abs(dy).T, np.abs(x))) / unit, "|dw0| + |alpha| sum |dy| |x| in units of min(|alpha|, 1)")
        if e["db0"] is not None:
            assert np.abs(e["db0"]).max() <= 1000
        return
    assert (dy != 0).all()
    if kernel == "ln":
        assert np.abs(e["dbeta0"]).max() <= 1000
        below(np.abs(e["dbeta0"]) + np.abs(dy).sum(0), "|dbeta0| + sum |dy|")
        return
    x, y, A, B = e["x"], e["y"], e["A"].astype(np.int64), e["B"].astype(np.int64)
    assert np.abs(x).max() <= 3 and (x != 0).all() and np.abs(y).max() <= 8 and (y != 0).all()
    assert set(np.unique(A)) <= {-1, 0, 1} and set(np.unique(B)) <= {-1, 0, 1}
    assert (A != 0).sum(1).max() <= 8 and (B != 0).sum(0).max() <= 8
    assert (A != 0).any(1).all() and (B != 0).any(0).all(), "no rank is idle"
    assert set(np.unique(e["mag"])) <= set(MAGS) and set(np.unique(e["nrm"])) <= set(NRMS)
    assert e["yscale"] in YSCALES and e["scaling"] in SCALINGS and np.abs(e["bias"]).max() <= 4
    gmin, gi = _g_units(e)
    u, vi = imatmul(x, A.T), imatmul(dy, gi[:, None] * B)
    assert significant_bits(u) <= 8, "u = x A^T needs more than 8 bits: not exact as bf16"
    assert significant_bits(vi) <= 8, "v = dy (g . B) needs more than 8 bits: not exact as bf16"
    assert significant_bits(gi[:, None] * B) <= 8
    below(imatmul(np.abs(x), np.abs(A).T), "sum |x| |A|")
    below(imatmul(np.abs(dy), gi[:, None] * np.abs(B)), "sum |dy| g |B| (units of min g)")
    below(imatmul(np.abs(vi).T, np.abs(x)), "sum |v| |x| (units of min g)")
    below(imatmul(np.abs(dy).T, np.abs(u)), "sum |dy| |u|")
    below((np.abs(dy) * np.abs(y)).sum(0) + np.abs(e["bias"]) * np.abs(dy).sum(0), "sum |dy y| + |b| sum |dy|")


def scrambled_f32(kernel, e, seed, groups=37):
    """The same quantities in fp32 numpy, rows permuted and summed in ``groups`` scrambled groups of unequal size, u and v
    rounded to bf16 as the kernels store them: {name: fp32 array}.  Must equal the reference bit for bit."""
    rng = np.random.default_rng(seed)
    M = e["dy"].shape[0]
    perm = rng.permutation(M)
    cuts = np.sort(rng.integers(0, M + 1, size=max(min(groups, M) - 1, 0)))
    parts = [p for p in np.split(perm, cuts) if p.size]
    f = lambda a: np.asarray(a, np.float32)
    acc = None
    for rows in parts:
        dy = f(e["dy"][rows])
        if kernel == "wgrad":
            part = [dy.T @ f(e["x"][rows]), dy.sum(0, dtype=np.float32)]
        elif kernel == "ln":
            part = [dy.sum(0, dtype=np.float32)]
        else:
            x, g = f(e["x"][rows]), f(_g(e))
            u = bf16_round(x @ f(e["A"]).T)
            v = bf16_round(dy @ bf16_round(g[:, None] * f(e["B"])))
            part = [v.T @ x, dy.T @ u, (dy * f(e["y"][rows])).sum(0, dtype=np.float32), dy.sum(0, dtype=np.float32)]
        acc = part if acc is None else [a + b for a, b in zip(acc, part)]
        assert all(a.dtype == np.float32 for a in acc)
    if kernel == "wgrad":
        al = np.float32(e["alpha"])
        out = {"dw": f(0 if e["dw0"] is None else e["dw0"]) + al * acc[0]}
        if e["want_db"]:
            out["db"] = f(0 if e["db0"] is None else e["db0"]) + al * acc[1]
        return out
    if kernel == "ln":
        return {"dbeta": f(e["dbeta0"]) + acc[0]}
    s, g, mag = np.float32(e["scaling"]), f(_g(e)), f(e["mag"])
    return {"dA": s * acc[0], "dB": s * g[:, None] * acc[1], "dm": (acc[2] - f(e["bias"]) * acc[3]) / mag}


# ------------------------------------------------------------------------------------------------------ mutations
def applicable(kernel, e):
    """The defects of MUTATIONS that exist for this case.  A defect that cannot occur or cannot show by construction is left
    out: swapped rows at M = 1; a swap in a plain row sum (ln: sum dy does not depend on the row order); the g of the
    neighbouring column in plain LoRA, where g is one constant; dw0 when nothing is pre-loaded; alpha applied twice at
    alpha = 1.  Every defect is applicable in at least one case of each kernel it can occur in (the host test checks)."""
    M = e["dy"].shape[0]
    m = ["row_dropped", "row_doubled", "dy_chunk_zeroed"]
    if kernel != "ln":
        m.append("x_chunk_zeroed")
        if M > 1:
            m += ["x_rows_swapped", "dy_rows_swapped"]
    if kernel == "wgrad":
        if e["dw0"] is not None:
            m.append("dw0_not_added")
        if e["alpha"] != 1.0:
            m.append("alpha_twice")
    if kernel in ("dora", "dora_multi", "adapter") and np.unique(_g(e)).size > 1:
        m.append("g_from_neighbour")
    return m


def mutate(kernel, e, which):
    """The effective operands with one defect: what a kernel with that defect would have summed.  The row is the last row
    that carries gradient (the ragged one of the last tile), the chunk its last 8 columns."""
    e = dict(e)
    dy = e["dy"]
    row = int(np.flatnonzero(dy.any(1))[-1])
    rowwise = [k for k in ("x", "dy", "y") if k in e]
    if which == "row_dropped":
        for k in rowwise:
            e[k] = np.delete(e[k], row, 0)
    elif which == "row_doubled":
        for k in rowwise:
            e[k] = np.concatenate([e[k], e[k][row:row + 1]], 0)
    elif which in ("x_chunk_zeroed", "dy_chunk_zeroed"):
        k = which[:-len("_chunk_zeroed")]
        e[k] = e[k].copy()
        e[k][row, -8:] = 0
    elif which in ("x_rows_swapped", "dy_rows_swapped"):
        k = which[:-len("_rows_swapped")]
        e[k] = e[k].copy()
        e[k][[row - 1, row]] = e[k][[row, row - 1]]
    elif which == "g_from_neighbour":      # column c takes the g of column c + 1: mag / nrm enter g, mag alone divides dm
        g = np.roll(_g(e), -1)
        e["nrm"] = e["yscale"] * e["mag"] / g
    elif which == "dw0_not_added":
        e["dw0"] = None
    elif which == "alpha_twice":
        e["alpha"] = e["alpha"] * e["alpha"]
    else:
        raise ValueError(which)
    return e


# ------------------------------------------------------------------------------------------------------ the table
WGRAD_M = (1, 63, 64, 65, 255, 256, 257, 513, 3001, 16385)
DORA_D = (128, 384, 512, 768, 1024, 1280)            # 128 / 1024 / 1280: k_dora_grads; 384 / 512 / 768: k_dora_grads_mfma
DORA_M = (1, 31, 32, 33, 255, 257, 8193)
DORA_LAYOUTS = ("plain", "q", "k", "v")
ADAPTER_R = (1, 8, 31, 32, 33, 64)
ADAPTER_M = (1, 31, 33, 129, 4097)
LN_D = (128, 640, 1280)
LN_M = (1, 3, 4, 5, 255, 257, 32769)


def _wgrad_cases():
    W = lambda **p: Case("wgrad", **p)
    out = [W(M=M, N=128, K=128) for M in WGRAD_M]                       # 16385: 52 slices, the last one 65 rows long
    out += [W(M=20161, N=128, K=128)]                                   # the cap of 64 slices, the last one a single row
    out += [W(M=M, N=N, K=K) for N, K in ((64, 16), (192, 144)) for M in (65, 257, 3001)]   # tiles ragged both ways
    out += [W(M=3001, N=384, K=384), W(M=777, N=1152, K=384)]
    out += [W(M=257, N=128, K=128, view="sections"), W(M=513, N=192, K=144, view="sections")]
    out += [W(M=2 * 151, N=128, K=384, view="conv2", B=2, Tn=150), W(M=2 * 302, N=128, K=256, view="conv1", B=2, Tin=300)]
    out += [W(M=257, N=128, K=128, view="rows")]
    out += [W(M=513, N=128, K=128, acc=True, alpha=a) for a in ALPHAS]
    out += [W(M=3001, N=192, K=144, acc=True, alpha=-2.0), W(M=65, N=64, K=16, acc=True, alpha=0.25, db=False)]
    out += [W(M=257, N=128, K=128, db=False)]
    return out


def _dora_cases():
    out = []
    for i, d in enumerate(DORA_D):
        D = lambda **p: Case("dora", d_in=d, d_out=d, r=8, **p)
        # every M once, the layouts and scales rotating so that every width meets each of them
        out += [D(M=M, layout=DORA_LAYOUTS[(i + j) % 4], yscale=YSCALES[(i + j) % 2], scaling=SCALINGS[(j // 2) % 2])
                for j, M in enumerate(DORA_M)]
        # every layout with both yscale at a ragged two-tile M, and a second packed section at the longest walk
        out += [D(M=33, layout=lay, yscale=ys, scaling=SCALINGS[1]) for lay in DORA_LAYOUTS for ys in YSCALES]
        out += [D(M=8193, layout="v" if DORA_LAYOUTS[(i + 6) % 4] != "v" else "q", yscale=YSCALES[(i + 1) % 2], scaling=4.0)]
    return list({c.id: c for c in out}.values())


def _multi_cases():
    out = []
    for d, nps in ((384, (1, 2, 3)), (512, (1, 2, 3)), (768, (1,))):
        for n in nps:
            fwd = {1: (1,), 2: (0, 2), 3: (0, 1, 2)}[n]
            for M in (31, 33, 8193):
                out.append(Case("dora_multi", d=d, M=M, order=fwd if M != 33 else fwd[::-1]))
            out.append(Case("dora_multi", d=d, M=33, order=fwd if n > 1 else (2,)))
    return out


def _adapter_cases():
    out, seen = [], set()
    shapes = [(k, d) for d in (128, 384) for k in ("square", "fc1", "fc2")] + [("square", 1280)]
    for i, (kind, d) in enumerate(shapes):
        d_in, d_out = {"square": (d, d), "fc1": (d, 4 * d), "fc2": (4 * d, d)}[kind]
        combos = [(r, 33) for r in ADAPTER_R] + [(8, M) for M in ADAPTER_M] + [(33, 4097), (64, 129), (32, 1), (1, 31)]
        for j, (r, M) in enumerate(combos):
            if (kind, d, r, M) in seen:
                continue
            seen.add((kind, d, r, M))
            out.append(Case("adapter", d_in=d_in, d_out=d_out, r=r, M=M, layout="strided" if (i + j) % 3 == 0 else "plain",
                            lora=(i + j) % 4 == 1, yscale=YSCALES[(i + j) % 2], scaling=SCALINGS[(j // 2) % 2]))
    return out


def _ln_cases():
    return [Case("ln", d=d, M=M, dy=t) for d in LN_D for M in LN_M for t in ("f32", "bf16")]


CASES = _wgrad_cases() + _dora_cases() + _multi_cases() + _adapter_cases() + _ln_cases()
assert len({c.id for c in CASES}) == len(CASES)


def cases(kernel):
    return [c for c in CASES if c.kernel == kernel]
