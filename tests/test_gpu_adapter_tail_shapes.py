"""The Q-adapter's tail (gww_qadapter_tail_f32 in csrc/qscan.hip, gww_qadapter_tail_backward_f32 in csrc/contrastive.hip)
at the output shapes ``QTransformAdapter(target_shape=...)`` accepts -- 128 mel bins, short contexts, time down-sampling,
Win at its limit -- against the fp64 torch composition, per element; the backward's four hand-computed adaptive-pool
regions pinned by impulse gradients; the scalar gradients against their conditioning; and gww_assemble_batch_f32 where
its grid-stride loop and its ragged last block run.

PyTorch's adaptive pooling: output index o of O covers the inputs [floor(o I / O), ceil((o + 1) I / O))."""

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
# (Hin, Win) -> (F, T)
SHAPES = [((128, 128), (128, 3000)), ((128, 128), (80, 1000)), ((512, 512), (80, 500)), ((33, 50), (128, 4096)),
          ((7, 4096), (80, 4)), ((200, 4000), (80, 1500)), ((1, 1), (1, 4)), ((128, 128), (80, 3000))]
IDS = [f"{a[0]}x{a[1]}-{b[0]}x{b[1]}" for a, b in SHAPES]
SCALE, BIAS, GAMMA, BETA, DET = 0.7, -0.2, (1.3, 0.8), (0.05, -0.1), 1


@pytest.fixture(scope="module")
def T():
    import torch
    assert torch.cuda.is_available()
    return torch


def _region(o, I, O):
    """[start, end) of output index o of O over I inputs, in integers."""
    return (o * I) // O, -((-(o + 1) * I) // O)


def _counts(T, I, O):
    """The number of inputs under each of the O outputs (int64 tensor [O])."""
    return T.tensor([_region(o, I, O)[1] - _region(o, I, O)[0] for o in range(O)], dtype=T.float64)


def _covering(T, I, O):
    """The number of outputs that cover each of the I inputs (float64 tensor [I])."""
    n = T.zeros(I, dtype=T.float64)
    for o in range(O):
        a, b = _region(o, I, O)
        n[a:b] += 1
    return n


def _params(T, grad=True):
    mk = lambda v: T.tensor(list(v) if isinstance(v, tuple) else [v], dtype=T.float32, device="cuda", requires_grad=grad)
    return mk(SCALE), mk(BIAS), mk(GAMMA), mk(BETA)


def _inputs(T, kind, B, Hin, Win):
    g = T.Generator().manual_seed(1000 * Hin + Win + (7 if kind == "offset" else 0))
    y = T.randn(B, Hin, Win, generator=g)
    if kind == "offset":                                   # a DC level of 100 and one loud pixel
        y += 100.0
        y[B - 1, Hin // 2, Win // 3] = 1e4
    return y


def _bits(t):
    return t.detach().cpu().contiguous().view(-1).numpy().view(np.uint32)


@pytest.mark.parametrize("kind", ["gaussian", "offset"])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_tail_forward_per_element(T, gww, shape, kind):
    """out[:, det] against ((scale pool(y) + bias) gamma + beta) in fp64, per element, within
        (rows + cols + 3) 2^-24 |scale gamma| mean_region |y| + 2^-23 (|scale gamma pool| + |bias gamma| + |beta|):
    the kernel adds a region's rows, then its columns, sequentially in fp32 (rows + cols roundings on a sum of |y|),
    scales by 1 / rows / cols (three roundings) and folds the affine into one fma of a = scale gamma and
    c0 = fma(bias, gamma, beta) (one rounding each, and the fma's own).  The other detector's plane stays untouched.

    Worst err / bound measured on an MI355X (gfx950), Gaussian y / offset y:
      128x128 -> 128x3000  0.916 / 0.161      7x4096 -> 80x4         0.003 / 0.020
      128x128 -> 80x1000   0.826 / 0.331      200x4000 -> 80x1500    0.332 / 0.335
      512x512 -> 80x500    0.318 / 0.280      1x1 -> 1x4             0.020 / 0.105
      33x50 -> 128x4096    0.821 / 0.197      128x128 -> 80x3000     0.826 / 0.331
    The ratios above 0.8 are elements of one-pixel regions with y near 0: the result is c0 within 0.26 <= |c0| < 0.5,
    whose two roundings (c0 and the fma, 2^-26 each) are 0.96 of the bound's 2^-23 (|bias gamma| + |beta|) = 2^-23 0.26."""
    from gw_whisper_amd.qscan import _AdapterTail
    (Hin, Win), (F, Tn) = shape
    B, D = 2, 2
    y = _inputs(T, kind, B, Hin, Win)
    scale, bias, gamma, beta = _params(T, grad=False)
    out = T.full((B, D, F, Tn), 7.0, device="cuda")
    out = _AdapterTail.apply(y.cuda(), scale, bias, gamma, beta, out, DET)
    got = out.cpu()
    assert (got[:, 1 - DET] == 7.0).all()
    pool = T.nn.functional.adaptive_avg_pool2d
    s, b_, ga, be = (float(np.float32(v)) for v in (SCALE, BIAS, GAMMA[DET], BETA[DET]))
    p = pool(y.double()[:, None], (F, Tn))[:, 0]
    ref = (s * p + b_) * ga + be
    pabs = pool(y.double().abs()[:, None], (F, Tn))[:, 0]
    cnt = _counts(T, Hin, F)[:, None] + _counts(T, Win, Tn)[None, :]
    bound = (cnt + 3) * U * abs(s * ga) * pabs + 2.0 ** -23 * ((s * ga * p).abs() + abs(b_ * ga) + abs(be))
    ratio = ((got[:, DET].double() - ref).abs() / bound).max().item()
    print(f"adapter tail forward {kind} {Hin}x{Win} -> {F}x{Tn}: worst err / bound {ratio:.3f}")
    assert T.isfinite(got).all() and ratio <= 1.0


def _impulses(Hin, Win, F, Tn):
    """(f, t) of the impulse gradients: the corners, t = 255, 256, 257 and T - 1, the first f whose region starts a new
    input row, every f whose region holds the last input row, three seeded positions."""
    rng = np.random.default_rng(Hin * 31 + Win * 7 + F + Tn)
    pos = [(0, 0), (0, Tn - 1), (F - 1, 0), (F - 1, Tn - 1)]
    pos += [(F // 2, t) for t in (255, 256, 257, Tn - 1) if t < Tn]
    new_row = [f for f in range(1, F) if _region(f, Hin, F)[0] != _region(f - 1, Hin, F)[0]]
    if new_row:
        pos.append((new_row[0], Tn // 3))
    pos += [(f, int(rng.integers(Tn))) for f in range(F) if _region(f, Hin, F)[1] == Hin]
    pos += [(int(rng.integers(F)), int(rng.integers(Tn))) for _ in range(3)]
    return pos


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_tail_backward_on_impulse_gradients(T, gww, shape):
    """One launch, one impulse per batch element: g[b] is 1 at (f, t) and 0 elsewhere, handed over as the strided view
    g_out[:, det] of a [B, 2, F, T] tensor.  d_y[b] must be nonzero exactly on PyTorch's region of (f, t), computed here
    in integers, and equal scale gamma / (rows cols) there to 2 ulp.  The positions (``_impulses``) pin the four
    floor / ceil expressions of the kernel: the forward map of rows and of columns, and the inverse of each.

    Worst error in ulp measured on an MI355X (gfx950): 1.44 at 200x4000 -> 80x1500, 1.38 at 512x512 -> 80x500 (regions of
    3 x 3 and 7 x 2 inputs: 1 / rows, 1 / cols, their product, scale gamma and the last product each round), 0.06 to 0.08 at
    the other six shapes, whose regions have one or two rows and columns (or 1024 columns: powers of two)."""
    from gw_whisper_amd import ops
    (Hin, Win), (F, Tn) = shape
    pos = _impulses(Hin, Win, F, Tn)
    nb = len(pos)
    scale, bias, gamma, _ = _params(T, grad=False)
    g_out = T.zeros(nb, 2, F, Tn, device="cuda")
    bi = T.arange(nb, device="cuda")
    g_out[bi, DET, T.tensor([p[0] for p in pos], device="cuda"), T.tensor([p[1] for p in pos], device="cuda")] = 1.0
    y = T.randn(nb, Hin, Win, generator=T.Generator().manual_seed(3)).cuda()
    view = g_out[:, DET]
    assert not view.is_contiguous() or nb == 1
    d_y = ops.qadapter_tail_backward(view, y, scale, bias, gamma[DET:DET + 1], F, Tn)[0]
    a = float(np.float32(SCALE)) * float(np.float32(GAMMA[DET]))
    want = T.zeros(nb, Hin, Win, dtype=T.float64)
    for b, (f, t) in enumerate(pos):
        (r0, r1), (k0, k1) = _region(f, Hin, F), _region(t, Win, Tn)
        assert 0 <= r0 < r1 <= Hin and 0 <= k0 < k1 <= Win
        want[b, r0:r1, k0:k1] = a / ((r1 - r0) * (k1 - k0))
    got = d_y.cpu()
    wrong = (got != 0) != (want != 0)
    assert not wrong.any(), [(pos[b], h, w) for b, h, w in wrong.nonzero().tolist()[:8]]
    ulp = T.from_numpy(np.spacing(want.abs().float().numpy())).double()
    worst = ((got.double() - want).abs() / ulp)[want != 0].max().item()
    print(f"adapter tail backward impulses {Hin}x{Win} -> {F}x{Tn}: {nb} impulses, worst error {worst:.2f} ulp")
    assert worst <= 2.0


def _dense_reference(T, y, w, F, Tn):
    """fp64 gradients of sum(w * tail(y)) and their conditioning: d_y, (d_scale, d_bias, d_gamma, d_beta), the d_y of
    |w| under |scale gamma| (every summand of d_y taken positive), sum |w pool(y)| and sum |w|."""
    pool = T.nn.functional.adaptive_avg_pool2d
    s, b_, ga = (float(np.float32(v)) for v in (SCALE, BIAS, GAMMA[DET]))
    y64, w64 = y.double().requires_grad_(True), w.double()
    p = pool(y64[:, None], (F, Tn))[:, 0]
    d_y = T.autograd.grad((p * w64).sum(), y64)[0] * (s * ga)
    y_abs = y.double().requires_grad_(True)
    d_y_abs = T.autograd.grad((pool(y_abs[:, None], (F, Tn))[:, 0] * w64.abs()).sum(), y_abs)[0] * abs(s * ga)
    p = p.detach()
    Sgp, Sg, Agp, Ag = (w64 * p).sum().item(), w64.sum().item(), (w64 * p).abs().sum().item(), w64.abs().sum().item()
    scalars = dict(d_scale=(ga * Sgp, abs(ga) * Agp), d_bias=(ga * Sg, abs(ga) * Ag),
                   d_gamma=(s * Sgp + b_ * Sg, abs(s) * Agp + abs(b_) * Ag), d_beta=(Sg, Ag))
    return d_y, d_y_abs, scalars


@pytest.mark.parametrize("centred", [False, True], ids=["plain", "zero-sum"])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_tail_backward_on_dense_gradients(T, gww, shape, centred):
    """_AdapterTail under autograd (so the kernel gets the strided view g_out[:, det] the module passes) on a Gaussian
    upstream gradient, and on one whose sum over the detector's plane is made to vanish (g -= g.mean()), against fp64:

      d_y per element within 1e-5 of its row's largest reference entry + cols 2^-24 sum_region |g|, where cols is the
      number of output columns over the element and sum_region |g| the same gather with every summand taken positive
      (|scale gamma| sum |g_ft| / (rows_f cols_t)): the kernel adds a row of the region sequentially in fp32;
      d_scale = gamma sum g pool(y) within 2^-22 |gamma| sum |g pool(y)|, and by the same reasoning (fp64 partial sums,
      one fp32 rounding of the result, so a 2^-22 share of the sum of magnitudes is ample and does not depend on the sum's
      own value) d_bias = gamma sum g within 2^-22 |gamma| sum |g|, d_beta = sum g within 2^-22 sum |g|, and
      d_gamma = scale sum g pool(y) + bias sum g within 2^-22 (|scale| sum |g pool(y)| + |bias| sum |g|);
      the other detector's FiLM gradients exactly 0; a second call gives identical bits.

    Worst err / bound measured on an MI355X (gfx950) over the eight shapes: d_y 0.027, d_scale 0.009, d_bias 0.057,
    d_gamma 0.037, d_beta 0.053 on the plain gradient; on the zero-sum one (sum g between 3e-8 and 2e-2 of a sum |g|
    between 8.5 and 1.25e6) d_y 0.027, d_scale 0.009, d_gamma 0.004, d_bias and d_beta below 0.0005."""
    from gw_whisper_amd.qscan import _AdapterTail
    (Hin, Win), (F, Tn) = shape
    B, D = 3, 2
    y = _inputs(T, "gaussian", B, Hin, Win)
    gen = T.Generator().manual_seed(Hin + 3 * Win + 5 * F + 7 * Tn)
    w = T.randn(B, D, F, Tn, generator=gen)
    w[:, DET] += 0.25
    if centred:
        w[:, DET] -= w[:, DET].mean()
    yc = y.cuda().requires_grad_(True)
    leaves = [yc, *_params(T)]
    wc = w.cuda()
    runs = []
    for _ in range(2):
        out = _AdapterTail.apply(yc, *leaves[1:], T.zeros(B, D, F, Tn, device="cuda"), DET)
        runs.append([t.cpu() for t in T.autograd.grad((out * wc).sum(), leaves)])
    for a, b in zip(*runs):
        assert np.array_equal(_bits(a), _bits(b)), "two calls differ"
    d_y, d_scale, d_bias, d_gamma, d_beta = runs[0]
    assert d_gamma[1 - DET].item() == 0.0 and d_beta[1 - DET].item() == 0.0
    ref_dy, abs_dy, scalars = _dense_reference(T, y, w[:, DET], F, Tn)
    cols = _covering(T, Win, Tn)[None, None, :]
    bound = 1e-5 * ref_dy.abs().max(2, keepdim=True).values + cols * U * abs_dy
    ratios = {"d_y": ((d_y.double() - ref_dy).abs() / bound).max().item()}
    got = dict(d_scale=d_scale[0], d_bias=d_bias[0], d_gamma=d_gamma[DET], d_beta=d_beta[DET])
    for k, (ref, cond) in scalars.items():
        ratios[k] = abs(got[k].double().item() - ref) / (2.0 ** -22 * cond)
    print(f"adapter tail backward dense {'zero-sum' if centred else 'plain'} {Hin}x{Win} -> {F}x{Tn}: sum g "
          f"{scalars['d_beta'][0]:.3e} of sum |g| {scalars['d_beta'][1]:.3e}; err / bound "
          + "  ".join(f"{k} {v:.3f}" for k, v in ratios.items()))
    assert all(T.isfinite(t).all() for t in runs[0])
    assert all(v <= 1.0 for v in ratios.values()), ratios


@pytest.mark.parametrize("target", [(128, 3000), (80, 1000)], ids=["128x3000", "80x1000"])
def test_adapter_module_at_other_target_shapes(T, gww, target):
    """QTransformAdapter.train_variant(n_detectors=2, target_shape=...) end to end, in two parts that share no allowance.

    The tail: the module's output and its gradients of scale, bias, film_gamma and film_beta against AdaptiveAvgPool2d ->
    affine -> FiLM in fp64 on the y that the module's own HIP CNN gives (``cnn_forward``) on the Q-scan maps the module
    computes (``q_transform(x[:, i])``), under the bounds of the tests above, unchanged: the forward bound per element,
    2^-22 of the conditioning per scalar gradient and detector, and one fp32 addition (2^-24 of the sum) where autograd
    adds the two detectors' d_scale and d_bias.  Q-scan and CNN repeat their bits, so this y is the y the module pooled.
    The CNN: that y against ``freq_adapter`` in fp64 on the same maps, to 1e-4 of max |y|, the bound of
    tests/test_gpu_qscan.py for its bf16-pair operands.

    Worst err / bound measured on an MI355X (gfx950), target (128, 3000) / (80, 1000): output 0.924 / 0.924 (an element
    with y near 0, as in test_tail_forward_per_element); scale 7.3e-5 / 8.9e-5, bias 1.2e-4 / 6.7e-5, film_gamma
    4.5e-5 / 2.4e-5, film_beta 6.3e-5 / 5.1e-5 (the kernel's sums are fp64, and the upstream gradient has zero mean, so
    2^-22 of the conditioning is about 2e-4 of a gradient's own size); CNN 0.099 / 0.099."""
    from gw_whisper_amd.qscan import QTransformAdapter
    T.manual_seed(17)
    F, Tn = target
    B, D = 2, 2
    ad = QTransformAdapter.train_variant(n_detectors=D, target_shape=target).cuda()
    with T.no_grad():
        ad.scale.fill_(SCALE), ad.bias.fill_(BIAS)
        ad.film_gamma.copy_(T.tensor(GAMMA)), ad.film_beta.copy_(T.tensor(BETA))
    x = T.randn(B, D, 2048, device="cuda")
    out = ad(x)
    assert out.shape == (B, D, F, Tn) and T.isfinite(out).all()
    w = T.randn(B, D, F, Tn, generator=T.Generator().manual_seed(23))
    names = ("scale", "bias", "film_gamma", "film_beta")
    grads = T.autograd.grad((out * w.cuda()).sum(), [getattr(ad, k) for k in names])
    got = {k: g.cpu().double() for k, g in zip(names, grads)}
    with T.no_grad():
        qs = [ad.q_transform(x[:, i]) for i in range(D)]
        ys = [ad.cnn_forward(q).double().cpu() for q in qs]
    pool = T.nn.functional.adaptive_avg_pool2d
    s, b_ = float(np.float32(SCALE)), float(np.float32(BIAS))
    ref = {k: T.zeros_like(v) for k, v in got.items()}
    cond = {k: T.zeros_like(v) for k, v in got.items()}
    worst = 0.0
    for i, y in enumerate(ys):
        ga, be = float(np.float32(GAMMA[i])), float(np.float32(BETA[i]))
        Hin, Win = y.shape[1:]
        p, pabs = pool(y[:, None], (F, Tn))[:, 0], pool(y.abs()[:, None], (F, Tn))[:, 0]
        cnt = _counts(T, Hin, F)[:, None] + _counts(T, Win, Tn)[None, :]
        bound = (cnt + 3) * U * abs(s * ga) * pabs + 2.0 ** -23 * ((s * ga * p).abs() + abs(b_ * ga) + abs(be))
        worst = max(worst, ((out[:, i].detach().cpu().double() - ((s * p + b_) * ga + be)).abs() / bound).max().item())
        g = w[:, i].double()
        Sgp, Sg, Agp, Ag = (g * p).sum().item(), g.sum().item(), (g * p).abs().sum().item(), g.abs().sum().item()
        ref["scale"] += ga * Sgp
        cond["scale"] += 2.0 ** -22 * abs(ga) * Agp
        ref["bias"] += ga * Sg
        cond["bias"] += 2.0 ** -22 * abs(ga) * Ag
        ref["film_gamma"][i] = s * Sgp + b_ * Sg
        cond["film_gamma"][i] = 2.0 ** -22 * (abs(s) * Agp + abs(b_) * Ag)
        ref["film_beta"][i] = Sg
        cond["film_beta"][i] = 2.0 ** -22 * Ag
    cond["scale"] += U * ref["scale"].abs() * (D - 1)
    cond["bias"] += U * ref["bias"].abs() * (D - 1)
    ratios = {k: ((got[k] - ref[k]).abs() / cond[k]).max().item() for k in names}
    cnn = ad.freq_adapter.double().cpu()
    with T.no_grad():
        y64 = [cnn(q.double().cpu()[:, None])[:, 0] for q in qs]
    ad.freq_adapter.float().cuda()
    r_cnn = max(((a - b).abs().max() / (1e-4 * b.abs().max())).item() for a, b in zip(ys, y64))
    print(f"adapter module target {F}x{Tn}: worst output err / bound {worst:.3f}; gradients "
          + "  ".join(f"{k} {v:.1e}" for k, v in ratios.items()) + f"; CNN err / (1e-4 max |y|) {r_cnn:.3f}")
    assert worst <= 1.0 and all(v <= 1.0 for v in ratios.values()) and r_cnn <= 1.0, (worst, ratios, r_cnn)


def test_batch_assembly_stride_loop_and_ragged_tail(T, gww):
    """gww_assemble_batch_f32 at a row of 262 144 + 257 samples: the grid covers 1024 x 256 elements of a row, so the
    stride loop runs a second time and its last block is ragged.  Bit for bit fp32 ``noise + snr * wave`` (two roundings,
    torch on the CPU) at snr 7.3, 0.0 and -0.0, and a noise-only row (idx_wave < 0)."""
    from gw_whisper_amd import ops
    L = 262144 + 257
    gen = T.Generator().manual_seed(29)
    noise, wave = T.randn(2, L, generator=gen), T.randn(1, L, generator=gen)
    noise[1, -1], noise[0, 262144] = -0.0, 0.0
    nd, wd = noise.cuda(), wave.cuda()
    for idx_n, idx_w, snr in (([0, 1], [0, -1], [7.3, 7.3]), ([1, 0], [0, 0], [0.0, -0.0])):
        out = ops.assemble_batch(nd, wd, idx_n, idx_w, snr).cpu()
        assert out.shape == (2, L)
        for r in range(2):
            want = noise[idx_n[r]] if idx_w[r] < 0 else noise[idx_n[r]] + T.tensor(snr[r], dtype=T.float32) * wave[idx_w[r]]
            bad = np.flatnonzero(_bits(out[r]) != _bits(want))
            assert bad.size == 0, (idx_n[r], idx_w[r], snr[r], bad[:8], bad.size)
