"""GPU checks of the detection head step, the evaluation / efficiency statistics kernels (csrc/detect.hip), the device
pipeline of gw_whisper_amd/efficiency.py and the two programs (harness/run_efficiency_train.py,
harness/run_efficiency_estimate.py).

The head step follows the rule of tests/test_gpu_glitch.py: the HIP step and the torch fp32 head it can replace
(``models.efficiency_classifier``'s nn.Sequential + ``inference.RegBCELoss``) are both fp32 chains that differ in summation
order, so neither is privileged.  Both are measured against fp64 on the same inputs in the same test and
    err_hip <= 2 * err_torch + floor
with floor = 20 * 2^-24 * max|logit| for the logits (maximum error) and 20 * 2^-24 for the probabilities (maximum error),
the loss, the row losses, every parameter gradient and the pooled-token gradient (relative Frobenius error): the project's
4 * 2^-24 per chained fp32 dot product, for five.  The fp64 side is efficiency_helpers.head64, which
tests/test_efficiency_host.py pins to the reference's own head class and loss through tests/golden/efficiency.npz; logits,
probs and loss of the fixture cases are compared with the stored values directly.  Every case asserts that no hidden
pre-activation of its inputs is within 2e-6 of zero before anything is compared (the ReLU condition of DESIGN.md
section 15).

The statistics kernels are integer selections and counts: they are compared with numpy on the same fp32 arrays for
equality, nothing else."""

import os
import subprocess
import sys

import numpy as np
import pytest

from . import efficiency_helpers as eh

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS20 = 20.0 * 2.0 ** -24


@pytest.fixture(scope="module")
def T():
    import torch
    assert torch.cuda.is_available()
    return torch


def _rel(a, ref):
    """Relative Frobenius error in fp64; 0 when both are exactly zero."""
    d = float((a.double() - ref.double()).norm())
    n = float(ref.double().norm())
    return 0.0 if d == 0.0 else d / n if n > 0 else float("inf")


def _torch_head(T, params, x, t, epsilon, upstream):
    """The torch fp32 head the HIP step can replace, with autograd."""
    from gw_whisper_amd.inference import RegBCELoss
    from gw_whisper_amd.models import efficiency_classifier
    d_in, C = params[0].shape[1], params[8].shape[0]
    enc = type("Enc", (), {"config": type("Cfg", (), {"d_model": d_in})()})()      # the head only reads config.d_model
    cls = efficiency_classifier(enc, num_classes=C).classifier.to(x.device)
    cls.load_state_dict({k: p for k, p in zip(eh.PARAM_KEYS, params)})
    xr = x.detach().clone().requires_grad_(True)
    z = T.nn.Sequential(*list(cls.children())[:-1])(xr)
    p = cls[-1](z)
    loss = RegBCELoss(epsilon=epsilon, dim=C)(p, t)
    (loss * upstream).backward()
    sd = cls.state_dict(keep_vars=True)
    q = epsilon + (1.0 - epsilon * C) * p.detach()
    rows = T.nn.functional.binary_cross_entropy(q, t, reduction="none").sum(1)
    return loss.detach(), z.detach(), p.detach(), rows, xr.grad, [sd[k].grad for k in eh.PARAM_KEYS]


def _compare(T, tag, x, params, t, epsilon=eh.EPSILON, upstream=1.0, fixture=None):
    """One head step three ways; prints both errors of every quantity, asserts the rule.  Returns the HIP outputs."""
    from gw_whisper_amd import ops
    B, C = t.shape
    g = T.tensor([upstream], dtype=T.float32, device=x.device)
    loss, logits, probs, row_loss, saved = ops.det_head_forward(x, params, t, epsilon)
    dx, grads = ops.det_head_backward(saved, g)
    l64, z64, p64, dx64, g64, margin = eh.head64(x, params, t, epsilon, upstream)
    assert margin >= 2e-6, f"{tag}: a hidden pre-activation of the test's own inputs is {margin:.2e} from zero"
    q64 = epsilon + (1.0 - epsilon * C) * p64
    rows64 = T.nn.functional.binary_cross_entropy(q64, t.double(), reduction="none").sum(1)
    if fixture is not None:       # the stored fp64 values of the reference's head class and loss
        z64, p64 = T.from_numpy(fixture[0]).to(x.device), T.from_numpy(fixture[1]).to(x.device)
        l64 = T.tensor(float(fixture[2]), dtype=T.float64, device=x.device)
    lt, zt, pt, rowst, dxt, gt = _torch_head(T, params, x, t, epsilon, upstream)
    zmax = float(z64.abs().max())
    for name, a, b, c, floor in (("logits", logits, zt, z64, EPS20 * zmax), ("probs", probs, pt, p64, EPS20)):
        e_hip, e_t = float((a.double() - c).abs().max()), float((b.double() - c).abs().max())
        print(f"{tag}: {name} max err hip {e_hip:.2e} torch {e_t:.2e} (max|logit| {zmax:.3f})")
        assert e_hip <= 2 * e_t + floor, (tag, name, e_hip, e_t)
    rows = [("loss", loss.reshape(()), lt, l64), ("row_loss", row_loss, rowst, rows64), ("d_pooled", dx, dxt, dx64)]
    rows += [(f"d_{k}", a, b, c) for k, a, b, c in zip(eh.PARAM_KEYS, grads, gt, g64)]
    for name, a, b, c in rows:
        assert bool(T.isfinite(a).all()), (tag, name)
        eh_, et = _rel(a, c), _rel(b, c)
        print(f"{tag}: {name:12s} rel err hip {eh_:.2e} torch {et:.2e}")
        assert eh_ <= 2 * et + EPS20, (tag, name, eh_, et)
    # the batch mean is the fp64 sum of the fp32 row losses over B C, rounded once
    assert abs(float(loss) - float(row_loss.double().sum()) / (B * C)) <= 2.0 ** -23 * abs(float(loss))
    return loss, logits, probs, row_loss, saved, dx, grads


def _fixture_case(T, g, ci):
    d_in, C, B = g["head_cases"][ci].tolist()
    x, t = eh.case_inputs(d_in, C, B, int(g["head_seeds"][ci]))
    return T.from_numpy(x).cuda(), T.from_numpy(t).cuda(), [T.from_numpy(p).cuda() for p in eh.case_params(ci, d_in, C)]


@pytest.mark.parametrize("ci", range(len(eh.CASES)))
def test_head_step_against_the_fixture(T, gww, golden, ci):
    """(d_in, C, B) = (384,2,32), (512,2,32), (1280,2,7), (128,2,1), (384,2,1000), (384,3,33), (256,64,17); one-hot targets,
    epsilon 1e-6.  Measured on MI355X, worst of the seven cases, HIP / torch: logits 4.3e-8 / 4.5e-8 (max|logit| 0.10, floor
    1.2e-7), probs 3.9e-8 / 5.3e-8, loss 5.6e-8 / 9.7e-8, last-layer bias gradient 5.6e-7 / 6.0e-6 relative
    (profiles/efficiency_train.md)."""
    g = golden("efficiency.npz")
    assert tuple(g["head_cases"][ci].tolist()) == eh.CASES[ci]
    x, t, params = _fixture_case(T, g, ci)
    _compare(T, f"case {ci} {eh.CASES[ci]}", x, params, t,
             fixture=(g[f"head{ci}_logits"], g[f"head{ci}_probs"], g[f"head{ci}_loss"]))


def test_head_step_soft_targets_and_upstream_gradient(T, gww, golden):
    """Targets anywhere in [0, 1] (with exact 0 and 1 among them), three classes, upstream gradient 0.37."""
    g = golden("efficiency.npz")
    x, t, params = _fixture_case(T, g, 5)
    soft = T.rand(t.shape, generator=T.Generator().manual_seed(5)).cuda()
    soft[0], soft[1] = t[0], 1.0 - t[1]
    _compare(T, "soft targets, upstream 0.37", x, params, soft, upstream=0.37)


def _gap_case(T, g, ci, row, gap):
    d_in, C, B = eh.CASES[ci]
    x, t = eh.case_inputs(d_in, C, B, int(g["head_seeds"][ci]))
    params = eh.with_gap(x, eh.case_params(ci, d_in, C), row, gap)
    t[row] = (0.0, 1.0)          # the row is confident in class 0: label it class 1
    x, t, params = T.from_numpy(x).cuda(), T.from_numpy(t).cuda(), [T.from_numpy(p).cuda() for p in params]
    z = eh.head64(x, params, t)[1]
    return x, t, params, float(z[row, 0] - z[row, 1]), float((z[:, 0] - z[:, 1]).abs().sort().values[-2])


def test_head_step_confident_and_wrong_row(T, gww, golden):
    """One row with a logit gap of 14 against its label at epsilon = 1e-6: log(1 - q) of its confident lane is where torch's
    fp32 1 - q cancels (its loss is ~3e-4 relative off fp64 on the CPU); the HIP step forms 1 - q from the other lane's
    exponential and must be no worse."""
    x, t, params, gap, second = _gap_case(T, golden("efficiency.npz"), 0, 5, 14.0)
    assert abs(gap - 14.0) < 1e-3 and second < 1.0
    loss, _, probs, row_loss, *_ = _compare(T, "gap 14", x, params, t)
    assert float(row_loss[5]) > 13.0


def test_head_step_epsilon_zero_clamped_row(T, gww, golden):
    """epsilon = 0 and a row with a logit gap of 120 against its label: p rounds to exactly 1 and 0, both logs clamp at
    -100 (row loss 200), and the gradient is finite.  Torch's fp32 gradient of that row is exactly zero (its p underflows);
    in exact arithmetic it is p_1 / 1e-12 / (B C) ~ 1e-42, and that -- a denormal at most -- is all the HIP step may leave
    there."""
    x, t, params, gap, second = _gap_case(T, golden("efficiency.npz"), 1, 7, 120.0)
    assert abs(gap - 120.0) < 1e-2 and second < 1.0
    loss, logits, probs, row_loss, saved, dx, grads = _compare(T, "gap 120, epsilon 0", x, params, t, epsilon=0.0)
    lt, zt, pt, rowst, dxt, gt = _torch_head(T, params, x, t, 0.0, 1.0)
    assert probs[7].tolist() == [1.0, 0.0] == pt[7].tolist()
    assert float(row_loss[7]) == 200.0 == float(rowst[7])
    assert float(saved[3][7].abs().max()) < 1e-37 and float(dx[7].abs().max()) < 1e-37 and bool((dxt[7] == 0).all())
    assert bool(T.isfinite(lt)) and abs(float(loss) - float(lt)) <= 1e-6 * float(lt)


def test_head_step_is_deterministic_and_scores_equal_the_forward(T, gww, golden):
    """A second identical call gives identical bits; scores mode 0 / 1 equal probs[:, 0] / z0 - z1 of the forward bit for
    bit, written into a strided slice of a larger buffer whose other elements stay untouched."""
    from gw_whisper_amd import ops
    g = golden("efficiency.npz")
    for ci in (0, 2, 4):
        x, t, params = _fixture_case(T, g, ci)
        B = x.shape[0]
        up = T.tensor([0.5], device="cuda")
        outs = []
        for _ in range(2):
            loss, logits, probs, row_loss, saved = ops.det_head_forward(x, params, t)
            dx, grads = ops.det_head_backward(saved, up)
            outs.append([loss, logits, probs, row_loss, dx, *grads, *saved[2], saved[3]])
        for a, b in zip(*outs):
            assert T.equal(a, b)
        for mode, ref in ((ops.SCORE_PROB0, probs[:, 0]), (ops.SCORE_LOGIT_DIFF, logits[:, 0] - logits[:, 1])):
            buf = T.full((3 * B + 5,), float("nan"), device="cuda")
            view = buf[2:2 + 3 * B:3]
            assert view.shape[0] == B and (B == 1 or view.stride(0) == 3)
            ops.det_head_scores(x, params, view, mode)
            assert T.equal(view, ref), (ci, mode)
            mask = T.ones_like(buf, dtype=T.bool)
            mask[2:2 + 3 * B:3] = False
            assert bool(T.isnan(buf[mask]).all())
    x, t, params = _fixture_case(T, g, 5)        # C = 3: mode 0 only
    _, _, probs, _, _ = ops.det_head_forward(x, params, t)
    out = T.empty(33, device="cuda")
    assert T.equal(ops.det_head_scores(x, params, out, ops.SCORE_PROB0), probs[:, 0])
    with pytest.raises(gww.GwwError, match="C = 2"):
        ops.det_head_scores(x, params, out, ops.SCORE_LOGIT_DIFF)


# ------------------------------------------------------------------------------------------------ statistics
def _score_array(kind, N, seed):
    rng = np.random.default_rng(seed)
    if kind == "normal":
        return rng.standard_normal(N).astype(np.float32)
    if kind == "equal":
        return np.full(N, -2.5, np.float32)
    if kind == "duplicated":
        return rng.integers(-2, 2, N).astype(np.float32)
    a = rng.standard_normal(N).astype(np.float32)         # "special"
    special = [np.nan, np.inf, -np.inf, 1e-40, -1e-42, 0.0, -0.0, 1.4e-45, np.float32(3.4e38)]
    pos = rng.permutation(N)[:len(special)]
    for p, v in zip(pos, special):
        a[p] = v
    return a


def _same(a, b):
    return bool(((a == b) | (np.isnan(a) & np.isnan(b))).all())       # == : +0 and -0 are equal


@pytest.mark.parametrize("N", [1, 2, 255, 256, 257, 4099, 70001])
def test_score_thresholds_equal_numpy(T, gww, N):
    """thr[f] == sort(scores)[N - rank] (rank 0: sort(scores)[0]) exactly, for F in {1, 5, 8}, ranks among them 0, 1 and N,
    on random, all-equal, heavily duplicated arrays and one with negatives, denormals, +-0, +-inf and one NaN."""
    from gw_whisper_amd import ops
    rng = np.random.default_rng(N)
    for kind in ("normal", "equal", "duplicated", "special"):
        a = _score_array(kind, N, 100 + N)
        srt = np.sort(a)                                   # NaN last, as torch.sort
        d = T.from_numpy(a).cuda()
        for F in (1, 5, 8):
            ranks = np.concatenate(([0, 1, N, max(N // 2, 1), min(2, N)], rng.integers(0, N + 1, 3)))[:F].astype(np.int64)
            if F == 1:
                ranks = np.asarray([[0, 1, N, N // 3][("normal", "equal", "duplicated", "special").index(kind)]], np.int64)
            ref = np.asarray([srt[N - r] if r > 0 else srt[0] for r in ranks], np.float32)
            thr = ops.score_thresholds(d, T.from_numpy(ranks).cuda()).cpu().numpy()
            assert _same(thr, ref), (kind, N, F, ranks.tolist(), thr.tolist(), ref.tolist())
    if N >= 255:       # the NaN is the largest: rank 1 selects it, rank 2 the +inf below it
        a = _score_array("special", N, 100 + N)
        thr = ops.score_thresholds(T.from_numpy(a).cuda(), T.tensor([1, 2], device="cuda")).cpu().numpy()
        assert np.isnan(thr[0]) and thr[1] == np.inf


@pytest.mark.parametrize("B", [1, 33, 1000])
def test_detection_counts_equal_numpy(T, gww, B):
    """counts[f] += #{scores > thr[f]} with scores placed exactly on a threshold (strict), a NaN score and a NaN threshold,
    accumulated over three calls into one row of an [S, F] table whose other rows stay zero."""
    from gw_whisper_amd import ops
    rng = np.random.default_rng(B)
    for F in (1, 5, 8):
        thr = np.sort(rng.standard_normal(F)).astype(np.float32)
        if F == 8:
            thr[3] = np.nan
            thr[5] = np.inf
        table = T.zeros((3, F), dtype=T.int64, device="cuda")
        ref = np.zeros(F, np.int64)
        for call in range(3):
            s = rng.standard_normal(B).astype(np.float32)
            s[rng.permutation(B)[:max(B // 3, 1)]] = thr[call % F]        # exactly on a threshold
            if B > 1:
                s[1] = np.nan if call == 0 else np.inf
            with np.errstate(invalid="ignore"):
                ref += (s[:, None] > thr[None, :]).sum(0)
            ops.detection_counts(T.from_numpy(s).cuda(), T.from_numpy(thr).cuda(), table[1])
        got = table.cpu().numpy()
        assert np.array_equal(got[1], ref), (B, F, got[1].tolist(), ref.tolist())
        assert not got[0].any() and not got[2].any()


def test_eval_accumulate_against_torch(T, gww, golden):
    """Batches of 32, 32 and 5 rows with an argmax tie (lowest index wins) and a NaN row (NaN is the maximum): correct, n
    and batches equal the torch composition exactly; loss_sum is the sum over batches of the batch's mean loss rounded
    to fp32, which is what the reference's ``valid_loss += loss.item()`` adds (within one fp32 rounding per batch of the
    fp64 composition), and equals the sum of the head forward's own ``loss`` outputs bit for bit."""
    from gw_whisper_amd import efficiency, ops
    C = 3
    gen = T.Generator(device="cuda").manual_seed(3)
    state = efficiency.EvalState("cuda")
    ref_correct, ref_sum, ref_n = 0, 0.0, 0
    for B in (32, 32, 5):
        p = T.softmax(T.randn(B, C, generator=gen, device="cuda"), 1)
        t = T.nn.functional.one_hot(T.randint(0, C, (B,), generator=gen, device="cuda"), C).float()
        p[1] = T.tensor([0.45, 0.1, 0.45])                # a tie: argmax 0
        t[1] = T.tensor([0.5, 0.0, 0.5])                  # ... in the targets too
        if B == 5:
            p[2, 1] = float("nan")                        # torch: NaN is the maximum
        row_loss = T.rand(B, generator=gen, device="cuda") * 3
        state.add(p, t, row_loss)
        pa, ta = T.argmax(p, 1), T.argmax(t, 1)
        assert int(pa[1]) == 0 and int(ta[1]) == 0 and (B != 5 or int(pa[2]) == 1)
        ref_correct += int((pa == ta).sum())
        ref_sum += float(np.float32(float(row_loss.double().sum()) / (B * C)))
        ref_n += B
    loss, acc, n, batches = state.read()
    assert n == ref_n == 69 and batches == 3 and acc == ref_correct / 69
    assert abs(loss * 3 - ref_sum) <= 3 * 2.0 ** -23 * ref_sum
    # behind the real forward: the same tree, the same bits
    g = golden("efficiency.npz")
    x, t, params = _fixture_case(T, g, 4)
    state, total, correct = efficiency.EvalState("cuda"), 0.0, 0
    for lo, hi in ((0, 32), (32, 700), (700, 1000)):
        l, _, probs, row_loss, _ = ops.det_head_forward(x[lo:hi], params, t[lo:hi])
        state.add(probs, t[lo:hi], row_loss)
        total += float(l)
        correct += int((probs.argmax(1) == t[lo:hi].argmax(1)).sum())
    assert float(state.loss_sum) == total and int(state.n) == 1000 and int(state.batches) == 3
    assert int(state.correct) == correct and 0 < correct < 1000


# ------------------------------------------------------------------------------------------------ pipeline
@pytest.fixture(scope="module")
def study(T):
    """whisper-tiny (seeded weights, DoRA on k_proj / v_proj) + the 96-signal / 160-noise synthetic dataset."""
    from gw_whisper_amd import efficiency, synth
    T.manual_seed(0)
    model = efficiency.build_model("tiny", seed=5).eval()
    sd = synth.head_state_dict([384, 512, 256, 128, 64, 2], seed=11)
    model.classifier.load_state_dict({k: T.from_numpy(v) for k, v in sd.items()})
    wave, noise = efficiency.synthetic_tensors(96, 160, seed=2)
    return model, T.from_numpy(wave).cuda(), T.from_numpy(noise).cuda()


def test_dataset_batch_is_assemble_then_logmel(T, gww, study):
    """The batch of a list of indices == ops.logmel(noise[noise_i] + snr * wave[wave_i]) (torch fp32) bit for bit, labels
    [1, 0] for injections and [0, 1] for pure noise; noises_per_signal = 2 and a clamped tail among the indices."""
    from gw_whisper_amd import efficiency, ops
    _, wave, noise = study
    ds = efficiency.ResampledDataset(wave[:40], noise, (5.0, 15.0), (30, 50), (100, 140), (120, 180), noises_per_signal=2, seed=9)
    assert len(ds) == 100
    idx = [0, 1, 39, 17, 40, 99, 25, 60]
    mel, targets, (noise_i, wave_i, snr, is_wave) = ds.batch(idx)
    assert wave_i.tolist() == [30, 30, 39, 38, -1, -1, 39, -1] and noise_i.tolist() == [100, 101, 139, 117, 120, 159, 125, 140]
    assert targets.tolist() == [[1.0, 0.0]] * 4 + [[0.0, 1.0]] * 2 + [[1.0, 0.0], [0.0, 1.0]]
    rows = []
    for n_i, w_i, s in zip(noise_i, wave_i, snr):
        rows.append(noise[n_i] + float(s) * wave[w_i] if w_i >= 0 else noise[n_i])
    assert mel.shape == (8, 80, 3000) and T.equal(mel, ops.logmel(T.stack(rows)))
    assert ((snr[is_wave] >= 5.0) & (snr[is_wave] <= 15.0)).all()


@pytest.mark.parametrize("softmax", [True, False], ids=["softmax", "logit-difference"])
def test_estimator_table_equals_numpy_statistics(T, gww, study, softmax):
    """The estimator's table == numpy's sort / index / compare on the scores the same model gives in a plain forward with
    another batch size (scores are per segment and per row, so the batching does not enter): plumbing, no tolerance.
    160 noise samples: the FAPs 0.1, 0.01, 0.001 give ranks 16, 1 and 0 -- the last one warns."""
    from gw_whisper_amd import efficiency, ops
    from gw_whisper_amd.models import _pooled
    base, wave, noise = study

    class Net(T.nn.Module):            # the same encoder and layers; remove_softmax then changes this wrapper only
        def __init__(self):
            super().__init__()
            self.encoder, self.classifier = base.encoder, T.nn.Sequential(*base.classifier.children())
    model = Net().eval()
    if not softmax:
        efficiency.remove_softmax(model)
    wave_ds = efficiency.ResampledDataset(wave, noise, (0., 0.), (0, 96), (0, 96), (0, 0))
    noise_ds = efficiency.ResampledDataset(wave, noise, (0., 0.), (0, 0), (0, 0), (0, 160))
    snrs, faps = [3.0, 8.0, 20.0], (0.1, 0.01, 0.001)
    est = efficiency.EfficiencyEstimator(wave_ds, noise_ds, snrs, batch_size=64, faps=faps)
    with pytest.warns(UserWarning, match="rank 0"):
        table = est(model)
    params = [p.detach() for p in efficiency._det_parameters(model.classifier)]
    zero_t = T.zeros(1, 2, device="cuda")

    def plain(x):
        out = []
        with T.no_grad():
            for i in range(0, len(x), 40):
                pooled = _pooled(model.encoder, ops.logmel(x[i:i + 40])).float()
                _, z, p, _, _ = ops.det_head_forward(pooled, params, zero_t.expand(len(pooled), 2).contiguous())
                out.append(p[:, 0] if softmax else z[:, 0] - z[:, 1])
        return T.cat(out).cpu().numpy()
    noise_scores = plain(noise)
    wave_scores = [plain(noise[:96] + float(np.float32(s)) * wave) for s in snrs]
    thr, ref = eh.numpy_statistics(noise_scores, wave_scores, faps)
    assert np.array_equal(est.thresholds.cpu().numpy(), thr) and thr[2] == noise_scores.min()
    assert table.shape == (3, 3) and np.array_equal(table, ref), (table, ref)
    assert (table[:, 2] >= table[:, 0]).all()      # the rank-0 threshold is the smallest noise score


def _dora_step(T, head):
    from gw_whisper_amd import efficiency, inference, ops, synth
    from gw_whisper_amd.models import _pooled
    T.manual_seed(0)                  # peft's lora_A initialisation draws from the global generator
    model = efficiency.build_model("micro", precision="fp32", seed=5)
    sd = synth.head_state_dict([128, 512, 256, 128, 64, 2], seed=9)
    model.classifier.load_state_dict({k: T.from_numpy(v) for k, v in sd.items()})
    with T.no_grad():
        gen = T.Generator().manual_seed(2)
        for n_, p_ in model.encoder.named_parameters():
            if "lora_B" in n_:
                p_.copy_(0.05 * T.randn(p_.shape, generator=gen))
    model.train()
    wave, noise = efficiency.synthetic_tensors(4, 8, seed=1)
    ds = efficiency.ResampledDataset(T.from_numpy(wave).cuda(), T.from_numpy(noise).cuda(), (5., 15.), (0, 4), (0, 4), (4, 8), seed=3)
    mel, targets, _ = ds.batch(np.arange(8))
    if head == "hip":
        loss, probs = efficiency.reg_bce_head(model.classifier, _pooled(model.encoder, mel), targets, 1e-6)
        assert probs.shape == (8, 2) and not probs.requires_grad
    else:
        loss = inference.RegBCELoss(epsilon=1e-6, dim=2)(model(mel).float(), targets)
    loss.backward()
    out = {n_: p_.grad.detach().clone() for n_, p_ in model.named_parameters() if p_.requires_grad}
    assert any("lora_A" in k for k in out) and any(k.startswith("classifier.") for k in out)
    return float(loss.detach()), out


def test_reg_bce_head_wiring_behind_a_peft_encoder(T, gww):
    """One DoRA step through reg_bce_head behind a get_peft_model-wrapped micro encoder of precision fp32: the loss and
    every adapter and head gradient agree with the same step through the torch head within the bounds
    tests/test_gpu_glitch.py::test_head_cross_entropy_wiring_behind_a_peft_encoder holds its own whole-step comparison to
    (1e-5 relative on the loss, 2e-4 relative Frobenius error on every gradient)."""
    l_hip, g_hip = _dora_step(T, "hip")
    l_t, g_t = _dora_step(T, "torch")
    assert set(g_hip) == set(g_t)
    worst = max((_rel(g_hip[k], g_t[k]), k) for k in g_t)
    print(f"wiring fp32: loss hip {l_hip:.7f} torch {l_t:.7f}; worst gradient {worst[1]} rel {worst[0]:.2e}")
    assert abs(l_hip - l_t) <= 1e-5 * abs(l_t)
    for k in g_t:
        assert _rel(g_hip[k], g_t[k]) <= 2e-4, (k, _rel(g_hip[k], g_t[k]))


# ------------------------------------------------------------------------------------------------ programs
def _run(cmd, timeout=600):
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    return r


@pytest.mark.parametrize("head", ["hip", "torch"])
def test_programs_end_to_end(T, gww, tmp_path, head):
    """run_efficiency_train.py --synthetic for 2 epochs with one curriculum step on the epoch scheduler, then
    run_efficiency_estimate.py on its artefacts, each in a fresh child process: file names, line formats, and that the
    scheduler stepped."""
    import re
    from gw_whisper_amd import efficiency
    out, sd = str(tmp_path / "outfiles"), str(tmp_path / "state_dicts")
    common = ["--synthetic", "32", "--seed", "1", "--outfiles-dir", out, "--state-dicts-dir", sd]
    r = _run([sys.executable, os.path.join(ROOT, "harness", "run_efficiency_train.py"), "3", *common, "--epochs", "2",
              "--batch-size", "16", "--snr-steps", "1", "--initial-snr-range", "20", "30", "--final-snr-range", "5", "15",
              "--cl-scheduler", "epoch", "--cl-patience", "0", "--head", head])
    lines = open(os.path.join(out, "out_train_0003.txt")).read().splitlines()
    assert len(lines) == 2
    for e, l in enumerate(lines, 1):
        assert re.fullmatch(r"%04i    \d\.\d{12}e[+-]\d\d    \d\.\d{12}e[+-]\d\d    [01]\.\d{6}" % e, l), l
    assert "# Reducing SNR range from 20.000000-30.000000 to 5.000000-15.000000" in r.stdout
    names = set(os.listdir(sd))
    want = {f"{p}_run_0003_epoch_{e:04d}{x}" for e in (1, 2) for p, x in
            (("state_dict", ".pt"), ("optim_state_dict", ".pt"), ("lora_weights", ".pt"), ("dense_layers", ".pth"))}
    want |= {"final_lora_weights_run_0003.pt", "final_dense_layers_run_0003.pth", "best_state_dict_0003.pt",
             "best_lora_weights_run_0003.pt", "best_dense_layers_run_0003.pth"}
    assert want <= names, sorted(want - names)
    assert os.path.isfile(os.path.join(sd, "lora_weights_run_0003_epoch_0002.pt", "adapter_model.safetensors"))
    assert list(T.load(os.path.join(sd, "dense_layers_run_0003_epoch_0002.pth"), map_location="cpu")) == list(eh.PARAM_KEYS)
    eff_dir = str(tmp_path / "efficiencies")
    _run([sys.executable, os.path.join(ROOT, "harness", "run_efficiency_estimate.py"), "3", *common, "--epochs-list", "1", "2",
          "--snrs", "5", "9", "30", "--faps", "0.1", "0.05", "--output-directory", eff_dir])
    for e in (1, 2):
        text = open(os.path.join(eff_dir, f"out_efficiencies_run_0003_epoch_{e:04d}.txt")).read()
        faps, snrs, table = efficiency.parse_efficiency_text(text)
        assert faps == [0.1, 0.05] and snrs == [5.0, 9.0, 30.0] and table.shape == (3, 2)
        assert efficiency.efficiency_text(faps, snrs, table) == text
        assert ((table >= 0) & (table <= 1)).all() and (table[:, 0] >= table[:, 1]).all()
