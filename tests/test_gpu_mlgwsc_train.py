"""The MLGWSC-1 training program on the MI355X: the HIP kernels of csrc/contrastive.hip against the reference's own
definitions (tests/golden/mlgwsc_train.npz, tools/make_golden_mlgwsc.py) and fp64 torch, the pretraining step's wiring,
the pretrained-weights reload, and harness/run_mlgwsc_train.py end to end into harness/run_inference.py."""

import os
import re
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def T():
    import torch
    assert torch.cuda.is_available()
    return torch


def test_info_nce_kernels_match_the_fp64_reference(T, gww, golden):
    """ContrastivePretrainer._info_nce run in fp64 with autograd: the loss to 1e-5 relative, dz1 / dz2 to 1e-5 of their
    largest magnitude; tau = 0.01 (the fp32 reference's exp overflows there) stays finite; two calls, identical bits."""
    from gw_whisper_amd.mlgwsc_train import info_nce
    z = golden("mlgwsc_train.npz")
    for k in range(int(z["nce_cases"])):
        tau = float(z[f"nce{k}_tau"])
        z1 = T.from_numpy(z[f"nce{k}_z1"]).cuda().requires_grad_(True)
        z2 = T.from_numpy(z[f"nce{k}_z2"]).cuda().requires_grad_(True)
        runs = []
        for _ in range(2):
            loss = info_nce(z1, z2, tau)
            g1, g2 = T.autograd.grad(loss, (z1, z2))
            runs.append((loss.detach().cpu().numpy(), g1.cpu().numpy(), g2.cpu().numpy()))
        (loss, g1, g2), again = runs
        for a, b in zip(runs[0], again):
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), f"case {k}: two calls differ"
        ref = float(z[f"nce{k}_loss"])
        assert np.isfinite(loss) and np.isfinite(g1).all() and np.isfinite(g2).all(), k
        assert abs(float(loss) - ref) <= 1e-5 * abs(ref) + 1e-7, (k, float(loss), ref)
        r1, r2 = z[f"nce{k}_dz1"], z[f"nce{k}_dz2"]
        scale = max(np.abs(r1).max(), np.abs(r2).max())
        err = max(np.abs(g1 - r1).max(), np.abs(g2 - r2).max())
        print(f"InfoNCE case {k} {r1.shape} tau {tau}: loss {float(loss):.7g} vs {ref:.7g}, grad err {err:.2e} of {scale:.2e}")
        assert err <= 1e-5 * scale + 1e-9, (k, err, scale)
    assert not np.isfinite(z["nce4_loss_ref_fp32"])       # the case the max-subtracted LSE exists for


@pytest.mark.parametrize("B", [3, 32])
@pytest.mark.parametrize("Hin,Win", [(32, 32), (128, 128), (80, 3000), (33, 50)])
def test_adapter_tail_backward_kernel_matches_fp64(T, gww, B, Hin, Win):
    """gww_qadapter_tail_backward_f32 (qscan._AdapterTail.backward) against the reference's torch composition in fp64:
    d_y, d_scale, d_bias, d_gamma, d_beta within 1e-5 of each gradient's scale; two calls give identical bits."""
    from gw_whisper_amd.qscan import _AdapterTail
    T.manual_seed(B * 7 + Hin + Win)
    D, det = 2, 1
    y = T.randn(B, Hin, Win, device="cuda", requires_grad=True)
    scale = T.tensor([0.7], device="cuda", requires_grad=True)
    bias = T.tensor([-0.2], device="cuda", requires_grad=True)
    gamma = T.tensor([1.3, 0.8], device="cuda", requires_grad=True)
    beta = T.tensor([0.05, -0.1], device="cuda", requires_grad=True)
    w = T.randn(B, D, 80, 3000, device="cuda")
    leaves = [y, scale, bias, gamma, beta]
    got = []
    for _ in range(2):
        out = _AdapterTail.apply(y, scale, bias, gamma, beta, T.zeros(B, D, 80, 3000, device="cuda"), det)
        got.append([g.cpu() for g in T.autograd.grad((out * w).sum(), leaves)])
    for a, b in zip(*got):
        assert T.equal(a.view(T.int32), b.view(T.int32)), "two calls differ"
    l64 = [t.detach().double().requires_grad_(True) for t in leaves]
    p = T.nn.functional.adaptive_avg_pool2d(l64[0][:, None], (80, 3000))[:, 0]
    ref = (l64[1] * p + l64[2]) * l64[3][det] + l64[4][det]
    g_ref = T.autograd.grad((ref * w[:, det].double()).sum(), l64)
    for name, a, b in zip(("d_y", "d_scale", "d_bias", "d_gamma", "d_beta"), got[0], g_ref):
        b = b.cpu()
        sc = b.abs().max().item()
        err = (a.double() - b).abs().max().item()
        assert err <= 1e-5 * sc, (name, err, sc)
    assert got[0][3][0].item() == 0.0 and got[0][4][0].item() == 0.0      # the other detector's FiLM gets nothing


def test_batch_assembly_kernel_is_bit_identical_to_the_reference(T, gww, golden):
    """gww_assemble_batch_f32 on plans drawn as the reference draws them: PretrainDataset's two views in ONE launch and
    BinaryGWDataset's items, bit for bit the reference's torch `noise + snr * waveform`."""
    from gw_whisper_amd.mlgwsc_train import BinaryGWDataset, ConcatGWData, PretrainDataset
    z = golden("mlgwsc_train.npz")
    ds = PretrainDataset(T.from_numpy(z["pre_noises"]), T.from_numpy(z["pre_waves"]), snr_range=(5.0, 15.0),
                         noise_only_prob=float(z["pre_prob"]), device="cuda")
    x1, x2 = ds.batch(z["pre_idx"], np.random.default_rng(int(z["pre_seed"])))
    assert np.array_equal(x1.cpu().numpy().view(np.uint32), z["pre_x1"].view(np.uint32))
    assert np.array_equal(x2.cpu().numpy().view(np.uint32), z["pre_x2"].view(np.uint32))
    data = ConcatGWData([BinaryGWDataset(z["bin_noises"], z["bin_waves"])], "cuda")
    x, lab = data.batch(z["bin_idx"], np.random.default_rng(int(z["bin_seed"])))
    assert np.array_equal(x.cpu().numpy().view(np.uint32), z["bin_x"].view(np.uint32))
    assert np.array_equal(lab.cpu().numpy(), z["bin_labels"])


def _pretrainer(T, seed=0, lr=1e-4):
    from gw_whisper_amd import synth
    from gw_whisper_amd.encoder import WhisperConfig, WhisperEncoder
    from gw_whisper_amd.mlgwsc_train import ContrastivePretrainer, apply_lora
    from gw_whisper_amd.qscan import QTransformAdapter
    T.manual_seed(seed)
    enc = WhisperEncoder.from_numpy_state_dict(synth.named_encoder_state_dict("micro", seed=seed), WhisperConfig.named("micro"),
                                               precision="bf16")
    enc = apply_lora(enc, r=8, alpha=32, use_dora=True).cuda()
    with T.no_grad():
        for n, p in enc.named_parameters():
            if "lora_B" in n:                             # away from the zero initialisation: every path carries gradient
                p.normal_(0.0, 0.02)
    ad = QTransformAdapter.train_variant(n_detectors=2).cuda()
    return ContrastivePretrainer(ad, enc, 2, device="cuda", lr=lr, temperature=0.1)


def _views(T, B, seed):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((2, B, 2, 2048)).astype(np.float32)
    x[1] += 0.5 * x[0]
    return T.from_numpy(x[0]).cuda(), T.from_numpy(x[1]).cuda()


def test_pretraining_step_gradients_match_a_torch_info_nce(T, gww):
    """One pretraining step's gradients on the adapter, the DoRA parameters and the projection with the HIP InfoNCE
    against the same step with the loss restated in torch fp32 (MLGWSC-1/train.py:410-424): the same forward, the loss
    gradient dz within 1e-4 relative, every parameter group within the bound its conditioning allows (below)."""
    F = T.nn.functional
    pt = _pretrainer(T)
    X1, X2 = _views(T, 4, 3)

    def torch_info_nce(z1, z2, temp=0.1):
        z1, z2 = F.normalize(z1, dim=1), F.normalize(z2, dim=1)
        B = z1.size(0)
        zz = T.cat([z1, z2], dim=0)
        sim = (zz @ zz.T) / temp
        mask = ~T.eye(2 * B, device=zz.device, dtype=T.bool)
        exp_sim = T.exp(sim) * mask
        pos = T.exp((z1 * z2).sum(dim=1) / temp)
        return (-T.log(pos / exp_sim[:B].sum(dim=1)) - T.log(pos / exp_sim[B:].sum(dim=1))).mean()

    # a fresh adapter and encoder map every window to nearly the same embedding; centre and scale the projection's first
    # layer on this batch's embeddings so that the projections differ (the comparison below stays ill-conditioned anyway)
    with T.no_grad():
        e1, e2 = pt._embed(X1, X2)
        mean = T.cat([e1, e2]).mean(0)
        pt.proj[0].bias.copy_(-(pt.proj[0].weight @ mean))
        pt.proj[0].weight.mul_(1.0 / max(1e-6, (T.cat([e1, e2]) - mean).std().item()))
    params = [(n, p) for n, p in list(pt.q_adapter.named_parameters()) + list(pt.encoder.named_parameters())
              + [("proj." + n, p) for n, p in pt.proj.named_parameters()] if p.requires_grad]
    grads, losses, embeds, dzs = [], [], [], []
    for fn in (pt._info_nce, torch_info_nce):
        for _, p in params:
            p.grad = None
        e1, e2 = pt._embed(X1, X2)
        z1, z2 = pt.proj(e1), pt.proj(e2)
        z1.retain_grad(), z2.retain_grad()
        loss = fn(z1, z2)
        loss.backward()
        losses.append(loss.item())
        embeds.append(T.cat([e1, e2]).detach())
        dzs.append(T.cat([z1.grad, z2.grad]))
        grads.append([p.grad.detach().clone() for _, p in params])
    assert T.equal(*embeds)                               # the same forward both times: only the loss differs
    dz_rel = ((dzs[0] - dzs[1]).norm() / dzs[1].norm()).item()
    assert abs(losses[0] - losses[1]) <= 1e-5 * abs(losses[1])
    assert any("lora" in n for n, _ in params) and any(n.startswith("freq_adapter") for n, _ in params)
    # Where the loss meets the model the two agree to 1e-4 (measured 6e-6).  The parameter gradients are compared per
    # group, ||a - b|| / ||b||, within 0.1: this batch's projections are nearly parallel and InfoNCE's dz nearly sums to
    # zero over the batch, so the projection's gradients (sums of dz over rows) are small residues that amplify the 6e-6
    # about 100-fold (measured 6e-4), and the bf16 encoder backward spreads it further into the DoRA and adapter groups
    # (3e-2 and 3e-3).  A wiring fault -- a missing, doubled or mis-signed path -- shows as O(1).
    assert dz_rel <= 1e-4, dz_rel
    groups = {}
    for (n, _), a, b in zip(params, *grads):
        assert T.isfinite(a).all() and b.norm() > 0, n
        key = "proj" if n.startswith("proj.") else ("lora" if "lora" in n else "adapter")
        da, nb = groups.get(key, (0.0, 0.0))
        groups[key] = (da + (a - b).double().norm().item() ** 2, nb + b.double().norm().item() ** 2)
    assert set(groups) == {"adapter", "lora", "proj"}
    rel = {key: (da / nb) ** 0.5 for key, (da, nb) in groups.items()}
    print(f"pretraining step: dz relative difference {dz_rel:.2e}; gradients per group:", {k: f"{v:.2e}" for k, v in rel.items()})
    assert all(v <= 0.1 for v in rel.values()), rel


def test_pretrained_weights_reload_bit_for_bit(T, gww, tmp_path):
    """q_adapter_pretrained.pt / encoder_pretrained.pt (MLGWSC-1/train.py:912-920) saved after a pretraining step and
    loaded into a fresh model -- one that already ran a forward, so its packed weights must follow the reload -- give the
    pretrained model's adapter maps and last tokens bit for bit."""
    pt = _pretrainer(T, seed=0, lr=1e-3)
    X1, X2 = _views(T, 2, 5)
    pt.step(X1, X2)
    T.save(pt.q_adapter.state_dict(), tmp_path / "q_adapter_pretrained.pt")
    T.save(pt.encoder.state_dict(), tmp_path / "encoder_pretrained.pt")
    fresh = _pretrainer(T, seed=9)
    with T.no_grad():
        f0 = fresh.q_adapter(X1)
        fresh.encoder.last_token(f0.reshape(-1, *f0.shape[2:]))
    fresh.q_adapter.load_state_dict(T.load(tmp_path / "q_adapter_pretrained.pt", map_location="cuda"))
    fresh.encoder.load_state_dict(T.load(tmp_path / "encoder_pretrained.pt", map_location="cuda"))
    with T.no_grad():
        fa, fb = pt.q_adapter(X1), fresh.q_adapter(X1)
        assert T.equal(fa, fb)
        flat = fa.reshape(-1, *fa.shape[2:])
        ta, tb = pt.encoder.last_token(flat), fresh.encoder.last_token(flat)
    assert T.equal(ta, tb)


def _run(cmd, timeout):
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    return r


def test_harness_end_to_end_resume_and_search(T, gww, tmp_path):
    """harness/run_mlgwsc_train.py: InfoNCE pretraining + two supervised epochs on synthetic data with the reduced encoder,
    every artefact under its reference name; --resume continues at epoch 3 with the optimizer state restored; the trained
    components drive harness/run_inference.py (train -> search)."""
    from gw_whisper_amd import synth
    wfile = str(tmp_path / "micro_encoder.pth")
    T.save({k: T.from_numpy(v) for k, v in synth.named_encoder_state_dict("micro", seed=4).items()}, wfile)
    out = str(tmp_path / "run")
    base = [sys.executable, os.path.join(ROOT, "harness", "run_mlgwsc_train.py"), "-d", str(tmp_path), "-o", out,
            "--synthetic", "32", "--encoder", "micro", "--encoder-weights", wfile, "--batch-size", "4", "--use-dora",
            "--learning-rate", "1e-4"]
    _run(base + ["--pretrain-steps", "2", "--epochs", "2"], 900)
    for name in ("losses.txt", "last.pt", "state_dict_e_0001.pt", "state_dict_e_0002.pt", "best_state_dict.pt",
                 "best_adapter.pt", "best_dense_layers.pth", "best_lora_weights/adapter_config.json",
                 "best_lora_weights/adapter_model.safetensors", "q_adapter_pretrained.pt", "encoder_pretrained.pt"):
        assert os.path.exists(os.path.join(out, name)), name
    line = re.compile(r"^\d{4}\t-?\d+\.\d{6}\t-?\d+\.\d{6}$")
    lines = open(os.path.join(out, "losses.txt")).read().splitlines()
    assert len(lines) == 2 and all(line.match(l) for l in lines) and lines[0].startswith("0001"), lines
    last = T.load(os.path.join(out, "last.pt"), map_location="cpu")
    assert last["epoch"] == 2
    steps = max(int(s["step"]) for s in last["optimizer_state"]["state"].values())
    assert steps == 2 * 8                                 # 32 items in batches of 4, two epochs
    # resume 'latest': epoch 3, Adam's step count carries on from last.pt
    _run(base + ["--pretrain-steps", "0", "--epochs", "3", "--resume", "--force"], 900)
    lines = open(os.path.join(out, "losses.txt")).read().splitlines()
    assert len(lines) == 3 and lines[2].startswith("0003\t") and line.match(lines[2]), lines
    last = T.load(os.path.join(out, "last.pt"), map_location="cpu")
    assert last["epoch"] == 3
    assert max(int(s["step"]) for s in last["optimizer_state"]["state"].values()) == 3 * 8
    # train -> search: the components are what run_inference.py reads
    res = str(tmp_path / "search.npz")
    _run([sys.executable, os.path.join(ROOT, "harness", "run_inference.py"), "unused.hdf", res, "--synthetic", "3", "--white",
          "--encoder", "micro", "--encoder-weights", wfile, "--adapter-weights", os.path.join(out, "best_adapter.pt"),
          "--lora-weights", os.path.join(out, "best_lora_weights"), "--dense-weights",
          os.path.join(out, "best_dense_layers.pth")], 900)
    r = np.load(res)
    assert len(r["all_vals"]) > 0 and np.isfinite(r["all_vals"]).all()
