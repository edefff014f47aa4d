"""The CNN decoder head in HIP (csrc/cnn_head.hip, ``ops.cnn_head_forward`` / ``ops.cnn_head_backward``,
``models.TwoChannelLIGOBinaryClassifierCNN``) against an fp64 ``torch.nn.functional.conv1d`` chain composed here.

The yardstick of every comparison is the error torch's own fp32 CPU evaluation of the same chain has against fp64
(``e_ref``, per tensor): the device result must lie within 8 x e_ref of fp64.  Both are fp32 chains of at most 385 terms in
different association orders, i.e. random walks of the same length; 8 covers the spread of a maximum over up to 1e5
elements, while a wrong tap, halo, bias or channel is an error of the order of the activations.  Needs an MI355X."""

import pytest

from gw_whisper_amd import synth
from oracle import logmel as olm

pytestmark = pytest.mark.gpu

FACTOR = 8.0
SHAPES = [(3, 128, 1), (2, 384, 3)]


@pytest.fixture(scope="module")
def T():
    import torch
    assert torch.cuda.is_available()
    return torch


def make_chain(T, C, seed=0):
    """The reference layout with torch's default init, seeded."""
    nn = T.nn
    T.manual_seed(seed)
    return nn.Sequential(nn.Conv1d(2, 64, 3, padding=1), nn.ReLU(), nn.Conv1d(64, 128, 3, padding=1), nn.ReLU(),
                         nn.Conv1d(128, 256, 3, padding=1), nn.ReLU(), nn.AdaptiveAvgPool1d(1), nn.Flatten(),
                         nn.Linear(256, C))


def chain_params(seq):
    return [t.detach() for i in (0, 2, 4, 8) for t in (seq[i].weight, seq[i].bias)]


def make_input(T, B, d, seed=0):
    """Standard normal with one position scaled x 20: pooled tokens are post-LayerNorm rows with outliers."""
    g = T.Generator().manual_seed(1000 + seed)
    x = T.randn(B, 2, d, generator=g)
    x[:, :, d // 3] *= 20.0
    return x


def chain_eval(T, params, x, dtype, masks=None):
    """(logits, [h1, h2, h3], [z1, z2, z3]) of the chain on the CPU in ``dtype``.  masks: the ReLU is replaced by a
    multiplication with these 0 / 1 tensors (the backward yardstick: ReLU's gradient for exactly those masks)."""
    F = T.nn.functional
    p = [t.to(dtype) for t in params]
    h, hs, zs = x.to(dtype), [], []
    for l in range(3):
        z = F.conv1d(h, p[2 * l], p[2 * l + 1], padding=1)
        h = z * masks[l].to(dtype) if masks is not None else T.relu(z)
        zs.append(z)
        hs.append(h)
    logits = F.linear(h.mean(dim=2), p[6], p[7])
    return logits, hs, zs


def split_saved(acts):
    return [acts[:, 0:64], acts[:, 64:192], acts[:, 192:448]]


def device_forward(T, params, x, train=True):
    from gw_whisper_amd import ops
    dev = [t.cuda() for t in params]
    if not train:
        return ops.cnn_head_forward(x.cuda(), dev)
    return ops.cnn_head_forward(x.cuda(), dev, train=True)


def check_forward(T, params, x, label):
    """Device logits + saved activations within FACTOR x e_ref of fp64, the ReLU masks equal up to the rounding band.
    Returns (logits, saved, e_ref per tensor)."""
    logits, saved = device_forward(T, params, x)
    r64 = chain_eval(T, params, x, T.float64)
    r32 = chain_eval(T, params, x, T.float32)
    got = [logits.cpu()] + [h.cpu() for h in split_saved(saved[2])]
    want64 = [r64[0]] + r64[1]
    want32 = [r32[0]] + r32[1]
    names = ["logits", "h1", "h2", "h3"]
    e_refs = []
    for n, g, w64, w32 in zip(names, got, want64, want32):
        e_ref = float((w32.double() - w64).abs().max())
        err = float((g.double() - w64).abs().max())
        e_refs.append(e_ref)
        print(f"[{label}] {n}: max|device - fp64| = {err:.3e}, e_ref = {e_ref:.3e}, ratio {err / max(e_ref, 1e-300):.2f}")
    for n, g, w64, e_ref in zip(names, got, want64, e_refs):
        err = float((g.double() - w64).abs().max())
        assert err <= FACTOR * e_ref, f"[{label}] {n}: {err:.3e} > {FACTOR} x {e_ref:.3e}"
    for l in range(3):
        z64 = r64[2][l]
        diff = (got[1 + l] > 0) != (z64 > 0)
        n_diff = int(diff.sum())
        outside = int((diff & (z64.abs() > FACTOR * e_refs[1 + l])).sum())
        print(f"[{label}] layer {l + 1}: {n_diff} of {diff.numel()} ReLU units differ from fp64, {outside} outside the band")
        assert outside == 0 and n_diff <= 4
    return logits, saved, dict(zip(names, e_refs))


def check_backward(T, params, x, saved, dlogits, label):
    """dx and the eight gradients within FACTOR x (torch fp32 autograd vs fp64 autograd), both through the chain with the
    DEVICE's masks."""
    from gw_whisper_amd import ops
    dx, grads = ops.cnn_head_backward(saved, dlogits.cuda())
    masks = [(h > 0).cpu() for h in split_saved(saved[2])]

    def autograd(dtype):
        leaves = [x.to(dtype).requires_grad_(True)] + [t.to(dtype).requires_grad_(True) for t in params]
        logits, _, _ = chain_eval(T, leaves[1:], leaves[0], dtype, masks)
        return T.autograd.grad((logits * dlogits.to(dtype)).sum(), leaves)
    g64, g32 = autograd(T.float64), autograd(T.float32)
    names = ["dx", "dw1", "db1", "dw2", "db2", "dw3", "db3", "dw4", "db4"]
    got = [dx.cpu()] + [g.cpu() for g in grads]
    bad = []
    for n, g, w64, w32 in zip(names, got, g64, g32):
        assert g.shape == w64.shape
        e_ref = float((w32.double() - w64).abs().max())
        err = float((g.double() - w64).abs().max())
        print(f"[{label}] {n}: max|device - fp64| = {err:.3e}, e_ref = {e_ref:.3e}, ratio {err / max(e_ref, 1e-300):.2f}, "
              f"max|fp64| = {float(w64.abs().max()):.3e}")
        if not err <= FACTOR * e_ref:
            bad.append(f"{n}: {err:.3e} > {FACTOR} x {e_ref:.3e}")
    assert not bad, f"[{label}] " + "; ".join(bad)
    return dx, grads


@pytest.fixture(scope="module")
def cases(T):
    """(params, x, dlogits) per shape, computed once and never modified."""
    out = {}
    for B, d, C in SHAPES + [(1, 1280, 1)]:
        seq = make_chain(T, C, seed=0)
        g = T.Generator().manual_seed(7 + d)
        out[(B, d, C)] = (chain_params(seq), make_input(T, B, d), T.randn(B, C, generator=g))
    return out


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "B%d-d%d-C%d" % s)
def test_forward_and_backward_against_fp64(T, gww, cases, shape):
    params, x, dlogits = cases[shape]
    _, saved, _ = check_forward(T, params, x, "B%d d%d C%d" % shape)
    check_backward(T, params, x, saved, dlogits, "B%d d%d C%d" % shape)


def test_forward_longest_walk(T, gww, cases):
    params, x, _ = cases[(1, 1280, 1)]
    check_forward(T, params, x, "B1 d1280 C1")


def test_edges_impulses_at_the_ends_and_at_every_tile_seam(T, gww, cases):
    """One impulse per sample: at 0, at d - 1 and at the two positions either side of every 64-position tile seam."""
    params, _, _ = cases[(2, 384, 3)]
    d = 384
    pos = [0, d - 1] + [p for s in range(64, d, 64) for p in (s - 1, s)]
    x = T.zeros(len(pos), 2, d)
    for i, p in enumerate(pos):
        x[i, i % 2, p] = 3.0
    _, saved, _ = check_forward(T, params, x, "impulses")
    g = T.Generator().manual_seed(11)
    check_backward(T, params, x, saved, T.randn(len(pos), 3, generator=g), "impulses")


def test_zero_sample_between_two_others_gives_the_bias_chain(T, gww, cases):
    """Nothing leaks across a sample boundary: an all-zero sample between two non-zero ones has the logits of the
    all-bias chain -- within the fp64 bound, and bit for bit those of the zero sample alone."""
    params, x2, _ = cases[(2, 384, 3)]
    x = T.zeros(3, 2, 384)
    x[0], x[2] = x2[0], x2[1]
    logits, _, e_refs = check_forward(T, params, x, "zero sample")
    alone = device_forward(T, params, x[1:2], train=False)
    assert T.equal(logits[1:2], alone)
    bias64 = chain_eval(T, params, T.zeros(1, 2, 384), T.float64)[0]
    err = float((logits[1:2].cpu().double() - bias64).abs().max())
    print(f"[zero sample] max|device - all-bias fp64| = {err:.3e}, e_ref (logits of the batch) = {e_refs['logits']:.3e}")
    assert err <= FACTOR * e_refs["logits"]


def test_reproducible_and_independent_of_the_batch(T, gww, cases):
    """Two calls give identical bits (forward and backward); a sample has bitwise the logits and dx it has alone, at index 0
    and at index 4 of a batch of 5; training-mode and inference-mode logits are bitwise equal."""
    from gw_whisper_amd import ops
    params, _, _ = cases[(2, 384, 3)]
    dev = [t.cuda() for t in params]
    x = make_input(T, 5, 384, seed=3).cuda()
    g = T.Generator().manual_seed(5)
    dl = T.randn(5, 3, generator=g).cuda()

    def step(xx, dd):
        logits, saved = ops.cnn_head_forward(xx, dev, train=True)
        dx, grads = ops.cnn_head_backward(saved, dd)
        return logits, saved[2], dx, grads
    a, b = step(x, dl), step(x, dl)
    assert T.equal(a[0], b[0]) and T.equal(a[1], b[1]) and T.equal(a[2], b[2])
    for ga, gb in zip(a[3], b[3]):
        assert T.equal(ga, gb)
    assert T.equal(ops.cnn_head_forward(x, dev), a[0])
    for i in range(5):
        one = step(x[i:i + 1].contiguous(), dl[i:i + 1].contiguous())
        assert T.equal(one[0], a[0][i:i + 1]) and T.equal(one[2], a[2][i:i + 1]), f"sample {i} alone differs from the batch"
    perm = T.tensor([4, 1, 2, 3, 0], device="cuda")
    p = step(x[perm].contiguous(), dl[perm].contiguous())
    assert T.equal(p[0][0], a[0][4]) and T.equal(p[0][4], a[0][0])
    assert T.equal(p[2][0], a[2][4]) and T.equal(p[2][4], a[2][0])


def test_wrong_shapes_raise(T, gww, cases):
    from gw_whisper_amd import GwwError, ops
    params, x, _ = cases[(3, 128, 1)]
    dev = [t.cuda() for t in params]
    with pytest.raises(GwwError, match="d=192"):
        ops.cnn_head_forward(T.zeros(1, 2, 192, device="cuda"), dev)
    with pytest.raises(GwwError, match=r"\[B, 2, d\]"):
        ops.cnn_head_forward(T.zeros(1, 3, 128, device="cuda"), dev)
    with pytest.raises(GwwError, match="parameter of shape"):
        ops.cnn_head_forward(x.cuda(), dev[:2] + [dev[2][:, :32].contiguous()] + dev[3:])
    _, saved = ops.cnn_head_forward(x.cuda(), dev, train=True)
    with pytest.raises(GwwError, match="dlogits"):
        ops.cnn_head_backward(saved, T.zeros(3, 2, device="cuda"))


# ------------------------------------------------------------------------------------------------- the module
def _micro_peft(T):
    from gw_whisper_amd.encoder import WhisperConfig, WhisperEncoder
    from gw_whisper_amd.peft import LoraConfig, get_peft_model
    d, L, H, F = synth.ENCODER_SIZES["micro"]
    sd = synth.encoder_state_dict(d, L, H, F, seed=3)
    enc = WhisperEncoder.from_numpy_state_dict(sd, WhisperConfig(d, L, H, F), precision="fp32")
    targets = [f"layers.{i}.self_attn.{p}" for i in range(L) for p in ("q_proj", "v_proj")]
    peft = get_peft_model(enc, LoraConfig(use_dora=True, r=8, lora_alpha=32, target_modules=targets)).cuda()
    g = T.Generator(device="cuda").manual_seed(2)
    with T.no_grad():
        for n, p in peft.named_parameters():
            p.requires_grad = "lora" in n
            if "lora_B" in n:
                p.copy_(0.02 * T.randn(p.shape, generator=g, device="cuda"))
    return peft


def test_module_hip_head_against_torch_head(T, gww):
    """TwoChannelLIGOBinaryClassifierCNN over a micro encoder: head="hip" against head="torch" on the same encoder and
    classifier weights -- logits within the forward bound, every classifier gradient within the backward bound, the
    adapter gradients within 1e-4 of each gradient's max (the project's figure for adapter gradients)."""
    from gw_whisper_amd import models, ops
    peft = _micro_peft(T)
    C = 3
    hip = models.TwoChannelLIGOBinaryClassifierCNN(peft, num_classes=C, head="hip").cuda()
    tor = models.TwoChannelLIGOBinaryClassifierCNN(peft, num_classes=C, head="torch").cuda()
    seq = make_chain(T, C, seed=4)
    hip.classifier.load_state_dict(seq.state_dict())
    tor.classifier.load_state_dict(seq.state_dict())
    params = chain_params(seq)
    mel = T.from_numpy(olm.log_mel(synth.strain_segments(4, seed=33))).cuda()
    m0, m1 = mel[:2], mel[2:]
    g = T.Generator().manual_seed(9)
    w = T.randn(2, C, generator=g)
    adapters = [(n, p) for n, p in peft.named_parameters() if p.requires_grad]
    assert len(adapters) == 3 * 4

    def run(model):
        for p in model.parameters():
            p.grad = None
        logits = model(m0, m1)
        (logits * w.cuda()).sum().backward()
        return (logits.detach().cpu(), [getattr(model.classifier[i], k).grad.cpu() for i in (0, 2, 4, 8) for k in ("weight", "bias")],
                [p.grad.detach().cpu().clone() for _, p in adapters])
    lh, ch, ah = run(hip)
    lt, ct, at = run(tor)
    with T.no_grad():
        both = models._pooled(peft, T.cat((m0, m1), dim=0))
        x = T.stack((both[:2], both[2:]), dim=1).float().cpu()
        assert T.equal(hip(m0, m1).cpu(), lh)                                  # the inference launch: same bits
    l64 = chain_eval(T, params, x, T.float64)[0]
    l32 = chain_eval(T, params, x, T.float32)[0]
    e_ref = float((l32.double() - l64).abs().max())
    err, dif = float((lh.double() - l64).abs().max()), float((lh - lt).abs().max())
    print(f"[module] logits: max|hip - fp64| = {err:.3e}, max|hip - torch| = {dif:.3e}, e_ref = {e_ref:.3e}")
    assert err <= FACTOR * e_ref and dif <= FACTOR * e_ref
    # classifier gradients: the fp64 masked chain on the pooled tokens, with the device's masks
    _, saved = ops.cnn_head_forward(x.cuda(), [t.cuda() for t in params], train=True)
    masks = [(h > 0).cpu() for h in split_saved(saved[2])]

    def autograd(dtype):
        leaves = [t.to(dtype).requires_grad_(True) for t in params]
        logits, _, _ = chain_eval(T, leaves, x, dtype, masks)
        return T.autograd.grad((logits * w.to(dtype)).sum(), leaves)
    g64, g32 = autograd(T.float64), autograd(T.float32)
    for i, (gh, w64, w32) in enumerate(zip(ch, g64, g32)):
        e_ref = float((w32.double() - w64).abs().max())
        err = float((gh.double() - w64).abs().max())
        print(f"[module] classifier gradient {i}: max|hip - fp64| = {err:.3e}, e_ref = {e_ref:.3e}")
        assert err <= FACTOR * e_ref
    for (n, _), gh, gt in zip(adapters, ah, at):
        rel = float((gh - gt).abs().max()) / float(gt.abs().max())
        print(f"[module] {n}: max|hip - torch| / max|torch| = {rel:.3e}")
        assert float(gt.abs().max()) > 0 and rel <= 1e-4


def test_run_train_with_the_cnn_head(T, gww, tmp_path):
    """harness/run_train.py --head cnn: one epoch on synthetic chirps with the reduced encoder; the best_dense_layers artefact
    is the CNN's classifier.state_dict() and loads into the reference layout."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = str(tmp_path)
    cmd = [sys.executable, os.path.join(root, "harness", "run_train.py"), "--synthetic", "32", "--encoder", "micro",
           "--batch-size", "8", "--num-epochs", "1", "--learning-rate", "1e-3", "--head", "cnn", "--models-path", out + "/models",
           "--log-dir", out + "/logs"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    recs = [json.loads(l) for l in open(out + "/logs/train_log.jsonl")]
    assert len(recs) == 1 and all(x["train_loss"] == x["train_loss"] and x["val_loss"] == x["val_loss"] for x in recs)
    for prefix in ("best_", ""):
        sd = T.load(out + f"/models/{prefix}dense_layers_8_32.pth", map_location="cpu")
        make_chain(T, 1).load_state_dict(sd)                       # strict: the reference's keys and shapes
        assert os.path.exists(out + f"/models/{prefix}lora_weights_8_32/adapter_model.safetensors")
