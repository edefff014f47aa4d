"""Small deterministic pieces shared by tools/make_golden.py (which runs the reference's code on them) and the tests
(which run this build's code on the same things)."""
import torch


def search_toy_network():
    """Stand-in network of the search loop: [B, 2, 2048] -> softmax over 2 classes (CPU / any device), fp32 out.
    The 4096-long dot products and the softmax run in fp64 and only the result is rounded to fp32: an fp32 GEMM's
    summation order depends on the machine's BLAS kernels, and the scores are compared with a stored fixture bit for bit."""
    g = torch.Generator().manual_seed(1234)
    w = (torch.randn(2 * 2048, 2, generator=g) * 0.05).double()

    class Net(torch.nn.Module):
        def forward(self, x):
            z = x.reshape(x.shape[0], -1).double() @ w.to(x.device)
            return torch.softmax(z, dim=1).float()
    return Net()


# ---------------------------------------------------------------- float64 restatement of the HF encoder
def encoder64(T, p, mel, cfg):
    """HF:models/whisper/modeling_whisper.py WhisperEncoder.forward in float64 (eval: no dropout).  ``T`` is the torch
    module, ``p`` the state dict as float64 tensors, ``cfg`` = (d, layers, heads)."""
    F_ = T.nn.functional
    d, L, H = cfg
    x = F_.gelu(F_.conv1d(mel, p["conv1.weight"], p["conv1.bias"], padding=1))
    x = F_.gelu(F_.conv1d(x, p["conv2.weight"], p["conv2.bias"], stride=2, padding=1))
    x = x.permute(0, 2, 1) + p["embed_positions.weight"]
    B, Tn, _ = x.shape
    for i in range(L):
        q_ = lambda n: p[f"layers.{i}.{n}"]
        h = F_.layer_norm(x, (d,), q_("self_attn_layer_norm.weight"), q_("self_attn_layer_norm.bias"), 1e-5)
        q = (h @ q_("self_attn.q_proj.weight").t() + q_("self_attn.q_proj.bias")) * (d // H) ** -0.5
        k = h @ q_("self_attn.k_proj.weight").t()
        v = h @ q_("self_attn.v_proj.weight").t() + q_("self_attn.v_proj.bias")
        sh = lambda t: t.view(B, Tn, H, d // H).transpose(1, 2)
        a = T.softmax(sh(q) @ sh(k).transpose(-1, -2), dim=-1) @ sh(v)
        a = a.transpose(1, 2).reshape(B, Tn, d)
        x = x + a @ q_("self_attn.out_proj.weight").t() + q_("self_attn.out_proj.bias")
        h = F_.layer_norm(x, (d,), q_("final_layer_norm.weight"), q_("final_layer_norm.bias"), 1e-5)
        h = F_.gelu(h @ q_("fc1.weight").t() + q_("fc1.bias"))
        x = x + h @ q_("fc2.weight").t() + q_("fc2.bias")
    return F_.layer_norm(x, (d,), p["layer_norm.weight"], p["layer_norm.bias"], 1e-5)


def dora64(T, sd, theta, mel, cfg, scaling):
    """fp64 forward with DoRA-merged targets (peft: the weight norm enters detached); ``theta`` maps a target's module
    name to its float64 (A, B, m) tensors."""
    p = {k: T.from_numpy(v).double() for k, v in sd.items()}
    for name, (A, Bm, m) in theta.items():
        W0 = p[name + ".weight"]
        Wp = W0 + scaling * (Bm @ A)
        p[name + ".weight"] = (m / T.linalg.norm(Wp, dim=1).detach())[:, None] * Wp
    return encoder64(T, p, mel, cfg)
