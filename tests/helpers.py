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
