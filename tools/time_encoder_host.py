"""Host time of the encoder's change tracking in one benchmark step, on the CPU: no GPU and no library needed.

Setup: whisper-tiny with the benchmark's adapters (get_peft_model, DoRA r = 8 on q / k / v, requires_grad = "lora" in name).
One step is two forward entries (the input check, _wants_grad, _group_keys) and the optimizer post-step hook's share
(_has_trainable_adapters, _group_keys); the parameter cache is validated once per entry.  The input is a stand-in that
answers the input check like a [2, 80, 3000] GPU tensor.  Prints min / median / max of 9 x 1000 steps in microseconds.

Made for A/B runs of two checkouts, interleaved on one machine: a tree whose encoder has no ``_enter`` (the one before
the self-validating cache) is timed through the calls its forward made, ``_check_input``, ``_wants_grad``, ``_group_keys``."""

import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from gw_whisper_amd.encoder import WhisperConfig, WhisperEncoder  # noqa: E402
from gw_whisper_amd.peft import LoraConfig, get_peft_model  # noqa: E402


class Mel:
    is_cuda, requires_grad, shape, device = True, False, (2, 80, 3000), torch.device("cpu")

    def dim(self):
        return 3


def main():
    enc = WhisperEncoder(WhisperConfig.named("tiny"))
    targets = [f"layers.{i}.self_attn.{p}" for i in range(4) for p in ("q_proj", "k_proj", "v_proj")]
    peft = get_peft_model(enc, LoraConfig(use_dora=True, r=8, lora_alpha=32, target_modules=targets))
    for n, p in peft.named_parameters():
        p.requires_grad = "lora" in n
    x = Mel()
    if hasattr(enc, "_enter"):
        def step():
            for _ in range(2):
                c = enc._enter(x)
                enc._wants_grad(x, c)
                enc._group_keys(c)
            c = enc._param_cache()
            enc._has_trainable_adapters(c)
            enc._group_keys(c)
    else:
        def step():
            for _ in range(2):
                enc._check_input(x)
                enc._wants_grad(x)
                enc._group_keys()
            enc._has_trainable_adapters()
            enc._group_keys()
    assert enc._wants_grad(x)
    for _ in range(200):
        step()
    runs = []
    for _ in range(9):
        t0 = time.perf_counter()
        for _ in range(1000):
            step()
        runs.append((time.perf_counter() - t0) * 1e3)   # ms per 1000 steps = us per step
    print(f"host us per step: min {min(runs):.1f} median {statistics.median(runs):.1f} max {max(runs):.1f}")


if __name__ == "__main__":
    main()
