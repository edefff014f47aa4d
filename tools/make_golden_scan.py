#!/usr/bin/env python3
"""Records tests/golden/scan_events_default.npz: ``real_events.scan_events`` without ``frontend`` -- resample to 16 kHz +
Whisper's published log-mel -- on the seeded model and strain of tests/native_scan.py, in ragged batches of 4.  The committed
file was recorded at the commit BEFORE the native front end existed (section 33 of DESIGN.md); tests/test_gpu_native_scan.py
holds the default path to it element for element.  Needs an MI355X."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from gw_whisper_amd import real_events  # noqa: E402
from tests import native_scan as ns  # noqa: E402

if __name__ == "__main__":
    assert torch.cuda.is_available(), "make_golden_scan.py needs an MI355X"
    strain = ns.scan_strain()
    out = real_events.scan_events(ns.default_scan_model(torch, strain), strain, batch_size=ns.SCAN_BATCH)
    path = os.path.join(ROOT, "tests", "golden", "scan_events_default.npz")
    np.savez(path, model_output=out)
    print(f"wrote {path}: {out.shape}, {out.min():.6f} .. {out.max():.6f}")
