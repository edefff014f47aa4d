"""What the constant-tail shortcut of the inference stem (csrc/stem_tail.hip) rests on, checked on the CPU oracle: the log-mel
of a short segment zero-padded to 30 s is ONE value per (segment, mel bin) behind its live frames, bit for bit."""

import numpy as np
import pytest

from gw_whisper_amd import synth
from oracle import logmel as olm

TC = 256   # csrc/common.h: kStemTc; the device test covers frames [TC - 6, 3000)


def _tail_is_constant(mel, t0):
    bits = np.ascontiguousarray(mel[:, :, t0:]).view(np.uint32)
    return bool((bits == bits[:, :, :1]).all())


@pytest.mark.parametrize("seconds,live", [(1.0, 102), (1.5, 152)])
def test_padded_logmel_tail_is_bitwise_constant(seconds, live):
    """live = ceil((n + 200) / 160) frames see a sample (csrc/logmel.hip); every later frame holds the segment's floor."""
    n = int(16000 * seconds)
    assert live == -(-(n + 200) // 160) and live <= TC - 6
    mel = olm.log_mel(synth.strain_segments(4, seed=1000, n_samples=n))
    assert _tail_is_constant(mel, live)
    assert not _tail_is_constant(mel, live - 2)
    assert _tail_is_constant(mel, TC - 6)


def test_three_seconds_do_not_qualify():
    mel = olm.log_mel(synth.strain_segments(2, seed=1000, n_samples=48000))
    assert not _tail_is_constant(mel, TC - 6)
