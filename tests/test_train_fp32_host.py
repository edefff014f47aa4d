"""CPU-side checks of the exact-fp32 training step's C entries: exported and bound, and bad arguments (NULL handles and
pointers, ranks outside 1..64) rejected before any HIP call; the target checks it shares with the bf16 backward entries
(ranks, NULL pointers, duplicates); the harness flag."""

import ctypes as C
import os
import subprocess
import sys

import gw_whisper_amd
from gw_whisper_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("gww_encoder_train_forward_f32", "gww_encoder_train_backward_f32", "gww_train_saved_bytes_f32",
       "gww_train_workspace_bytes_f32", "gww_attention_lse_f32", "gww_attention_bwd_f32",
       "gww_attention_bwd_f32_scratch_bytes", "gww_adapter_grads_f32", "gww_adapter_grads_f32_scratch_bytes")


def test_fp32_training_symbols_exported_and_bound():
    lib = gw_whisper_amd.lib()
    header = open(os.path.join(ROOT, "include", "gww.h")).read()
    for s in NEW:
        assert hasattr(lib, s) and s in _lib.SIGNATURES and f"{s}(" in header, s


def test_fp32_training_entries_reject_bad_arguments():
    lib = gw_whisper_amd.lib()
    assert lib.gww_train_saved_bytes_f32(None, 4) == 0 and lib.gww_train_workspace_bytes_f32(None, 4) == 0
    assert lib.gww_encoder_train_forward_f32(None, None, 1, None, 0, None, 0, None, 0, None) == -1
    assert b"NULL" in lib.gww_last_error()
    assert lib.gww_encoder_train_backward_f32(None, 1, None, 0, None, 0, None, None, 0, None, None, 0, None) == -1
    assert b"NULL" in lib.gww_last_error()
    assert lib.gww_attention_lse_f32(None, None, None, 1, 77, 2, None) == -1
    assert b"NULL" in lib.gww_last_error()
    assert lib.gww_attention_bwd_f32(None, None, None, None, None, None, 1, 77, 2, None) == -1
    assert b"NULL" in lib.gww_last_error()
    assert lib.gww_adapter_grads_f32(None, 128, None, None, 128, None, 1.0, 1.0, None, None, None, None, None, None,
                                     None, 16, 128, 128, 8, None, 0, None) == -1
    assert b"NULL" in lib.gww_last_error()
    fake = [C.c_void_p(4096 * (i + 1)) for i in range(11)]   # never dereferenced: the rank check comes first
    for r in (0, 65):
        rc = lib.gww_adapter_grads_f32(fake[0], 128, fake[1], fake[2], 128, fake[3], 1.0, 1.0, fake[4], fake[5], fake[6],
                                       fake[7], fake[8], fake[9], fake[10], 16, 128, 128, r, None, 0, None)
        assert rc == -1 and b"rank" in lib.gww_last_error(), r
    assert lib.gww_adapter_grads_f32_scratch_bytes(16, 128, 128, 0) == 0
    assert lib.gww_adapter_grads_f32_scratch_bytes(16, 128, 128, 65) == 0
    assert lib.gww_attention_bwd_f32_scratch_bytes(2, 77, 3) == 2 * 3 * (77 + 3) * 4


def _fake(i):
    return C.c_void_p(4096 * (i + 1))   # 256-byte aligned, never dereferenced: every call below fails its checks first


def test_fp32_entries_reject_each_null_pointer():
    """One NULL among otherwise valid-looking pointers is enough (not only the first argument of each entry)."""
    lib = gw_whisper_amd.lib()
    fwd = [_fake(0), _fake(1), 2, _fake(2), 1 << 20, _fake(3), 1 << 20, _fake(4), 0, None]
    for i in (1, 3, 5, 7):   # mel, workspace, saved, last_hidden
        args = list(fwd)
        args[i] = None
        assert lib.gww_encoder_train_forward_f32(*args) == -1 and b"NULL" in lib.gww_last_error(), i
    bwd = [_fake(0), 2, _fake(1), 1 << 20, _fake(2), 1 << 20, _fake(3), None, 0, None, None, 0, None]
    for i in (2, 4, 6):      # workspace, saved, d_last_hidden
        args = list(bwd)
        args[i] = None
        assert lib.gww_encoder_train_backward_f32(*args) == -1 and b"NULL" in lib.gww_last_error(), i
    args = list(bwd)
    args[8] = 1              # one target, no target array
    assert lib.gww_encoder_train_backward_f32(*args) == -1 and b"bad argument" in lib.gww_last_error()
    att = [_fake(i) for i in range(6)]
    for i in range(6):
        args = list(att)
        args[i] = None
        assert lib.gww_attention_bwd_f32(*args, 1, 77, 2, None) == -1 and b"NULL" in lib.gww_last_error(), i
    for i in range(3):
        args = [_fake(j) for j in range(3)]
        args[i] = None
        assert lib.gww_attention_lse_f32(*args, 1, 77, 2, None) == -1 and b"NULL" in lib.gww_last_error(), i
    ptr_slots = (0, 2, 3, 5, 8, 9, 10, 11, 12, 13, 14)   # X, dY, Y, bias, A, B, mag, nrm, dA, dB, dm
    for i in ptr_slots:
        args = [_fake(j) if j in ptr_slots else v for j, v in
                enumerate([None, 128, None, None, 128, None, 1.0, 1.0] + [None] * 7)]
        args[i] = None
        assert lib.gww_adapter_grads_f32(*args, 16, 128, 128, 8, None, 0, None) == -1, i
        assert b"NULL" in lib.gww_last_error(), i


def _backward_entries(lib):
    """(name, call(targets, n)) of the three backward entry points on fake, never dereferenced arguments."""
    head = [_fake(0), 2, _fake(1), 1 << 20, _fake(2), 1 << 20, _fake(3)]
    return [("gww_encoder_train_backward", lambda t, n: lib.gww_encoder_train_backward(*head, t, n, None, None, 0, None)),
            ("gww_encoder_train_backward_full",
             lambda t, n: lib.gww_encoder_train_backward_full(*head, t, n, None, None, 0, None, None)),
            ("gww_encoder_train_backward_f32", lambda t, n: lib.gww_encoder_train_backward_f32(*head, t, n, None, None, 0, None))]


def test_fp32_backward_rejects_target_ranks_before_any_hip_call():
    """The per-target checks shared by gww_encoder_train_backward_f32 and the two bf16 entries (check_targets,
    csrc/encoder_impl.h): rank 0 or 65 and a NULL gradient pointer are refused before the handle is read or anything is
    launched."""
    lib = gw_whisper_amd.lib()
    for name, call in _backward_entries(lib):
        for r, null_dm in ((0, False), (65, False), (8, True)):
            t = (_lib.DoraTarget * 1)()
            t[0] = _lib.DoraTarget(0, 4, r, 4.0, *(_fake(10 + j).value for j in range(6)), None if null_dm else _fake(20).value)
            assert call(t, 1) == -1, (name, r)
            assert (b"NULL pointer in target" if null_dm else b"rank") in lib.gww_last_error(), (name, r)


def test_backward_entries_refuse_duplicate_targets_before_any_hip_call():
    """Two targets with the same (layer, proj) are refused by all three backward entry points with the argument-error
    status, before the handle is read or anything is launched, and the message names the duplicate."""
    lib = gw_whisper_amd.lib()
    for name, call in _backward_entries(lib):
        t = (_lib.DoraTarget * 3)()
        for i, (layer, proj) in enumerate(((1, 3), (0, 0), (1, 3))):
            t[i] = _lib.DoraTarget(layer, proj, 8, 4.0, *(_fake(10 + 7 * i + j).value for j in range(7)))
        assert call(t, 3) == -1, name
        err = lib.gww_last_error()
        assert b"duplicate" in err and b"layer 1 proj 3" in err and b"0 and 2" in err, (name, err)


def test_fp32_adapter_grads_rejects_misaligned_scratch():
    lib = gw_whisper_amd.lib()
    args = [_fake(0), 128, _fake(1), _fake(2), 128, _fake(3), 1.0, 1.0] + [_fake(4 + j) for j in range(7)]
    rc = lib.gww_adapter_grads_f32(*args, 16, 128, 128, 8, C.c_void_p(4096 + 16), 1 << 20, None)
    assert rc == -1 and b"scratch" in lib.gww_last_error()


def test_run_train_help_lists_precision():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "harness", "run_train.py"), "--help"], capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0 and "--precision" in r.stdout and "fp32" in r.stdout
