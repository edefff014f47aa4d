"""The order-preserving integer images of csrc/device_sort.h on the host: the header's three functions, compiled for the
CPU with the host compiler, against a numpy restatement of the four key functions the kernels had before they shared one
(``roc_key``, ``sel_key`` / ``sel_value``, ``fkey`` / ``fkey_inv``, ``sc_key``), bit for bit.  The header's images have no
NaN rule and fold no zeros; each kernel's one-line special case is restated here beside the call."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

WRAPPER = """
#include "device_sort.h"
#include <string.h>
// bit patterns in and out: a NaN's payload must survive the call
extern "C" void key32(const unsigned* bits, unsigned* key, int n) {
  for (int i = 0; i < n; ++i) { float v; memcpy(&v, bits + i, 4); key[i] = gww::ordered_u32(v); }
}
extern "C" void inv32(const unsigned* key, unsigned* bits, int n) {
  for (int i = 0; i < n; ++i) { const float v = gww::from_ordered_u32(key[i]); memcpy(bits + i, &v, 4); }
}
extern "C" void key64(const unsigned long long* bits, unsigned long long* key, int n) {
  for (int i = 0; i < n; ++i) { double v; memcpy(&v, bits + i, 8); key[i] = gww::ordered_u64(v); }
}
"""

# +-0, +-denormals, +-inf, NaN of both signs (quiet, signalling, all-ones payload), +-1.5 and their neighbours, the extremes
BITS32 = np.array([0x00000000, 0x80000000, 0x00000001, 0x80000001, 0x007FFFFF, 0x807FFFFF, 0x00800000, 0x80800000,
                   0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00000, 0x7F800001, 0xFF800001, 0x7FFFFFFF, 0xFFFFFFFF,
                   0x3FC00000, 0xBFC00000, 0x3FBFFFFF, 0x3FC00001, 0xBFBFFFFF, 0xBFC00001, 0x7F7FFFFF, 0xFF7FFFFF], np.uint32)
BITS64 = np.array([0x0000000000000000, 0x8000000000000000, 0x0000000000000001, 0x8000000000000001, 0x000FFFFFFFFFFFFF,
                   0x800FFFFFFFFFFFFF, 0x0010000000000000, 0x8010000000000000, 0x7FF0000000000000, 0xFFF0000000000000,
                   0x7FF8000000000000, 0xFFF8000000000000, 0x7FF0000000000001, 0xFFF0000000000001, 0x7FFFFFFFFFFFFFFF,
                   0xFFFFFFFFFFFFFFFF, 0x3FF8000000000000, 0xBFF8000000000000, 0x3FF7FFFFFFFFFFFF, 0x3FF8000000000001,
                   0xBFF7FFFFFFFFFFFF, 0xBFF8000000000001, 0x7FEFFFFFFFFFFFFF, 0xFFEFFFFFFFFFFFFF], np.uint64)


@pytest.fixture(scope="module")
def keys(tmp_path_factory):
    d = tmp_path_factory.mktemp("ordered_keys")
    src, so = d / "keys.cpp", d / "keys.so"
    src.write_text(WRAPPER)
    cxx = os.environ.get("CXX") or shutil.which("c++") or "g++"
    subprocess.run([cxx, "-O2", "-std=c++17", "-shared", "-fPIC", "-I", os.path.join(ROOT, "gw_whisper_amd", "csrc"), str(src),
                    "-o", str(so)], check=True)
    lib = ctypes.CDLL(str(so))
    for fn in (lib.key32, lib.inv32, lib.key64):
        fn.restype, fn.argtypes = None, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int]
    return lib


# ---- the four functions as the kernels had them, in numpy, on the bit patterns ------------------------------------------------
def image32(u):
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000))


def fkey(u):
    return image32(u)


def fkey_inv(k):
    return np.where(k & np.uint32(0x80000000), k & np.uint32(0x7FFFFFFF), ~k)


def sel_key(u):
    return np.where(np.isnan(u.view(np.float32)), np.uint32(0xFFFFFFFF), image32(u))


def sel_value(k):
    return np.where(k == np.uint32(0xFFFFFFFF), np.uint32(0x7FC00000), fkey_inv(k))


def roc_key(u):
    v = u.view(np.float32)
    u = np.where(v == 0, np.uint32(0), u)                    # -0.0 and +0.0 are one value
    return np.where(np.isnan(v), np.uint32(0), ~image32(u))


def sc_key(u):
    v = u.view(np.float64)
    u = np.where(v == 0, np.uint64(0), u)
    top = np.uint64(0x8000000000000000)
    return np.where(np.isnan(v), ~np.uint64(0), np.where(u & top, ~u, u | top))


# ---- the header's functions through ctypes ---------------------------------------------------------------------------------
def _call(fn, x):
    x = np.ascontiguousarray(x)
    out = np.empty_like(x)
    fn(x.ctypes.data, out.ctypes.data, x.size)
    return out


def c_key32(lib, u):
    return _call(lib.key32, u.astype(np.uint32))


def c_inv32(lib, k):
    return _call(lib.inv32, k.astype(np.uint32))


def c_key64(lib, u):
    return _call(lib.key64, u.astype(np.uint64))


def test_logmel_keys(keys):
    """fkey / fkey_inv: the plain image and its inverse, NaNs included"""
    got = c_key32(keys, BITS32)
    assert np.array_equal(got, fkey(BITS32))
    assert np.array_equal(c_inv32(keys, got), fkey_inv(got))
    assert np.array_equal(c_inv32(keys, got), BITS32)


def test_detect_keys(keys):
    """sel_key: a NaN is 0xFFFFFFFF; sel_value: 0xFFFFFFFF comes back as the canonical NaN"""
    nan = np.isnan(BITS32.view(np.float32))
    got = np.where(nan, np.uint32(0xFFFFFFFF), c_key32(keys, BITS32))
    assert np.array_equal(got, sel_key(BITS32))
    k = sel_key(BITS32)
    back = np.where(k == np.uint32(0xFFFFFFFF), np.uint32(0x7FC00000), c_inv32(keys, k))
    assert np.array_equal(back, sel_value(k))
    assert got[0] != got[1]                                   # -0.0 and +0.0 stay two keys


def test_roc_keys(keys):
    """roc_key: a NaN is 0, the zeros fold, the key is the complement of the image"""
    v = BITS32.view(np.float32)
    folded = np.where(v == 0, np.uint32(0), BITS32)
    got = np.where(np.isnan(v), np.uint32(0), ~c_key32(keys, folded))
    assert np.array_equal(got, roc_key(BITS32))
    assert got[0] == got[1]


def test_score_keys(keys):
    """sc_key: a NaN is all ones, the zeros fold"""
    v = BITS64.view(np.float64)
    folded = np.where(v == 0, np.uint64(0), BITS64)
    got = np.where(np.isnan(v), ~np.uint64(0), c_key64(keys, folded))
    assert np.array_equal(got, sc_key(BITS64))
    assert got[0] == got[1]


def test_images_preserve_the_order(keys):
    for bits, fn, ft in ((BITS32, c_key32, np.float32), (BITS64, c_key64, np.float64)):
        b = bits[~np.isnan(bits.view(ft))]
        v, k = b.view(ft), fn(keys, b)
        o = np.argsort(k, kind="stable")
        assert (np.diff(v[o]) >= 0).all() and np.unique(k).size == k.size
        zeros = k[v == 0]
        assert zeros[1] + 1 == zeros[0]                       # -0.0 sits just below +0.0
