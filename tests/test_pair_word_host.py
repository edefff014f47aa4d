"""The packed count pair of csrc/device_compact.h on the host: ``pair_word`` / ``pair_first`` / ``pair_second`` compiled
for the CPU with the host compiler (the pattern of tests/test_ordered_keys_host.py).  Two counts travel as one 64-bit word
and add as words; the entry points take at most 2^27 elements, so at the bound both halves hold 2^27 and nothing crosses
bit 32."""
import ctypes
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

WRAPPER = """
#include "device_compact.h"
extern "C" unsigned long long word(int first, int second) { return gww::pair_word(first != 0, second != 0); }
// n_first words of a first-list element and n_second of a second-list one, added one by one
extern "C" unsigned long long sum(long n_first, long n_second) {
  unsigned long long w = 0ull;
  for (long i = 0; i < n_first; ++i) w += gww::pair_word(true, false);
  for (long i = 0; i < n_second; ++i) w += gww::pair_word(false, true);
  return w;
}
extern "C" unsigned first(unsigned long long w) { return gww::pair_first(w); }
extern "C" unsigned second(unsigned long long w) { return gww::pair_second(w); }
"""


@pytest.fixture(scope="module")
def pair(tmp_path_factory):
    d = tmp_path_factory.mktemp("pair_word")
    src, so = d / "pair.cpp", d / "pair.so"
    src.write_text(WRAPPER)
    cxx = os.environ.get("CXX") or shutil.which("c++") or "g++"
    subprocess.run([cxx, "-O2", "-std=c++17", "-shared", "-fPIC", "-I", os.path.join(ROOT, "gw_whisper_amd", "csrc"), str(src),
                    "-o", str(so)], check=True)
    lib = ctypes.CDLL(str(so))
    lib.word.restype, lib.word.argtypes = ctypes.c_ulonglong, [ctypes.c_int, ctypes.c_int]
    lib.sum.restype, lib.sum.argtypes = ctypes.c_ulonglong, [ctypes.c_long, ctypes.c_long]
    for fn in (lib.first, lib.second):
        fn.restype, fn.argtypes = ctypes.c_uint, [ctypes.c_ulonglong]
    return lib


def test_an_element_counts_once(pair):
    """first wins: an element of the first list is not counted in the second as well"""
    assert pair.word(0, 0) == 0
    assert pair.word(1, 0) == pair.word(1, 1) == 1 << 32
    assert pair.word(0, 1) == 1


def test_both_halves_hold_the_bound(pair):
    n = 1 << 27
    w = pair.sum(n, n)
    assert w == (n << 32) | n
    assert (pair.first(w), pair.second(w)) == (n, n)
    assert (pair.first(pair.sum(n, 0)), pair.second(pair.sum(n, 0))) == (n, 0)
    assert (pair.first(pair.sum(0, n)), pair.second(pair.sum(0, n))) == (0, n)
    assert (pair.first(pair.sum(3, 1025)), pair.second(pair.sum(3, 1025))) == (3, 1025)
