"""The survey's transform network (radiosonde_auto_rx_amd/csrc/sonde_power_fft.h: radix-8 register passes, exact twiddles, natural in /
bit-reversed out, |X|^2 accumulated in network order) executed on the CPU by tests/emu/power_fft_emu.cpp and compared with numpy's float64
FFT for every size the kernel is instantiated for.  The same source is compiled by hipcc into k_power_seg; tests/test_gpu_power.py runs it there."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU_SRC = os.path.join(ROOT, "tests", "emu", "power_fft_emu.cpp")
EMU_SO = os.path.join(ROOT, "tests", "emu", "libpower_fft_emu.so")
DEPS = [EMU_SRC, os.path.join(ROOT, "radiosonde_auto_rx_amd", "csrc", "sonde_power_fft.h")]


@pytest.fixture(scope="module")
def emu():
    if not os.path.exists(EMU_SO) or any(os.path.getmtime(d) > os.path.getmtime(EMU_SO) for d in DEPS):
        tmp = EMU_SO + ".%d.tmp" % os.getpid()
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", tmp, EMU_SRC])
        os.replace(tmp, EMU_SO)
    L = C.CDLL(EMU_SO)
    L.emu_power_segments.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_void_p]
    return L


def _brev(n):
    bits = n.bit_length() - 1
    k = np.arange(n)
    r = np.zeros(n, dtype=np.int64)
    for t in range(bits):
        r |= ((k >> t) & 1) << (bits - 1 - t)
    return r


@pytest.mark.parametrize("log2n", range(8, 15))
def test_network_matches_float64_fft(emu, log2n):
    """Two segments (the accumulator adds), a strong tone over noise so that the spectrum spans ~60 dB.  Bound: the radix-2 f32 rounding
    bound 8 log2(n) 2^-24 on the norm, as the GPU test uses."""
    n = 1 << log2n
    rng = np.random.default_rng(100 + log2n)
    t = np.arange(2 * n)
    x = 0.5 * np.exp(2j * np.pi * (37.3 / n) * t) + 0.001 * (rng.standard_normal(2 * n) + 1j * rng.standard_normal(2 * n))
    x32 = x.astype(np.complex64)
    out = np.zeros(n, np.float32)
    threads = emu.emu_power_segments(log2n, x32.view(np.float32).ctypes.data_as(C.c_void_p), 2, out.ctypes.data_as(C.c_void_p))
    assert threads == min(512, max(64, n // 8))
    ref = sum(np.abs(np.fft.fft(x32[s * n:(s + 1) * n].astype(np.complex128))) ** 2 for s in range(2))
    got = out[_brev(n)].astype(np.float64)
    err = np.linalg.norm(got - ref) / np.linalg.norm(ref)
    print("log2n %d: norm-wise error %.2e, worst bin %.2e dB" % (log2n, err, np.max(np.abs(10 * np.log10(got / ref)))))
    assert err <= 8 * log2n * 2.0 ** -24
    assert np.max(np.abs(10 * np.log10(got / ref))) <= 0.005


def test_unknown_size_is_refused(emu):
    assert emu.emu_power_segments(7, None, 0, None) == -1
    assert emu.emu_power_segments(15, None, 0, None) == -1
