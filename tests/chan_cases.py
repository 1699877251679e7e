"""Cases and float64 reference of the channelizer sweep (tests/test_gpu_chan_sweep.py; tests/test_chan_cases_design.py keeps this module
honest without a GPU).  The reference has no channelizer, so the defining sum of include/sonde_chan.h is the oracle:

    y_k[m] = sum_n h[n] x[m D - n] exp(-2 pi i k (m D - n) / M),   x = 0 before the stream starts.

Everything here is numpy in float64; nothing touches the GPU."""
import functools

import numpy as np

CH_F = 16                      # output samples per workgroup (sonde_chan.hip)
CH_THREADS = 256
EPS = 2.0 ** -24               # float32 unit roundoff

# (M, D, P): each is the smallest place where a different part of the kernel can go wrong
RUN = [
    (16, 16, 4),               # smallest M and P; D = M so the phase is always 1; 8 butterflies per transform
    (16, 1, 32),               # D = 1; largest P
    (64, 48, 8),               # shape of tests/test_gpu_chan.py
    (128, 77, 6),              # odd D so the phase index visits every value; P not a power of two
    (256, 200, 16),            # product default
    (256, 256, 16),            # 64 512 B of LDS, just under 64 KB
    (256, 200, 32),            # first shape above 64 KB
    (512, 400, 8),             # two iterations of the thread-strided loops
    (1024, 128, 4),            # four iterations; 155 136 B, near the device limit
]
REFUSED = [(1024, 800, 8), (1024, 1024, 32)]          # accepted by the M, D, P ranges, too large for the LDS of a compute unit
LDS_LIMIT = 160 * 1024                                 # gfx950


def case_id(c):
    return "M%d_D%d_P%d" % c


def lds_bytes(M, D, P):
    """dynamic LDS of one k_channelize launch: the staged span of raw cs16 words, rounded up to even, and CH_F transforms of M complex floats"""
    span = M * P + (CH_F - 1) * D
    return 4 * ((span + 1) & ~1) + 8 * CH_F * M


def stream_len(M, D, P):
    """three full workgroups of 16 output samples and a partial one, with the filter full"""
    return M * P + 48 * D + 5


def n_frames(n, D):
    return (n - 1) // D + 1 if n > 0 else 0


@functools.lru_cache(maxsize=None)
def taps(M, P):
    """the prototype as sonde_chan_create designs it, operation for operation: Blackman-windowed sinc in float64, -6 dB at half the channel
    spacing, divided by its sum (accumulated in order), rounded to float32"""
    T = M * P
    fc = 0.5 / M
    n = np.arange(T, dtype=np.float64)
    t = n - 0.5 * (T - 1)                                   # never 0: T is even
    x = 2.0 * np.pi * fc * t
    w = 0.42 - 0.5 * np.cos(2.0 * np.pi * n / (T - 1)) + 0.08 * np.cos(4.0 * np.pi * n / (T - 1))
    hd = 2.0 * fc * (np.sin(x) / x) * w
    h = (hd / np.cumsum(hd)[-1]).astype(np.float32)
    h.setflags(write=False)
    return h


def to_complex(xi):
    """interleaved int16 -> complex128 at the kernel's scale (2^-15)"""
    xi = np.asarray(xi)
    return (xi[0::2].astype(np.float64) + 1j * xi[1::2].astype(np.float64)) / 32768.0


def reference(x, h, M, D, frames):
    """-> (y [M][len(frames)] complex128, ||u||_2 per frame, ||A||_2 per frame).
    x: complex128 stream, h: the float32 taps (widened here, so their rounding is no part of any tolerance).  Per frame m:
    v[n] = h[n] x[mD - n]; folded into M bins by (mD - n) mod M; np.fft.fft of the bins is the defining sum over all k.
    u[r] = sum_p h[r + pM] x[mD - r - pM] are the branch sums the kernel forms, A[r] = sum_p |h| |x| their magnitude budget
    (real and imaginary parts separately, combined in quadrature)."""
    h = np.asarray(h, np.float64)
    T = len(h)
    P = T // M
    frames = np.asarray(frames, np.int64)
    idx = frames[:, None] * D - np.arange(T)[None, :]                         # [F][T] stream index of tap n
    xv = np.where(idx >= 0, x[np.clip(idx, 0, len(x) - 1)], 0.0)
    assert idx.max() < len(x)
    v = h[None, :] * xv
    u = v.reshape(len(frames), P, M).sum(axis=1)                              # [F][M], branch r
    a_re = (np.abs(h)[None, :] * np.abs(xv.real)).reshape(len(frames), P, M).sum(axis=1)
    a_im = (np.abs(h)[None, :] * np.abs(xv.imag)).reshape(len(frames), P, M).sum(axis=1)
    bins = np.zeros((len(frames), M), np.complex128)
    b = (frames[:, None] * D - np.arange(M)[None, :]) % M                     # bin of branch r: (mD - r) mod M, one to one
    np.put_along_axis(bins, b, u, axis=1)
    y = np.fft.fft(bins, axis=1).T
    return y, np.linalg.norm(u, axis=1), np.sqrt((a_re ** 2 + a_im ** 2).sum(axis=1))


def bound(M, P, u_norm, a_norm):
    """||y^_m - y_m||_2 <= 2^-24 sqrt(M) (8 log2(M) ||u_m||_2 + (P + 2) ||A_m||_2): P fused multiply-adds per branch sum, the 2^-15 scale and
    the phase multiply (+2), and the radix-2 float32 transform with the constant tests/test_gpu_power.py uses; sqrt(M) is the transform's gain"""
    return EPS * np.sqrt(M) * (8.0 * np.log2(M) * u_norm + (P + 2) * a_norm)


def direct(x, h, M, D, m_list, k_list):
    """the brute-force sum of tests/test_gpu_chan.py::_direct, term by term in float64: pins the fold and the transform's sign"""
    h = np.asarray(h, np.float64)
    out = np.zeros((len(k_list), len(m_list)), np.complex128)
    n = np.arange(len(h))
    for j, m in enumerate(m_list):
        idx = m * D - n
        xv = np.where(idx >= 0, x[np.clip(idx, 0, len(x) - 1)], 0)
        for i, k in enumerate(k_list):
            out[i, j] = np.sum(h * xv * np.exp(-2j * np.pi * k * idx / M))
    return out


# ------------------------------------------------------------------------------------------------------------------------------ inputs
INPUTS = ("uniform", "impulse", "tone")
TONE_AMP = 0.9


def tone_channel(M):
    return M - 3                                            # a negative frequency


def impulse_index(M, D, P):
    """the lone sample sits where its M P taps straddle the edge between the first two workgroups: output samples 15 and 16 both see it"""
    return max(0, CH_F * D - M * P // 2)


@functools.lru_cache(maxsize=None)
def stream(M, D, P, kind, n=None):
    """interleaved int16, read-only.
    uniform: the whole int16 range, both rails on both parts in the first samples (the sign extension of the packed cs16 word);
    impulse: one full-scale sample (32767 - 32768 i): every output is one tap times one phase;
    tone:    0.9 of full scale exactly on channel M - 3."""
    n = stream_len(M, D, P) if n is None else n
    if kind == "uniform":
        x = np.random.default_rng(1000 * M + 10 * D + P).integers(-32768, 32768, size=2 * n).astype(np.int16)
        x[:8] = [-32768, 32767, 32767, -32768, -32768, -32768, 32767, 32767]
    elif kind == "impulse":
        x = np.zeros(2 * n, np.int16)
        i0 = impulse_index(M, D, P)
        x[2 * i0], x[2 * i0 + 1] = 32767, -32768
    elif kind == "tone":
        z = TONE_AMP * 32768.0 * np.exp(2j * np.pi * tone_channel(M) * np.arange(n) / M)
        x = np.empty(2 * n, np.int16)
        x[0::2], x[1::2] = np.round(z.real), np.round(z.imag)
    else:
        raise ValueError(kind)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def expected(M, D, P, kind, n=None):
    """reference over every frame of stream(...): computed once, shared, read-only"""
    xi = stream(M, D, P, kind, n)
    out = reference(to_complex(xi), taps(M, P), M, D, np.arange(n_frames(len(xi) // 2, D)))
    for a in out:
        a.setflags(write=False)
    return out


def first_full_frame(M, D, P):
    """first output sample whose M P taps all lie inside the stream"""
    return (M * P - 1 + D - 1) // D


def quant_allowance(M, P):
    """what rounding the tone to int16 can move any output by at most: half a step on both parts of every sample, sum |h| of them"""
    return 2.0 ** -16 * np.sqrt(2.0) * np.abs(taps(M, P).astype(np.float64)).sum()


@functools.lru_cache(maxsize=None)
def stopband_level(M, P):
    """largest |H(f)| of the prototype two channel spacings and more from its centre (the Blackman main lobe ends 0.5 + 3 / P <= 1.25
    spacings out), on a grid 16 times finer than 1 / (M P), times the tone's amplitude, plus the tone's own quantisation allowance"""
    h = taps(M, P).astype(np.float64)
    nfft = 16 * len(h)
    H = np.abs(np.fft.fft(h, nfft))
    f = np.minimum(np.arange(nfft), nfft - np.arange(nfft)) / nfft            # |f| in cycles per sample
    return TONE_AMP * H[f >= 2.0 / M].max() + quant_allowance(M, P)


# ------------------------------------------------------------------------------------------------------------------------------ call cuts
def cut_stream_len(M, D, P):
    """the listed calls add up to 4 D + 3 M P samples, more than stream_len() for most shapes: the cut test draws the uniform input at this
    length instead, the listed calls and a rest of a workgroup and more"""
    return max(stream_len(M, D, P), min(D + 3, 260) + 3 * D + 3 * M * P - 3 + CH_F * D + 5)


def cuts(M, D, P, n):
    """call lengths in stream order: min(D + 3, 260) single samples, a zero-length call, D - 1, D, D + 1, T - 2, T - 1, T, the rest at an odd count"""
    T = M * P
    seq = [1] * min(D + 3, 260) + [0, D - 1, D, D + 1, T - 2, T - 1, T]
    rest = n - sum(seq)
    assert rest > 1
    odd = (rest // 2) | 1
    return seq + [odd, rest - odd]
