"""The impulse comb: an input on which a rational-ratio polyphase resampler's output is known EXACTLY, tap by tap, in
any arithmetic -- the yardstick of mm_resample_banded_f32 (matrix pipe, host-built operand tables) and mm_resample_f32
(tests/test_resample_host.py, tests/test_gpu_resample.py).

The resampler computes  y[m] = sum_j h[ph + j L] x[ih - j],  t = m M + half, ih = t div L, ph = t mod L  (h = the
float32 taps of audio_io.design_taps, zero signal outside the clip).  One impulse of amplitude a at input sample p
therefore gives  y[m] = a h[m M + half - p L]  where that index lies inside the filter and zero elsewhere.

The comb puts S impulses (S = the banded operator's input period, F M / L) at  lead + s W,  s < S,  with W = 1 (mod S)
and W larger than the filter's reach in input samples (ceil(len(h) / L) + 2), amplitudes +-2^k, k in -2 .. 2:

  * no two responses overlap, and every output's sum holds at most ONE non-zero product a h -- exact in float32
    (a power of two times a float32) -- beside products that are +-0: the expected output is exact whatever the order
    of summation, the accumulator type or the number of accumulator chains;
  * the positions run through every residue mod S and gcd(L, M) = 1, so every entry A[b][r][k] of the banded operator
    (audio_io.banded_tables) meets exactly one impulse in exactly one output, and every tap h[i] appears in exactly
    F / L outputs: count_nonzero(want) == count_nonzero(h) F / L says that no tap of no copy was skipped;
  * `lead` and a tail of the filter's reach keep every response inside the clip.  The EDGE comb drops both: an impulse
    sits on sample 0 and one on sample n - 1, and only the part of their responses inside [0, n_out) is expected --
    that pins the zero fill outside the clip and the last partial period.

`want` is computed from the formula above with integer index arithmetic only: not from banded_tables, and not through
scipy.signal.resample_poly (whose window = h / L times L round trip is not exact).  Both kernels start their sums at
+0.0 and add the +-0 products in round-to-nearest, so every expected zero is +0.0: `want` carries no -0.0.

Nothing in the package imports this module.
"""
from __future__ import annotations

import ctypes as C
import functools

import numpy as np

# (sr_in, sr_out) of every rate pair the GPU file runs.  Classified by mm_resample_banded_shape (test_resample_host.py
# asserts the coverage; L / M, QT, pad, G % 3 with G = ksteps / 8, F % 16 as the library reports them):
MATRIX = (
    (48000, 16000),     # 1 / 3      QT 8  pad  G%3 2  F%16 0   NB 1
    (16000, 48000),     # 3 / 1      QT 8  -    G%3 1  F%16 14
    (16000, 10000),     # 5 / 8      QT 8  pad  G%3 2  F%16 14
    (16000, 12000),     # 3 / 4      QT 8  pad  G%3 0  F%16 14
    (44100, 16000),     # 160 / 441  QT 2  -    G%3 0  F%16 0
    (44100, 10000),     # 100 / 441  QT 2  -    G%3 1  F%16 4
    (22050, 10000),     # 200 / 441  QT 2  -    G%3 2  F%16 8
    (48000, 44100),     # 147 / 160  QT 4  pad  G%3 1  F%16 3
    (192000, 16000),    # 1 / 12     QT 4  pad  G%3 1  F%16 0   NB 1
    (16000, 11025),     # 441 / 640  QT 1  pad  G%3 1  F%16 9   NB 28
    (44100, 48000),     # 160 / 147  QT 8  -    G%3 1  F%16 0
)
UNSUPPORTED = (
    (48000, 250),       # 1 / 192: S = 3072, a window of ~37 k samples
    (44100, 250),       # 5 / 882: S = 14112
)


def ratio_id(pair):
    return f"{pair[0]}to{pair[1]}"


@functools.lru_cache(maxsize=None)
def tables(sr_in, sr_out):
    """dict(L, M, h32 float32 taps, half, tabs = audio_io.banded_tables of those taps) for a rate pair."""
    from modulation_mfcc_amd.audio_io import banded_tables, design_taps, resample_ratio
    L, M = resample_ratio(sr_in, sr_out)
    h, half = design_taps(L, M)
    h32 = h.astype(np.float32)
    h32.setflags(write=False)
    return dict(L=L, M=M, h32=h32, half=half, tabs=banded_tables(L, M, h32.astype(np.float64), half))


def shape_of(tabs):
    """mm_resample_banded_shape for a table set: (status, qt, pad, lds_bytes); no GPU involved."""
    from modulation_mfcc_amd import _lib
    lib = _lib.load()
    qt, pad, lds = C.c_int32(-1), C.c_int32(-1), C.c_size_t(0)
    rc = lib.mm_resample_banded_shape(tabs["F"], tabs["S"], tabs["NB"], tabs["ksteps"], tabs["win"], C.byref(qt),
                                      C.byref(pad), C.byref(lds))
    return rc, qt.value, pad.value, lds.value


def amplitude(s):
    """+-2^k, k in -2 .. 2, varying with the impulse number."""
    return np.float32((-1.0 if s % 3 == 1 else 1.0) * 2.0 ** (s % 5 - 2))


def response(want, tap, h32, L, M, half, p, a):
    """Add the exact response of one impulse (sample p, amplitude a) to want [n_out]; tap [n_out] receives the filter
    index each touched output reads (-1 elsewhere).  Integer index arithmetic only."""
    n_out, nh = want.shape[0], h32.shape[0]
    # 0 <= m M + half - p L < nh
    m_lo = max(0, -(-(p * L - half) // M))
    m_hi = min(n_out - 1, (p * L - half + nh - 1) // M)
    if m_hi < m_lo:
        return
    m = np.arange(m_lo, m_hi + 1, dtype=np.int64)
    idx = m * M + half - p * L
    assert idx.min() >= 0 and idx.max() < nh
    assert (tap[m_lo:m_hi + 1] == -1).all(), "two impulse responses overlap"
    want[m_lo:m_hi + 1] = a * h32[idx]                 # a power of two times a float32: exact
    tap[m_lo:m_hi + 1] = idx


@functools.lru_cache(maxsize=None)
def comb(sr_in, sr_out, edge=False):
    """(x float32 [n], want float32 [n_out], tap int64 [n_out]) -- the impulse comb of a rate pair (module docstring);
    edge: without lead-in and tail.  Arrays are shared and read-only."""
    t = tables(sr_in, sr_out)
    L, M, h32, half, S = t["L"], t["M"], t["h32"], t["half"], t["tabs"]["S"]
    reach = -(-len(h32) // L) + 2
    W = (reach // S + 1) * S + 1                       # = 1 (mod S), > reach
    assert W % S == 1 % S and W > reach
    lead = 0 if edge else reach
    n = lead + (S - 1) * W + 1 + (0 if edge else reach)
    n_out = -(-n * L // M)
    x = np.zeros(n, dtype=np.float32)
    want = np.zeros(n_out, dtype=np.float32)
    tap = np.full(n_out, -1, dtype=np.int64)
    for s in range(S):
        p = lead + s * W
        x[p] = amplitude(s)
        response(want, tap, h32, L, M, half, p, amplitude(s))
    want[want == 0] = 0.0                              # a zero tap times a negative amplitude: the kernels' sums give +0.0
    for a in (x, want, tap):
        a.setflags(write=False)
    return x, want, tap


def bits(a):
    """float32 array -> its uint32 bit patterns (NaN payloads and the sign of zero count)."""
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)
