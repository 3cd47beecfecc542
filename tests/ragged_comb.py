"""Prefixes of the edge comb: the exact yardstick of the ragged resamplers (mm_resample_banded_ragged_f32,
mm_resample_ragged_f32; tests/test_audio_batch_host.py, tests/test_gpu_resample_ragged.py).

A ragged row of length n_b must come out as the resampler's answer to x[:n_b] ALONE.  For the edge comb of
resample_comb.py (impulses at s W, s = 0, 1, ..., amplitudes +-2^k, W larger than the filter's reach) that answer is
known exactly: the responses (resample_comb.response) of the impulses at p < n_b, clipped to n_out_b = ceil(n_b L / M)
outputs -- an impulse at or behind n_b does not exist for the row, although the padded batch may hold it there.  The
comb is continued past resample_comb.comb's S impulses where a row has to span several LDS tiles (16 -> 48 kHz: the
comb proper is 1.4 tiles long); positions and amplitudes are those of resample_comb.comb(pair, edge=True) where both
exist (test_audio_batch_host.py asserts it).

Nothing in the package imports this module.
"""
from __future__ import annotations

import numpy as np

import resample_comb as RC

# the rate pairs of the ragged GPU file (resample_comb.MATRIX classifies them)
PAIRS = ((48000, 16000), (44100, 16000), (16000, 48000), (16000, 11025))


def spacing(pair):
    """W of resample_comb.comb: the distance between two impulses (= 1 mod S, larger than the filter's reach)."""
    t = RC.tables(*pair)
    reach = -(-len(t["h32"]) // t["L"]) + 2
    return (reach // t["tabs"]["S"] + 1) * t["tabs"]["S"] + 1


def edge_comb(pair, n):
    """float32 [n]: impulses of amplitude resample_comb.amplitude(s) at s W, s = 0, 1, ... while s W < n."""
    W = spacing(pair)
    x = np.zeros(n, dtype=np.float32)
    for s in range(-(-n // W)):
        x[s * W] = RC.amplitude(s)
    return x


def out_len(pair, n):
    t = RC.tables(*pair)
    return -(-int(n) * t["L"] // t["M"])


def prefix_want(pair, n_b, n_out_max=None):
    """float32 [n_out_max] (default n_out_b): what the resampler gives for edge_comb(pair, .)[:n_b] alone in the columns
    [0, n_out_b) -- the responses of the impulses at p < n_b, clipped to n_out_b --, +0.0 behind them."""
    t = RC.tables(*pair)
    W = spacing(pair)
    n_out_b = out_len(pair, n_b)
    want = np.zeros(n_out_b if n_out_max is None else n_out_max, dtype=np.float32)
    head = want[:n_out_b]
    tap = np.full(n_out_b, -1, dtype=np.int64)
    for s in range(-(-int(n_b) // W)):
        assert s * W < n_b
        RC.response(head, tap, t["h32"], t["L"], t["M"], t["half"], s * W, RC.amplitude(s))
    head[head == 0] = 0.0                               # a zero tap times a negative amplitude: the kernels' sums give +0.0
    return want


def shortest_for(pair, n_out):
    """The smallest n whose output count is >= n_out (== n_out for every n_out when L <= M)."""
    t = RC.tables(*pair)
    n = max(1, (int(n_out) - 1) * t["M"] // t["L"])
    while out_len(pair, n) < n_out:
        n += 1
    return n


def row_lengths(pair):
    """The rows of the tap-by-tap case: n_b such that n_out_b is 1, 2, 3 (upsampling by 3: 3 only), a value below F, F, one
    LDS tile of 16 QT F outputs less one / exactly / plus one (or the next reachable count), rows cut AT an impulse
    (x[n_b] is an impulse: the first sample the kernel must not read) and just behind one, and the longest row, three
    tiles and a partial period.  Returns (lengths int64 ascending and distinct, n_max = the last one, tile)."""
    t = RC.tables(*pair)
    F = t["tabs"]["F"]
    rc, qt, _, _ = RC.shape_of(t["tabs"])
    assert rc == 0
    tile = 16 * qt * F
    W = spacing(pair)
    n_max = shortest_for(pair, 3 * tile + F + 5)
    ns = {1, n_max}
    for target in (1, 2, 3, F - 3, F, tile - 1, tile, tile + 1):
        ns.add(shortest_for(pair, target))
    for s in (1, 2, n_max // W):                        # cut at an impulse / one sample behind it
        if 0 < s * W < n_max:
            ns.update((s * W, s * W + 1))
    return np.array(sorted(ns), dtype=np.int64), n_max, tile
