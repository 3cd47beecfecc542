"""The yardstick of the top_db clamp + DCT-II stage (row A6: max(L, max(L) - top_db) over the clip, then the orthonormal
DCT-II along the mel axis): a float64 reference built on stage_oracle's log-mel reference, an error measure normalised by a
floor that is the FRAME's own and the COEFFICIENT's own, the same measure of float32 host pipelines the kernels get a fixed
margin over -- per coefficient index -- and the clip lengths that meet the kernels' frame tiles.  Host only; nothing in the
package imports this module.  The clips are stage_oracle.cases; MARGIN and EPS are modspec_oracle's.

Reference, for the case clips of a configuration (a dict of MfccConfig keywords; top_db defaults to 80, negative = no clamp)
at one length, in float64, from stage_oracle.reference: the log-mel L[b, t, m] and its floor dL[b, t, m]:

    thr_b = max_{t, m} L[b] - top_db          x = max(L, thr_b)          M[b, t, k] = sum_m D[k, m] x[b, t, m]

D is the orthonormal DCT-II matrix in float64 (scipy.fft.dct of the identity; not the library's mm_build_dct).

Floor.  The threshold inherits the floor of whichever element is the maximum.  An element can be the maximum a float32
pipeline finds when L + dL >= max(L - dL); d_thr_b is the largest dL among those.  max() is 1-Lipschitz in both arguments
(|max(a, b) - max(a', b')| <= max(|a - a'|, |b - b'|)), so a clamped value is uncertain by max(dL, d_thr) wherever the clamp
CAN be active (L - dL < thr + d_thr) and by dL elsewhere:

    d_x = max(dL, d_thr) where L - dL < thr + d_thr, else dL
    d_M[b, t, k] = sum_m |D[k, m]| d_x[b, t, m] + EPS (|M[b, t, k]| + sum_m |D[k, m]| |x[b, t, m]|)
    c_M[b, t, k] = |M_got[b, k, t] - M[b, t, k]| / d_M[b, t, k]                  (NaN counts as inf)

The first term carries the input's floor through the sum at its worst sign pattern; the second is the storage of the result
plus ONE rounding at the magnitude of the terms.  A float32 sum of n_mels terms of one sign (c0 of a frame on the amin
floor: every term is -100 D[0, m]) rounds n_mels times in the same direction class and reaches a few times that second term:
this is why the bound is taken per coefficient index --

    c_M[..., k].max() <= MARGIN * max(C_ref[k], 1)

with C_ref[k] the largest c_M at index k that two honest float32 host pipelines reach over the case set at every length of
frame_lengths(cfg).  Both are fed stage_oracle.host's float32 log-mel and clamp in float32 against the float32 clip maximum;
then (a) scipy.fftpack.dct(type=2, norm='ortho') in float32, (b) a float32 multiply and add over m ascending with the
float32-rounded D -- the order the lane <-> frame kernels sum in.  All of it is computed here, on the host, cached per
configuration, never from the code under test.  One constant for all k would loosen the high coefficients (C_ref[k >= 2]
stays below 1) by the factor c0 needs (about 2 .. 5 at 40 .. 128 filters).

The fused kernels store the DCT of the UNCLAMPED values before the clip maximum is known and add sum_m D[k, m] max(thr - L, 0)
to the clips that clamp (mm_clamp_corr).  Where most of a frame is clamped the two sums cancel, each as large as
sum |D| |L| with L tens of dB under the threshold, against a floor built from |x| = |thr|.  fused32 is that arithmetic on the
host; it is NOT part of C_ref: test_dct_host measures it at 0.25 .. 0.57 of the bound, so those kernels are held to the
same figures as every other.

What the bound does NOT see: a DCT table built from a float32 angle (cos of float32(pi (m + 1/2) k / n_mels)) stays at
0.3 .. 0.6 of the bound on the configurations probed -- its entries are off by a few 2^-24 with changing sign, which is the
size of the table's own float32 rounding.  A clamp threshold off by 0.001 dB at top_db 80 can move c0 alone on some plans.

    frame_lengths(cfg)             clip lengths with 1, 2, 15, 16, 17, 63, 64, 65, 255, 256, 257 frames (the 16-, 64- and
                                   256-frame tiles of the kernels, one fewer and one more), each >= 4 samples
    aligned_length(cfg, n)         n rounded up to a multiple of 4 with the same frame count (extra cases for kernels with
                                   an alignment gate, held to the bound of frame_lengths; C_ref is not taken over them)
    dct64(n_mels, n_mfcc)          D
    reference(cfg, n)              Ref(M, dM, L, dL, thr, d_thr) of stage_oracle.cases(n, cfg), cached; reference_from(L, dL, cfg)
    mfcc_error(got, ref)           c_M [B, T, n_mfcc] of got [B, n_mfcc, T]
    host_logmel(cfg, n)            stage_oracle.host's float32 log-mel [B, n_mels, T]
    clamp32, fftpack32, sequential32, fused32      the pieces of the float32 pipelines; the mutants of test_dct_host replace one
    c_ref(cfg), bounds(cfg)        C_ref[k] and MARGIN * max(C_ref[k], 1), arrays [n_mfcc]
    check_case_set(cfg)            the conditions on the case set every test relies on, asserted against the reference alone
"""
from __future__ import annotations

import functools
from collections import namedtuple

import numpy as np

import stage_oracle as S
from modspec_oracle import EPS, MARGIN

FRAME_EDGES = (1, 2, 15, 16, 17, 63, 64, 65, 255, 256, 257)
_STAGE_KEYS = ("sr", "n_fft", "win_length", "hop_length", "n_mels", "fmin", "fmax", "preemph", "amin")

Ref = namedtuple("Ref", "M dM L dL thr d_thr")      # [B, T, n_mfcc] twice; [B, T, n_mels] twice; [B, 1, 1] twice


def stage_cfg(cfg):
    """What the stages in front of the clamp read: two configurations that differ in n_mfcc / top_db share a log-mel."""
    return {k: cfg[k] for k in _STAGE_KEYS if k in cfg}


def top_db_of(cfg):
    """None for 'no clamp' (a negative top_db), else the value."""
    t = float(cfg.get("top_db", 80.0))
    return None if t < 0 else t


def frame_lengths(cfg):
    hop = int(cfg["hop_length"])
    assert hop >= 5, "frame_lengths: four samples in the last hop need hop_length >= 5"
    return tuple((T - 1) * hop + 4 for T in FRAME_EDGES)


def aligned_length(cfg, n):
    hop, m = int(cfg["hop_length"]), (int(n) + 3) & ~3
    assert m // hop == n // hop, (n, hop)
    return m


def dct64(n_mels, n_mfcc):
    from scipy import fft as sfft
    D = sfft.dct(np.eye(int(n_mels)), type=2, norm="ortho", axis=0)[:int(n_mfcc)]
    assert D.dtype == np.float64 and D.shape == (n_mfcc, n_mels)
    return D


def reference_from(L, dL, cfg):
    L, dL = np.asarray(L, dtype=np.float64), np.asarray(dL, dtype=np.float64)
    D = dct64(L.shape[-1], int(cfg["n_mfcc"]))
    aD = np.abs(D)
    top_db = top_db_of(cfg)
    if top_db is None:
        x, d_x = L, dL
        thr = np.full((L.shape[0], 1, 1), -np.inf)
        d_thr = np.zeros((L.shape[0], 1, 1))
    else:
        can_be_max = L + dL >= (L - dL).max(axis=(1, 2), keepdims=True)
        d_thr = np.where(can_be_max, dL, 0.0).max(axis=(1, 2), keepdims=True)
        thr = L.max(axis=(1, 2), keepdims=True) - top_db
        x = np.maximum(L, thr)
        d_x = np.where(L - dL < thr + d_thr, np.maximum(dL, d_thr), dL)
    M = x @ D.T
    dM = d_x @ aD.T + EPS * (np.abs(M) + np.abs(x) @ aD.T)
    return Ref(M, dM, L, dL, thr, d_thr)


@functools.lru_cache(maxsize=128)       # small arrays ([14, T, n_mels]); stage_oracle's own caches hold the spectra of 16 lengths
def _stage(k, n):
    cfg = dict(k)
    ref = S.reference(cfg, n)
    return ref.L, ref.dL, S.host(cfg, n)[1]


@functools.lru_cache(maxsize=48)
def _reference(k, n):
    cfg = dict(k)
    L, dL, _ = _stage(S.key(stage_cfg(cfg)), n)
    return reference_from(L, dL, cfg)


def reference(cfg, n):
    return _reference(S.key(cfg), int(n))


def host_logmel(cfg, n):
    return _stage(S.key(stage_cfg(cfg)), int(n))[2]


def mfcc_error(got, ref):
    """got as the plan returns it: [B, n_mfcc, T]."""
    got = np.swapaxes(np.asarray(got).astype(np.float64), -1, -2)
    assert got.shape == ref.M.shape, (got.shape, ref.M.shape)
    return S._ratio(np.abs(got - ref.M), ref.dM)


# ---- the float32 host pipelines ---------------------------------------------------------------------------------------------

def clip_max32(lm):
    lm = np.asarray(lm)
    assert lm.dtype == np.float32 and lm.ndim == 3
    return lm.reshape(lm.shape[0], -1).max(-1)


def clamp32(lm, top_db, thr=None):
    """float32 max(lm, max(lm) - top_db) per clip; thr [B] float32 replaces the threshold; top_db None: no clamp."""
    if top_db is None:
        return lm
    if thr is None:
        thr = clip_max32(lm) - np.float32(top_db)
    thr = np.asarray(thr, dtype=np.float32)
    return np.maximum(lm, thr[:, None, None])


def fftpack32(x, n_mfcc):
    """(a): scipy.fftpack.dct along the mel axis of [B, n_mels, T], in float32."""
    import scipy.fftpack
    M = scipy.fftpack.dct(np.ascontiguousarray(x), type=2, norm="ortho", axis=1)
    assert M.dtype == np.float32
    return np.ascontiguousarray(M[:, :int(n_mfcc)])


def sequential32(x, D):
    """(b): acc = acc + float32(D[k, m]) * x[m] in float32, m ascending -> [B, n_mfcc, T]."""
    D = np.asarray(D).astype(np.float32)
    assert x.dtype == np.float32
    acc = np.zeros((x.shape[0], D.shape[0], x.shape[2]), dtype=np.float32)
    for m in range(D.shape[1]):
        acc += D[None, :, m, None] * x[:, m, None, :]
    return acc


def fused32(lm, top_db, D):
    """The fused kernels' arithmetic (not in C_ref): sequential32 of the UNCLAMPED rows plus sequential32 of max(thr - lm, 0), added once."""
    base = sequential32(lm, D)
    if top_db is None:
        return base
    thr = clip_max32(lm) - np.float32(top_db)
    return base + sequential32(np.maximum(thr[:, None, None] - lm, np.float32(0.0)), D)


def host_mfccs(cfg, n):
    """The two float32 pipelines' MFCC [B, n_mfcc, T] of the case clips at one length: (a), (b)."""
    x = clamp32(host_logmel(cfg, n), top_db_of(cfg))
    return fftpack32(x, cfg["n_mfcc"]), sequential32(x, dct64(int(cfg["n_mels"]), int(cfg["n_mfcc"])))


@functools.lru_cache(maxsize=None)
def _c_ref(k):
    cfg = dict(k)
    c = np.zeros(int(cfg["n_mfcc"]))
    for n in frame_lengths(cfg):
        ref = reference(cfg, n)
        for got in host_mfccs(cfg, n):
            c = np.maximum(c, mfcc_error(got, ref).max(axis=(0, 1)))
    c.setflags(write=False)
    return c


def c_ref(cfg):
    """C_ref[k], k < n_mfcc: the largest c_M the two float32 host pipelines reach at index k over stage_oracle.cases(n, cfg),
    n in frame_lengths(cfg)."""
    return _c_ref(S.key(cfg))


def bounds(cfg, margin=None):
    return (MARGIN if margin is None else margin) * np.maximum(c_ref(cfg), 1.0)


# ---- the case set -----------------------------------------------------------------------------------------------------------

def clamp_census(ref):
    """(clamps [B], mixed [B]): whether a clip has an element that is clamped beyond doubt (L + dL < thr - d_thr), and
    whether one of its frames has such a filter beside one that is beyond doubt not clamped (L - dL > thr + d_thr)."""
    under = ref.L + ref.dL < ref.thr - ref.d_thr
    over = ref.L - ref.dL > ref.thr + ref.d_thr
    return under.any(axis=(1, 2)), (under.any(-1) & over.any(-1)).any(-1)


def check_case_set(cfg):
    """What the tests rely on, at the longest length (257 frames) for the clamp census and at every length for the two
    single clips: at top_db 80 at least five clips clamp and at least three have a frame with clamped and unclamped filters;
    at top_db 40 the AM clip and the step clip have one too; the impulse at n - 1 has its clip maximum in the LAST frame
    (and nowhere before it); the all-zero clip lies wholly on the amin floor and does not clamp."""
    n = frame_lengths(cfg)[-1]
    clamps, mixed = clamp_census(reference(dict(cfg, top_db=80.0), n))
    assert clamps.sum() >= 5 and mixed.sum() >= 3, (clamps.tolist(), mixed.tolist())
    _, mixed40 = clamp_census(reference(dict(cfg, top_db=40.0), n))
    assert mixed40[S.ROW_AM] and mixed40[S.ROW_STEP], mixed40.tolist()
    floor_db = 10.0 * np.log10(float(cfg.get("amin", 1e-10)))
    for n in frame_lengths(cfg):
        for top_db in (80.0, 40.0):
            ref = reference(dict(cfg, top_db=top_db), n)
            Li = ref.L[S.ROW_IMP_LAST]
            assert Li[-1].max() == Li.max() and (Li.shape[0] == 1 or Li[:-1].max() < Li.max()), n
            assert (ref.L[S.ROW_ZERO] == floor_db).all() and not clamp_census(ref)[0][S.ROW_ZERO], n
