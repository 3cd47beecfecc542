"""CPU: the yardstick of the Welch modulation power spectrum (tests/modpsd_oracle.py) catches what it must and is finite
where it has to be; the second header's symbols are exported and bound; the host-side segment count and parameter checks."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import scipy.signal
from scipy import fft as sfft

import modpsd_oracle as O
from conftest import ROOT
from modulation_mfcc_amd import _lib, modpsd

HEADER = os.path.join(ROOT, "include", "modmfcc_modpsd.h")


def _prototypes():
    """name -> parameter text of every mm_*( prototype of the second header (comments removed)."""
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return {m.group(1): m.group(2) for m in re.finditer(r"\b(mm_[a-z0-9_]+)\s*\(([^)]*)\)", txt)}


# ---- the yardstick ----------------------------------------------------------------------------------------------------------
def _case(T=2 * 64 + 7, **kw):
    p = O.Params(200.0, **dict(dict(window="hann", nperseg=64, noverlap=32, nfft=64), **kw))
    return p, O.rows_for(p, T)


def test_the_reference_passes_its_own_bound():
    for kw in (dict(), dict(detrend="linear", scaling="spectrum"), dict(window="boxcar", detrend=False, noverlap=0),
               dict(nperseg=100, nfft=128, noverlap=99)):
        p, x = _case(**kw)
        assert O.check(O.psd32(x, p), x, p, "psd32") <= O.tolerance(p, x.shape[1])
        assert O.check(O.welch64(x, p)[1], x, p, "welch64") == 0.0


def test_it_catches_a_missing_one_sided_factor():
    p, x = _case()
    got = O.welch64(x, p)[1].copy()
    got[:, 1:-1] /= 2
    with pytest.raises(AssertionError, match="beyond c"):
        O.check(got, x, p)


def test_it_catches_a_dropped_segment():
    p, x = _case(T=64 + 32 * 9)                 # ten segments: the mean over the first nine
    K = p.num_segments(x.shape[1])
    assert K == 10
    got = O.welch64(x[:, :x.shape[1] - p.step], p)[1]
    with pytest.raises(AssertionError, match="beyond c"):
        O.check(got, x, p)


def test_it_catches_a_swapped_scaling():
    p, x = _case()
    q = O.Params(200.0, "hann", 64, 32, 64, "constant", "spectrum")
    with pytest.raises(AssertionError, match="beyond c"):
        O.check(O.welch64(x, q)[1], x, p)


def test_it_catches_a_negative_power_and_a_nan():
    p, x = _case()
    got = O.welch64(x, p)[1].copy()
    got[2, 5] = -got[2, 5]
    with pytest.raises(AssertionError, match="negative power"):
        O.check(got, x, p)
    got = O.welch64(x, p)[1].copy()
    got[2, 5] = np.nan
    with pytest.raises(AssertionError, match="beyond c"):
        O.check(got, x, p)
    got = O.welch64(x, p)[1].copy()
    got[O.ROW_ZERO, 3] = 1e-30              # the zero row must come back as zeros
    with pytest.raises(AssertionError, match="beyond c"):
        O.check(got, x, p)


def test_it_catches_a_float32_running_sum_over_2000_segments():
    """|X|^2 of every segment added to ONE float32 accumulator in turn: the constant row (every term the same) loses
    c ~ 130 at 2000 segments; the same float32 powers averaged in float64 pass."""
    p = O.Params(200.0, "boxcar", 64, 0, 64, False, "density")
    x = O.rows_for(p, 64 * 2000)
    seg = O.segments(x, p)
    X = sfft.rfft(seg.astype(np.float32) * p.w, n=p.nfft, axis=-1)
    pw = (X.real ** 2 + X.imag ** 2).astype(np.float32)
    assert pw.shape[1] == 2000
    running = np.add.accumulate(pw, axis=1, dtype=np.float32)[:, -1].astype(np.float64) / 2000 * (p.s * p.d)
    with pytest.raises(AssertionError, match="beyond c"):
        O.check(running, x, p)
    O.check(pw.astype(np.float64).mean(axis=1) * (p.s * p.d), x, p, "float64 mean of float32 powers")


@pytest.mark.parametrize("nperseg,nfft", [(64, 64), (100, 128), (512, 512), (1000, 1024)])
@pytest.mark.parametrize("window", ["hann", "boxcar", "flattop", ("kaiser", 7.4)])
def test_the_measure_is_finite(nperseg, nfft, window):
    """Every row of the case set -- the impulse at sample 0 under a zero of the taper and the mean-1e4 trajectory among
    them -- has a finite measure for the float32 reference, for the three detrends, at no, half and full-but-one overlap,
    at one segment and at 2 nperseg + 7 samples.  (nperseg 2048 / 2048 and 3000 / 4096 gave finite values too: up to 5.8,
    minutes of host time at hop 1, not repeated here.)"""
    for noverlap in (0, nperseg // 2, nperseg - 1):
        for detrend in (False, "constant", "linear"):
            for T in (nperseg, 2 * nperseg + 7):
                if noverlap == nperseg - 1 and T > nperseg and nperseg > 512:
                    continue                    # (a thousand segments of a thousand points per row: the smaller sizes cover hop 1)
                p = O.Params(200.0, window, nperseg, noverlap, nfft, detrend, "density")
                c = O.c_ref(p, T)
                assert np.isfinite(c) and c < 16, (nperseg, nfft, window, noverlap, detrend, T, c)


def test_parseval_of_the_reference():
    """Boxcar, no detrend, no overlap, 'density', nfft = nperseg: sum P df = mean x^2 over the samples the segments use."""
    p = O.Params(200.0, "boxcar", 64, 0, 64, False, "density")
    x = O.rows_for(p, 64 * 5 + 9)
    f, P = O.welch64(x, p)
    used = x[:, :64 * 5].astype(np.float64)
    np.testing.assert_allclose(P.sum(axis=1) * (f[1] - f[0]), (used ** 2).mean(axis=1), rtol=1e-12, atol=0)


# ---- the second header ------------------------------------------------------------------------------------------------------
def test_every_symbol_of_the_second_header_is_exported_and_bound():
    lib = _lib.load()
    protos = _prototypes()
    assert set(protos) == set(_lib.PROTOTYPES_MODPSD) and len(protos) == 7, set(protos) ^ set(_lib.PROTOTYPES_MODPSD)
    assert not set(protos) & set(_lib.PROTOTYPES)
    taking_stream = []
    for name, params in protos.items():
        assert hasattr(lib, name), f"{name} declared in include/modmfcc_modpsd.h but not exported"
        res, args = _lib.PROTOTYPES_MODPSD[name]
        n_params = 0 if params.strip() in ("", "void") else params.count(",") + 1
        assert len(args) == n_params, (name, params, args)
        if re.search(r"void\s*\*\s*stream\s*$", params):
            taking_stream.append(name)
            assert args[-1] is C.c_void_p and res is C.c_int, name
    assert taking_stream == ["mm_modpsd_f32"]
    assert lib.mm_modpsd_version() == 1
    assert lib.mm_version() == 123              # the first header's version does not move


def test_the_params_struct_matches_the_header():
    assert C.sizeof(_lib.mm_modpsd_params) == 8 + 8 * 4
    assert [f[0] for f in _lib.mm_modpsd_params._fields_] == ["fs", "nperseg", "noverlap", "nfft", "detrend", "scaling", "reserved"]
    txt = open(HEADER).read()
    assert re.search(r"double fs;\s*int32_t nperseg, noverlap, nfft;\s*int32_t detrend;[^;]*\s*int32_t scaling;[^;]*\s*"
                     r"int32_t reserved\[3\];", txt)
    assert f"#define MM_MODPSD_CHUNK {32}" in txt


def _params(**kw):
    d = dict(fs=200.0, nperseg=256, noverlap=128, nfft=256, detrend=1, scaling=0)
    d.update(kw)
    return _lib.mm_modpsd_params(d["fs"], d["nperseg"], d["noverlap"], d["nfft"], d["detrend"], d["scaling"])


def test_num_segments_equals_scipys_count():
    lib = _lib.load()
    x = np.random.default_rng(0).standard_normal(700)
    for nperseg in (1, 2, 7, 32, 100, 256):
        for noverlap in sorted({0, 1, nperseg // 2, nperseg - 1} - {nperseg}):
            if noverlap >= nperseg:
                continue
            p = _params(nperseg=nperseg, noverlap=noverlap, nfft=256)
            for n in sorted({nperseg, nperseg + 1, 2 * nperseg - noverlap - 1, 2 * nperseg - noverlap, 3 * nperseg + 5, 699, 700}):
                if n < nperseg or n > 700:
                    continue
                _, t, _ = scipy.signal.spectrogram(x[:n], nperseg=nperseg, noverlap=noverlap, window="boxcar")
                assert lib.mm_modpsd_num_segments(C.byref(p), n) == len(t) == modpsd.modpsd_segments(n, nperseg, noverlap), \
                    (n, nperseg, noverlap)
            for n in (0, nperseg - 1):
                assert lib.mm_modpsd_num_segments(C.byref(p), n) == 0 == modpsd.modpsd_segments(n, nperseg, noverlap)
    assert lib.mm_modpsd_num_segments(C.byref(_params()), -1) == _lib.MM_ERR_INVALID_ARG
    assert lib.mm_modpsd_num_segments(C.byref(_params(noverlap=256)), 1000) == _lib.MM_ERR_INVALID_ARG
    assert (modpsd.modpsd_segments(np.array([255, 256, 383, 384, 1001])) == [0, 1, 1, 2, 6]).all()


@pytest.mark.parametrize("bad,status", [
    (dict(nperseg=0), -1), (dict(noverlap=-1), -1), (dict(noverlap=256), -1), (dict(nfft=128), -1), (dict(detrend=3), -1),
    (dict(detrend=-1), -1), (dict(scaling=2), -1), (dict(fs=0.0), -1), (dict(fs=float("nan")), -1), (dict(fs=float("inf")), -1),
    (dict(nfft=300), -2), (dict(nfft=8192), -2), (dict(nperseg=8, noverlap=4, nfft=16), -2), (dict(nfft=4096), 0),
    (dict(nperseg=1, noverlap=0, nfft=32), 0), (dict(nperseg=100, noverlap=99, nfft=128), 0),
])
def test_check_rejects(bad, status):
    lib = _lib.load()
    assert lib.mm_modpsd_check(C.byref(_params(**bad))) == status
    h = C.c_void_p()
    if status:
        w = np.ones(4096, np.float32)
        assert lib.mm_modpsd_create(C.byref(_params(**bad)), w.ctypes.data, C.byref(h)) == status and not h
    assert lib.mm_modpsd_check(None) == -1


def test_create_rejects_a_window_without_scale_before_it_touches_the_device():
    lib = _lib.load()
    h = C.c_void_p()
    zero, odd = np.zeros(256, np.float32), np.tile(np.array([1, -1], np.float32), 128)
    bad = np.ones(256, np.float32)
    bad[7] = np.nan
    assert lib.mm_modpsd_create(C.byref(_params()), zero.ctypes.data, C.byref(h)) == -1
    assert lib.mm_modpsd_create(C.byref(_params(scaling=1)), odd.ctypes.data, C.byref(h)) == -1       # sum w = 0
    assert lib.mm_modpsd_create(C.byref(_params()), bad.ctypes.data, C.byref(h)) == -1
    assert lib.mm_modpsd_create(C.byref(_params()), None, C.byref(h)) == -1
    assert lib.mm_modpsd_create(C.byref(_params()), zero.ctypes.data, None) == -1
    assert not h
    assert lib.mm_modpsd_workspace_bytes(None, 4, 1000) == 0
    assert lib.mm_modpsd_f32(None, None, 1, 1000, 1000, None, None, 129, None, 0, None) == -1
    lib.mm_modpsd_destroy(None)


@pytest.mark.parametrize("kw,exc,text", [
    (dict(noverlap=256), ValueError, "noverlap must be less than nperseg"),
    (dict(noverlap=300), ValueError, "noverlap must be less than nperseg"),
    (dict(noverlap=-1), ValueError, "nonnegative"),
    (dict(nfft=128), ValueError, "nfft must be greater than or equal to nperseg"),
    (dict(nperseg=0), ValueError, "nperseg must be a positive integer"),
    (dict(window=np.ones(100)), ValueError, "different from length of window"),
    (dict(window=np.ones((2, 128))), ValueError, "window must be 1-D"),
    (dict(window=np.zeros(256)), ValueError, "window sums to zero"),
    (dict(window=np.tile([1.0, -1.0], 128), scaling="spectrum"), ValueError, "window sums to zero"),
    (dict(window="no-such-window"), ValueError, "Unknown window"),
    (dict(detrend="quadratic"), ValueError, "detrend"),
    (dict(detrend=True), ValueError, "detrend"),
    (dict(scaling="psd"), ValueError, "Unknown scaling"),
    (dict(fs=0.0), ValueError, "fs"),
    (dict(nfft=300), NotImplementedError, "nfft = 300"),
    (dict(nperseg=5000, nfft=None), NotImplementedError, "nfft = 8192"),
])
def test_python_validation(kw, exc, text):
    args = dict(fs=200.0, window="hann", nperseg=256, noverlap=None, nfft=None, detrend="constant", scaling="density")
    args.update(kw)
    with pytest.raises(exc, match=text):
        modpsd._Spec(**args)


def test_python_defaults_follow_scipy_but_for_nfft():
    s = modpsd._Spec(200.0, "hann", 256, None, None, "constant", "density")
    assert (s.nperseg, s.noverlap, s.nfft, s.bins) == (256, 128, 256, 129)
    assert s.window.dtype == np.float32 and (s.window == scipy.signal.get_window("hann", 256).astype(np.float32)).all()
    np.testing.assert_array_equal(s.freqs(), np.fft.rfftfreq(256, 1 / 200.0))
    for nperseg, nfft in ((1, 32), (32, 32), (33, 64), (100, 128), (1000, 1024), (2049, 4096), (4096, 4096)):
        assert modpsd.modpsd_nfft(nperseg) == nfft == modpsd._Spec(1.0, "boxcar", nperseg, 0, None, False, "spectrum").nfft
    f, _ = O.welch64(np.zeros((1, 300), np.float32), O.Params(200.0, "hann", 100, None, 128))
    np.testing.assert_array_equal(modpsd._Spec(200.0, "hann", 100, None, None, "constant", "density").freqs(), f)


def test_host_and_float64_input_raise_type_errors():
    import torch
    import modulation_mfcc_amd as M
    assert M.modulation_psd_batch is modpsd.modulation_psd_batch and M.modulation_psd_ragged_batch is modpsd.modulation_psd_ragged_batch
    assert "modulation_psd_batch" in modpsd.__all__ and callable(M.mfcc_modpsd_batch) and callable(M.mfcc_modpsd_ragged_batch)
    for x in (np.zeros((2, 600), np.float32), torch.zeros(2, 600), torch.zeros(2, 600, dtype=torch.float64)):
        with pytest.raises(TypeError):
            modpsd.modulation_psd_batch(x, 200.0)
        with pytest.raises(TypeError):
            modpsd.modulation_psd_ragged_batch(x, [600, 300], 200.0)


def test_the_unit_is_in_both_builds():
    csrc = os.path.join(ROOT, "modulation_mfcc_amd", "csrc")
    assert re.search(r"^TUS\s*:=.*\bmm_modpsd\b", open(os.path.join(csrc, "Makefile")).read(), flags=re.M)
    assert '#include "mm_modpsd.hip"' in open(os.path.join(csrc, "mm_unity.hip")).read()
