"""CPU: the yardstick of the Welch cross spectrum and coherence (tests/modcsd_oracle.py) on every parameter set the GPU
tests use -- its float32 pipeline inside its own bound, no pair and no bin without a finite measure -- and what it must
catch; the third header's symbols exported, bound and prototyped; mm_modcsd_check; the Python refusals that need no device;
the y shape / group arithmetic."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import modcsd_oracle as O
import modpsd_oracle as P
from conftest import ROOT
from modulation_mfcc_amd import _lib, modcsd, modpsd

HEADER = os.path.join(ROOT, "include", "modmfcc_modcsd.h")


# ---- the yardstick on the GPU tests' parameter sets -------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(O.N_GPU_SETS), ids=O.GPU_SET_IDS)
def test_the_float32_pipeline_stays_within_its_own_bound_and_no_bin_is_excluded(i):
    p, T = O.gpu_set(i)
    x, y = O.pairs_for(p, T)
    assert x.shape == y.shape == (64, T) and x.dtype == y.dtype == np.float32
    pxx, pyy, pxy, coh = O.spectra32(x, y, p)
    c1, c2 = O.check_pxy(pxy, x, y, p, "spectra32")
    assert c1 == O.c_ref(p, T) and c2 == O.c_ref(p, T, True)
    # the second-order measure binds on every set, at every pair and bin: finite, and of the size of the PSD yardstick's
    c = O.cross_error2(pxy, x, y, p)
    assert c.shape == (64, p.bins) and np.isfinite(c).all() and c2 < 8, (O.GPU_SET_IDS[i], c2)
    # an exact 0 is due (denominator 0) only where a side puts nothing but zeros into the transform and has no trend (the
    # zero row; the impulse behind the last segment, or under a zero of the taper without a detrend): its row norm is 0
    zero_side = ((O.row_norm(x, p) == 0) | (O.row_norm(y, p) == 0))[:, 0]
    assert zero_side[48:].all() and zero_side[15] and not zero_side[:7].any()
    assert ((O.denominators(x, y, p)[1] == 0).any(axis=1) == zero_side).all() and (pxy[zero_side] == 0).all()
    # the auto spectra of both sides pass modpsd_oracle.check as it stands; scipy passes both measures with c = 0
    P.check(pxx, x, p, "spectra32 Pxx")
    P.check(pyy, y, p, "spectra32 Pyy")
    assert O.check_pxy(O.csd64(x, y, p)[1], x, y, p, "csd64") == (0.0, 0.0)
    # the coherence of the zero-row pairs is scipy's NaN, that of a row with itself 1 wherever the row has power
    ref = O.coherence64(x, y, p)[1]
    assert np.isnan(ref[48:]).all() and (np.isnan(coh) == ~(pxx * pyy > 0)).all()


def test_the_first_order_measure_alone_binds_nothing_on_some_sets():
    """Why check_pxy checks twice (the oracle's module text): bin 0 behind a constant detrend under a boxcar window has
    Ax = Ay = 0 exactly, the float32 pipeline does not."""
    p, T = O.gpu_set(10)
    assert p.window_arg == "boxcar" and p.detrend == "constant"
    assert O.c_ref(p, T) == np.inf and O.c_ref(p, T, True) < 8


def _small():
    p, T = O.gpu_set(5)                           # 64 in 64, no overlap, 32 segments
    return (p, T) + O.pairs_for(p, T)


def test_it_catches_a_conjugate_on_the_wrong_side():
    p, T, x, y = _small()
    with pytest.raises(AssertionError, match="beyond c"):
        O.check_pxy(np.conj(O.csd64(x, y, p)[1]), x, y, p)


def test_it_catches_a_missing_one_sided_factor_and_a_swapped_scaling():
    p, T, x, y = _small()
    got = O.csd64(x, y, p)[1].copy()
    got[:, 1:-1] /= 2
    with pytest.raises(AssertionError, match="beyond c"):
        O.check_pxy(got, x, y, p)
    q = O.Params(O.FS, "hann", 64, 0, 64, False, "density")
    with pytest.raises(AssertionError, match="beyond c"):
        O.check_pxy(O.csd64(x, y, q)[1], x, y, p)


def test_it_catches_a_dropped_segment_a_nan_and_a_nonzero_for_the_zero_row():
    p, T, x, y = _small()
    with pytest.raises(AssertionError, match="beyond c"):
        O.check_pxy(O.csd64(x[:, :T - p.step], y[:, :T - p.step], p)[1], x, y, p)
    got = O.csd64(x, y, p)[1].copy()
    got[2, 5] = np.nan
    with pytest.raises(AssertionError, match="beyond c"):
        O.check_pxy(got, x, y, p)
    got = O.csd64(x, y, p)[1].copy()
    got[50, 3] = 1e-30j                           # a pair with the zero row: exact zeros
    with pytest.raises(AssertionError, match="beyond c"):
        O.check_pxy(got, x, y, p)


def test_it_catches_a_float32_mean_of_products():
    """conj(X) Y of every segment added to ONE complex64 accumulator in turn: at 2000 segments the constant row against
    itself (every term the same) is far outside; the same products averaged in float64 pass."""
    p = O.Params(O.FS, "boxcar", 64, 0, 64, False, "density")
    r = O.rows_for(p, 64 * 2000)
    x, y = r[[3, 0]], r[[3, 1]]
    X, Y = O._transform32(x, p), O._transform32(y, p)
    prod = (np.conj(X) * Y).astype(np.complex64)
    running = np.add.accumulate(prod, axis=1, dtype=np.complex64)[:, -1].astype(np.complex128) / 2000 * (p.s * p.d)
    tol = O.MARGIN * 1.0                          # (C_ref on the 64 pairs of 128 000 samples: not needed to see c > 100)
    assert O.cross_error2(running, x, y, p).max() > 25 * tol
    assert O.cross_error2(prod.astype(np.complex128).mean(axis=1) * (p.s * p.d), x, y, p).max() <= tol


def test_the_coherence_pairs_carry_power_in_every_bin():
    for i in O.COH_SETS:
        p, T = O.gpu_set(i)
        x, y = O.coherence_pairs(T)
        ref = O.coherence64(x, y, p)[1]
        assert np.isfinite(ref).all() and ref.min() >= 0 and ref.max() <= 1 + 1e-12
        e = O.coherence_ref_error(x, y, p)
        assert np.isfinite(e) and e < 1e-5, (O.GPU_SET_IDS[i], e)
        sd = p.s * p.d
        for side in (x, y):                       # power: no bin below a millionth of the row's mean bin
            A2 = P.welch64(side, p)[1] / sd
            assert (A2 > 1e-6 * A2.mean(axis=1, keepdims=True)).all(), O.GPU_SET_IDS[i]


def test_the_list_covers_what_it_has_to():
    s = O._GPU_SETS
    assert {32, 64, 128, 1024, 2048} <= {e[1] for e in s}
    assert {(31, 32), (255, 256), (1200, 2048)} <= {(e[0], e[1]) for e in s}
    assert {1, 4, 5, 32, 33, 65} <= {e[3] for e in s}
    assert {False, "constant", "linear"} == {e[4] for e in s} and {"density", "spectrum"} == {e[5] for e in s}
    assert "array" in {e[6] for e in s}
    assert {0, None} <= {e[2] for e in s} and {(32, 31), (64, 63)} <= {(e[0], e[2]) for e in s}
    assert len(O.COH_SETS) == O.N_GPU_SETS - 2


# ---- the third header ---------------------------------------------------------------------------------------------------------
def _prototypes():
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return {m.group(1): m.group(2) for m in re.finditer(r"\b(mm_[a-z0-9_]+)\s*\(([^)]*)\)", txt)}


def test_every_symbol_of_the_third_header_is_exported_and_bound():
    lib = _lib.load()
    protos = _prototypes()
    assert set(protos) == set(_lib.PROTOTYPES_MODCSD) and len(protos) == 4, set(protos) ^ set(_lib.PROTOTYPES_MODCSD)
    assert not set(protos) & (set(_lib.PROTOTYPES) | set(_lib.PROTOTYPES_MODPSD))
    assert len(_lib.PROTOTYPES_MODPSD) == 7
    taking_stream = []
    for name, params in protos.items():
        assert hasattr(lib, name), f"{name} declared in include/modmfcc_modcsd.h but not exported"
        res, args = _lib.PROTOTYPES_MODCSD[name]
        n_params = 0 if params.strip() in ("", "void") else params.count(",") + 1
        assert len(args) == n_params, (name, params, args)
        assert getattr(lib, name).argtypes == args and getattr(lib, name).restype is res
        if re.search(r"void\s*\*\s*stream\s*$", params):
            taking_stream.append(name)
            assert args[-1] is C.c_void_p and res is C.c_int, name
    assert taking_stream == ["mm_modcsd_f32"]
    assert lib.mm_modcsd_version() == 1 and lib.mm_modpsd_version() == 1 and lib.mm_version() == 123
    assert '#include "modmfcc_modpsd.h"' in open(HEADER).read()


def test_the_unit_is_in_both_builds():
    csrc = os.path.join(ROOT, "modulation_mfcc_amd", "csrc")
    mk = open(os.path.join(csrc, "Makefile")).read()
    assert re.search(r"^TUS\s*:=.*\bmm_modcsd\b", mk, flags=re.M) and re.search(r"^HDRS\s*:=.*modmfcc_modcsd\.h", mk, flags=re.M)
    assert '#include "mm_modcsd.hip"' in open(os.path.join(csrc, "mm_unity.hip")).read()


def _params(**kw):
    d = dict(fs=200.0, nperseg=256, noverlap=128, nfft=256, detrend=1, scaling=0)
    d.update(kw)
    return _lib.mm_modpsd_params(d["fs"], d["nperseg"], d["noverlap"], d["nfft"], d["detrend"], d["scaling"])


@pytest.mark.parametrize("bad,status", [
    (dict(), 0), (dict(nperseg=1, noverlap=0, nfft=32), 0), (dict(nperseg=1200, noverlap=600, nfft=2048), 0),
    (dict(nperseg=2048, noverlap=2047, nfft=2048), 0),
    (dict(nperseg=0), -1), (dict(noverlap=-1), -1), (dict(noverlap=256), -1), (dict(nfft=128), -1), (dict(detrend=3), -1),
    (dict(scaling=2), -1), (dict(fs=0.0), -1), (dict(fs=float("nan")), -1),
    (dict(nfft=4096), -2), (dict(nperseg=4096, noverlap=0, nfft=4096), -2), (dict(nfft=300), -2), (dict(nfft=8192), -2),
    (dict(nperseg=8, noverlap=4, nfft=16), -2),
])
def test_check(bad, status):
    lib = _lib.load()
    assert (_lib.MM_ERR_INVALID_ARG, _lib.MM_ERR_UNSUPPORTED) == (-1, -2)
    assert lib.mm_modcsd_check(C.byref(_params(**bad))) == status
    if bad.get("nfft") == 4096:
        assert lib.mm_modpsd_check(C.byref(_params(**bad))) == 0      # the second header keeps its 4096
    assert lib.mm_modcsd_check(None) == -1


def test_the_entry_refuses_before_it_touches_the_device():
    lib = _lib.load()
    assert lib.mm_modcsd_workspace_bytes(None, 4, 1000) == 0
    assert lib.mm_modcsd_f32(None, None, 1, 1000, 1000, None, 1000, 1, None, None, None, None, None, 129, None, 0, None) == -1


# ---- Python, without a device ---------------------------------------------------------------------------------------------------
def test_the_names_are_exported():
    import modulation_mfcc_amd as M
    for name in ("modulation_cross_spectra_batch", "modulation_csd_batch", "modulation_coherence_batch",
                 "modulation_cross_spectra_ragged_batch", "modulation_csd_ragged_batch", "modulation_coherence_ragged_batch"):
        assert getattr(M, name) is getattr(modcsd, name) and name in modcsd.__all__
    assert callable(M.mfcc_modcsd_batch) and callable(M.mfcc_modcsd_ragged_batch) and callable(M.MfccPlan.mfcc_modcsd)
    import inspect
    assert "scaling" not in inspect.signature(modcsd.modulation_coherence_batch).parameters
    assert "scaling" not in inspect.signature(modcsd.modulation_coherence_ragged_batch).parameters
    assert "scaling" in inspect.signature(modcsd.modulation_csd_batch).parameters


@pytest.mark.parametrize("kw,exc,text", [
    (dict(nfft=4096), NotImplementedError, r"nfft = 4096 .*\[32, 2048\]"),
    (dict(nperseg=2049, nfft=None), NotImplementedError, r"nfft = 4096 .*\[32, 2048\]"),
    (dict(nfft=300), NotImplementedError, "nfft = 300"),
    (dict(nperseg=5000, nfft=None), NotImplementedError, "nfft = 8192"),
    (dict(noverlap=256), ValueError, "noverlap must be less than nperseg"),
    (dict(nfft=128), ValueError, "nfft must be greater than or equal to nperseg"),
    (dict(nperseg=0), ValueError, "nperseg must be a positive integer"),
    (dict(window=np.ones(100)), ValueError, "different from length of window"),
    (dict(window=np.zeros(256)), ValueError, "window sums to zero"),
    (dict(detrend="quadratic"), ValueError, "detrend"),
    (dict(scaling="psd"), ValueError, "Unknown scaling"),
    (dict(fs=0.0), ValueError, "fs"),
])
def test_python_validation(kw, exc, text):
    args = dict(fs=200.0, window="hann", nperseg=256, noverlap=None, nfft=None, detrend="constant", scaling="density")
    args.update(kw)
    with pytest.raises(exc, match=text):
        modcsd._spec(**args)


def test_the_defaults_are_those_of_modpsd():
    s, q = modcsd._spec(200.0, "hann", 100, None, None, "constant", "density"), modpsd._Spec(200.0, "hann", 100, None, None,
                                                                                             "constant", "density")
    assert s.key == q.key and (s.nperseg, s.noverlap, s.nfft, s.bins) == (100, 50, 128, 65)
    assert modcsd._spec(1.0, "boxcar", 2048, 0, None, False, "spectrum").nfft == 2048


def test_host_and_float64_input_raise_type_errors():
    import torch
    for x in (np.zeros((2, 600), np.float32), torch.zeros(2, 600), torch.zeros(2, 600, dtype=torch.float64)):
        for f in (modcsd.modulation_cross_spectra_batch, modcsd.modulation_csd_batch, modcsd.modulation_coherence_batch):
            with pytest.raises(TypeError, match="float32 CUDA"):
                f(x, x, 200.0)
        for f in (modcsd.modulation_cross_spectra_ragged_batch, modcsd.modulation_csd_ragged_batch,
                  modcsd.modulation_coherence_ragged_batch):
            with pytest.raises(TypeError, match="float32 CUDA"):
                f(x, x, [600, 300], 200.0)


def test_y_group_arithmetic():
    assert modcsd.y_group(26, 26) == 1 and modcsd.y_group(26, 2) == 13 and modcsd.y_group(26, 1) == 26
    assert modcsd.y_group(1, 1) == 1 and modcsd.y_group(0, 0) == 1
    for x_rows, y_rows in ((26, 4), (26, 27), (26, 52), (26, 0), (1, 2)):
        with pytest.raises(ValueError, match="divisor"):
            modcsd.y_group(x_rows, y_rows)
