"""CPU: the long FIR / Savitzky-Golay filters without a device -- the long-double oracle (tests/longfilt_oracle.py) pinned
against scipy where scipy is itself accurate, the host table builders against the oracle, the exported symbols and the
argument checks that answer before any launch.  The figure is 1e-12 of the curve's maximum throughout, the one
test_fir_filtfilt_stencil_on_the_host uses."""
import os
import re

import numpy as np
import pytest
import scipy.signal

import longfilt_oracle as Q
from conftest import ROOT
from modulation_mfcc_amd import _lib, filters

TOL = 1e-12


def _fir(L, kind="lowpass"):
    cut = [0.1, 0.4] if kind == "bandpass" else 0.24
    return scipy.signal.firwin(L, cut, window=("kaiser", 7.4), pass_zero=kind)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("L", [2, 6, 9, 21])
def test_fir_oracle_is_scipy_filtfilt(L, dtype):
    rng = np.random.default_rng(L)
    for n in (3 * L + 1, 3 * L + 2, 500):
        x = Q.curve_rows(rng, 3, n, dtype)
        for taps in (_fir(L), _fir(L, "highpass") if L % 2 else rng.standard_normal(L)):
            want = scipy.signal.filtfilt(taps, 1, x)
            got = Q.fir_filtfilt_ext_ld(taps, x)
            assert want.dtype == np.float64 and got.shape == want.shape
            assert Q.rel_err(want, got) <= TOL, (L, n, Q.rel_err(want, got))
    with pytest.raises(ValueError, match=f"greater than padlen, which is {3 * L}"):
        Q.fir_filtfilt_ext_ld(_fir(L), np.zeros(3 * L))
    one = Q.curve_rows(rng, 1, 400, dtype)[0]             # a 1-D curve
    assert Q.rel_err(scipy.signal.filtfilt(_fir(L), 1, one), Q.fir_filtfilt_ext_ld(_fir(L), one)) <= TOL


def test_fir_oracle_extends_a_float32_curve_in_float32():
    """The extension of a float32 curve is rounded to float32 (scipy's odd_ext runs before lfilter upcasts): against
    scipy on the same curve widened first, the oracle differs at the float32 level -- the third tooth of the GPU test."""
    x = Q.curve_rows(np.random.default_rng(0), 1, 300, np.float32)
    got = Q.fir_filtfilt_ext_ld(_fir(21), x)
    assert Q.rel_err(scipy.signal.filtfilt(_fir(21), 1, x), got) <= TOL
    assert Q.rel_err(scipy.signal.filtfilt(_fir(21), 1, x.astype(np.float64)), got) > 1e-11


@pytest.mark.parametrize("deriv", [0, 1, 2])
@pytest.mark.parametrize("p", [2, 3])
@pytest.mark.parametrize("W", [5, 6, 16, 17, 18, 21])
def test_savgol_oracle_is_scipy_savgol_filter(W, p, deriv):
    """Odd AND even windows: an even window's taps sit on x[i - (W - 1) // 2 .. i + W // 2] (calc.velocity_stencil)."""
    rng = np.random.default_rng(100 * W + 10 * p + deriv)
    for n, delta in ((W, 1.0), (W + 1, 0.005), (200, 0.005)):
        x = Q.curve_rows(rng, 2, n)
        want = scipy.signal.savgol_filter(x, W, p, deriv=deriv, delta=delta, mode="interp")
        got = Q.savgol_ext_ld(x, W, p, deriv, delta)
        assert Q.rel_err(want, got) <= TOL, (n, Q.rel_err(want, got))
    w = Q.savgol_weights_ld(W, p, deriv, 0.005, [(W - 1) / 2.0])[0].astype(np.float64)
    taps = scipy.signal.savgol_coeffs(W, p, deriv=deriv, delta=0.005)[::-1]
    assert np.abs(w - taps).max() <= TOL * np.abs(taps).max()
    with pytest.raises(ValueError, match="window_length must be less than or equal to the size of x"):
        Q.savgol_ext_ld(np.zeros(W - 1), W, p, deriv)
    with pytest.raises(ValueError, match="polyorder must be less than window_length"):
        Q.savgol_weights_ld(3, 3, 0, 1.0, [1.0])


def test_savgol_oracle_float32_and_low_orders():
    rng = np.random.default_rng(5)
    x = Q.curve_rows(rng, 2, 120, np.float32)
    want = scipy.signal.savgol_filter(x, 21, 3, mode="interp")
    assert want.dtype == np.float32
    assert Q.rel_err(want, Q.savgol_ext_ld(x, 21, 3)) <= 2.0 ** -23        # scipy's single rounding to float32
    for p in (0, 1):
        y = Q.curve_rows(rng, 1, 90)
        assert Q.rel_err(scipy.signal.savgol_filter(y, 18, p, mode="interp"), Q.savgol_ext_ld(y, 18, p)) <= TOL
    y = Q.curve_rows(rng, 1, 50)
    assert np.abs(Q.savgol_ext_ld(y, 9, 2, deriv=3)).max() == 0            # deriv > polyorder: scipy returns zeros too
    assert np.abs(scipy.signal.savgol_filter(y, 9, 2, deriv=3, mode="interp")).max() == 0


# ---------------------------------------------------------------------------------------------------------------------
# the package's side: symbols, constants, tables, checks
# ---------------------------------------------------------------------------------------------------------------------
def test_exported_symbols_and_constants():
    import modulation_mfcc_amd as M
    from modulation_mfcc_amd import calc
    assert M.fir_filtfilt_batch is filters.fir_filtfilt_batch and M.savgol_batch is filters.savgol_batch
    hdr = open(os.path.join(ROOT, "include", "modmfcc.h")).read()
    lib = _lib.load()
    for name in ("mm_fir_filtfilt_f64", "mm_fir_filtfilt_f32_f64", "mm_savgol_f64"):
        assert name in _lib.PROTOTYPES and hasattr(lib, name) and re.search(rf"\bint {name}\(", hdr), name
    assert lib.mm_version() == 123
    # the tile and chunk the GPU tests take their boundary lengths from are the kernel's
    src = open(os.path.join(ROOT, "modulation_mfcc_amd", "csrc", "mm_longfilt.hip")).read()
    k = {m.group(1): int(m.group(2)) for m in re.finditer(r"constexpr int (kLf\w+) = (\d+);", src)}
    assert filters.LONGFILT_TILE == k["kLfThreads"] * k["kLfPer"] == 2048
    assert filters.LONGFILT_CHUNK == k["kLfChunk"] == 128
    for unit in ("Makefile", "mm_unity.hip"):
        assert "mm_longfilt" in open(os.path.join(ROOT, "modulation_mfcc_amd", "csrc", unit)).read()
    # the short filters keep their limits: longer ones are NOT squeezed into the stencil
    with pytest.raises(NotImplementedError):
        filters.fir_filtfilt_stencil(np.ones(9) / 9)
    with pytest.raises(NotImplementedError):
        calc.velocity_stencil(200.0, 1, "sg", 17, 2, 3)


@pytest.mark.parametrize("L", [2, 9, 21, 101])
def test_fir_filtfilt_taps(L):
    b = _fir(L)
    h = filters.fir_filtfilt_taps(b)
    assert h.dtype == np.float64 and h.shape == (2 * L - 1,)
    assert np.abs(h - np.convolve(b, b[::-1])).max() <= 4 * np.finfo(np.float64).eps * np.abs(h).max()
    assert np.abs(h - h[::-1]).max() <= np.finfo(np.float64).eps * np.abs(h).max()
    # applied with numpy to the odd-extended curve: the oracle
    x = Q.curve_rows(np.random.default_rng(L), 2, 3 * L + 40)
    ext = Q.odd_ext(x, 3 * L)
    y = np.stack([np.correlate(r, h, "valid")[2 * L + 1:2 * L + 1 + x.shape[1]] for r in ext])
    assert Q.rel_err(y, Q.fir_filtfilt_ext_ld(b, x)) <= TOL


@pytest.mark.parametrize("W,p,deriv", [(5, 2, 0), (6, 3, 1), (16, 3, 2), (17, 2, 1), (18, 3, 2), (21, 3, 0), (64, 3, 1),
                                       (101, 5, 2), (257, 5, 2), (257, 2, 0), (9, 8, 1), (1, 0, 0), (2, 1, 1), (9, 2, 3)])
def test_savgol_tables_reproduce_the_oracle(W, p, deriv):
    """c, Q and P applied with numpy: interior c . x[i - (W - 1) // 2 ...], edges P (Q x[window]) -- also where scipy's
    raw-power fit has degraded (W 101 / 257, p 5, deriv 2: scipy's own error against the oracle is 1e-10 .. 7e-9)."""
    delta = 0.005
    c, Qt, P = filters.savgol_tables(W, p, deriv, delta)
    half = W // 2
    assert c.shape == (W,) and Qt.shape == (p + 1, W) and P.shape == (2, half, p + 1)
    assert all(t.dtype == np.float64 for t in (c, Qt, P))
    assert np.abs(Qt @ Qt.T - np.eye(p + 1)).max() <= 1e-14                  # orthonormal
    w = Q.savgol_weights_ld(W, p, deriv, delta, [(W - 1) / 2.0])[0]
    assert np.abs(c - w).max() <= TOL * max(float(np.abs(w).max()), 1e-300)
    rng = np.random.default_rng(W + p)
    for n in (W, W + 3, 2 * W + 5):
        x = Q.curve_rows(rng, 2, n)
        y = np.zeros_like(x)
        m = n - 2 * half
        if m > 0:
            first = half - (W - 1) // 2
            for k in range(W):
                y[:, half:n - half] += c[k] * x[:, first + k:first + k + m]
        y[:, :half] = (x[:, :W] @ Qt.T) @ P[0].T
        y[:, n - half:] = (x[:, n - W:] @ Qt.T) @ P[1].T
        want = Q.savgol_ext_ld(x, W, p, deriv, delta)
        if deriv > p:
            assert np.abs(y).max() == 0 and np.abs(want).max() == 0
        else:
            assert Q.rel_err(y, want) <= TOL, (n, Q.rel_err(y, want))


def test_argument_checks_answer_before_any_launch():
    # scipy's own ValueErrors from the table builder
    with pytest.raises(ValueError, match="polyorder must be less than window_length"):
        filters.savgol_tables(5, 5)
    with pytest.raises(ValueError, match="polyorder must be less than window_length"):
        filters.savgol_tables(4, 7, 1, 0.01)
    # host data is not the batch functions' business (numpy input keeps the reference's scipy arithmetic in applyFilter)
    for call in (lambda: filters.fir_filtfilt_batch(np.zeros(100), np.ones(9) / 9),
                 lambda: filters.savgol_batch(np.zeros(100), 21, 3)):
        with pytest.raises(TypeError):
            call()
    # the C entry points: MM_ERR_INVALID_ARG (-1) for every bad argument; the pointers are never dereferenced
    lib = _lib.load()
    fake = 4096
    for fn in (lib.mm_fir_filtfilt_f64, lib.mm_fir_filtfilt_f32_f64):
        assert fn(None, 1, 100, 100, fake, 9, fake, 100, None) == -1          # NULL x
        assert fn(fake, 1, 100, 100, None, 9, fake, 100, None) == -1          # NULL taps
        assert fn(fake, 1, 100, 100, fake, 9, None, 100, None) == -1          # NULL y
        assert fn(fake, 0, 100, 100, fake, 9, fake, 100, None) == -1          # no rows
        assert fn(fake, 1, 27, 27, fake, 9, fake, 27, None) == -1             # n == 3 L: scipy's padlen rule
        assert fn(fake, 1, 100, 100, fake, 1, fake, 100, None) == -1          # a single tap
        assert fn(fake, 2, 100, 99, fake, 9, fake, 100, None) == -1           # x_stride < n
        assert fn(fake, 2, 100, 100, fake, 9, fake, 99, None) == -1           # y_stride < n
    sg = lib.mm_savgol_f64
    assert sg(None, 1, 100, 100, fake, fake, fake, 21, 4, fake, 100, None) == -1
    assert sg(fake, 1, 100, 100, fake, None, fake, 21, 4, fake, 100, None) == -1      # edges need Q and P
    assert sg(fake, 1, 20, 20, fake, fake, fake, 21, 4, fake, 20, None) == -1          # window > n
    assert sg(fake, 1, 100, 100, fake, fake, fake, 0, 1, fake, 100, None) == -1
    assert sg(fake, 1, 100, 100, fake, fake, fake, 21, 22, fake, 100, None) == -1      # polyorder >= window
    assert sg(fake, 1, 100, 100, fake, fake, fake, 21, 0, fake, 100, None) == -1
    assert sg(fake, 2, 100, 50, fake, fake, fake, 21, 4, fake, 100, None) == -1
