"""GPU (-m gpu): scipy.signal.sosfiltfilt on the device -- mm_sosfiltfilt_f64 / _f32_f64 and the two filters inside
mm_mfcc_change_f64 -- in its four forms (a wave per 1088-sample segment, a workgroup per row, the time-major chunked
kernels, the clip-resident change tail), against tests/sos_oracle.py: scipy's sosfiltfilt restated sequentially in
80-bit long double, with scipy's OWN float64 error against it as the unit where the poles approach the unit circle.

A  conditioning sweep    E_dev <= R * max(E_ref, 1e-15);  E_dev <= 1e-8 wherever applyFilter's UI can reach
B  foreign sections      elliptic / Chebyshev / Bessel / notch / peak / hand-built: 1e-10, padlen, rows independent
C  kind x form x segment boundary   1e-10
D  the change tail: every parameter set on every form   1e-10 against scipy (wn >= 0.02)
E  edges: non-finite rows, scipy's two SOS ValueErrors, 16 and 17 sections

MEASURED (MI355X; n = 12 000, rows 0 and last; E = max|y - ext| / max|ext|; 4 rows: a wave per segment, 128 rows: a
workgroup per row; butter(10, .) is five sections: the time-major kernels at both row counts):

    filter                sections  E_ref (scipy)  E_dev 4 rows  ratio  E_dev 128 rows  ratio
    butter2_12Hz@10k             1       4.49e-13      1.19e-12   2.66        1.19e-12   2.66
    butter2_12Hz@16k             1       1.19e-12      1.95e-12   1.64        1.95e-12   1.64
    butter2_12Hz@44.1k           1       1.68e-11      1.19e-11   0.71        1.19e-11   0.71
    butter2_12Hz@48k             1       3.10e-11      1.40e-11   0.45        1.40e-11   0.45
    butter2_3Hz@48k              1       3.22e-10      3.94e-10   1.22        3.94e-10   1.22
    butter4_12Hz@10k             2       1.06e-12      1.29e-12   1.21        1.29e-12   1.21
    butter4_12Hz@16k             2       2.71e-12      4.18e-12   1.54        4.18e-12   1.54
    butter4_12Hz@44.1k           2       1.73e-11      2.47e-11   1.43        2.47e-11   1.43
    butter4_12Hz@48k             2       1.65e-11      2.58e-11   1.57        2.58e-11   1.57
    butter4_3Hz@48k              2       2.09e-10      4.41e-10   2.11        4.41e-10   2.11
    butter6_12Hz@10k             3       1.29e-12      1.94e-12   1.51        1.94e-12   1.51
    butter6_12Hz@16k             3       3.43e-12      5.04e-12   1.47        5.04e-12   1.47
    butter6_12Hz@44.1k           3       3.75e-11      2.38e-11   0.63        2.38e-11   0.63
    butter6_12Hz@48k             3       4.65e-11      4.43e-11   0.95        4.43e-11   0.95
    butter6_3Hz@48k              3       6.36e-10      6.20e-10   0.98        6.20e-10   0.98
    butter8_12Hz@10k             4       1.96e-12      2.04e-12   1.04        2.04e-12   1.04
    butter8_12Hz@16k             4       3.56e-12      6.08e-12   1.71        6.08e-12   1.71
    butter8_12Hz@44.1k           4       1.25e-11      4.09e-11   3.28        4.09e-11   3.28
    butter8_12Hz@48k             4       3.53e-11      3.18e-11   0.90        3.18e-11   0.90
    butter8_3Hz@48k              4       7.93e-10      4.15e-10   0.52        4.15e-10   0.52
    band2_0.0100_0.0105          2       1.09e-12      1.51e-12   1.37        1.51e-12   1.37
    notch_0.1_q300               1       2.17e-14      3.51e-15   0.16        3.51e-15   0.16
    butter10_12Hz@16k            5       4.02e-12      1.47e-12   0.37        1.47e-12   0.37

Worst ratio 3.28 (butter(8, 5.4e-4)); R = 4 x 3.28 = 13.1, rounded up to a power of two: 16.  Before the scan tables were
built in extended precision (mm_sos.hip.inc, sos_scan_tables) the same sweep gave ratios of 55 - 2700 and
E_dev = 6.5e-9 - 2.9e-8 at 12 Hz on 44.1 / 48 kHz.
"""
import contextlib
import functools
import re

import numpy as np
import pytest
import scipy.signal

import mfcc_oracle as O
import sos_oracle as Q
from conftest import load_golden

pytestmark = pytest.mark.gpu

# four times the worst measured E_dev / max(E_ref, 1e-15) of the sweep (table above), rounded up to a power of two
R_SWEEP = 16.0


def _dev(x, gpu):
    import torch
    x = np.ascontiguousarray(x)
    return torch.from_numpy(x if x.flags.writeable else x.copy()).to(gpu)      # (the shared inputs are read-only)


def _batch(x, sos, gpu):
    from modulation_mfcc_amd import sosfiltfilt_batch
    return sosfiltfilt_batch(_dev(x, gpu), sos).cpu().numpy()


def _via_apply_filter(x, sos, gpu):
    from modulation_mfcc_amd import applyFilter     # (sr and cutOff only pass applyFilter's argument checks)
    return applyFilter(_dev(x, gpu), 2.0, filt="iir", cutOff=[0.5], coeffs=sos).cpu().numpy()


# ---------------------------------------------------------------------------------------------------------------------
# A. conditioning sweep
# ---------------------------------------------------------------------------------------------------------------------
_SWEEP_WN = {2.4e-3: "12Hz@10k", 1.5e-3: "12Hz@16k", 5.4e-4: "12Hz@44.1k", 5e-4: "12Hz@48k", 1.25e-4: "3Hz@48k"}
_UI_WN = (2.4e-3, 1.5e-3, 5.4e-4, 5e-4)


def _sweep_points():
    pts = []
    for order in (2, 4, 6, 8):
        for wn in _SWEEP_WN:
            pts.append((f"butter{order}_{_SWEEP_WN[wn]}", functools.partial(scipy.signal.butter, order, wn, output="sos"),
                        wn in _UI_WN))
    pts.append(("band2_0.0100_0.0105", functools.partial(scipy.signal.butter, 2, [0.0100, 0.0105], "band", output="sos"), False))
    pts.append(("notch_0.1_q300", lambda: scipy.signal.tf2sos(*scipy.signal.iirnotch(0.1, 300)), False))
    pts.append(("butter10_12Hz@16k", functools.partial(scipy.signal.butter, 10, 1.5e-3, output="sos"), False))
    return pts


_SWEEP = _sweep_points()
_SWEEP_N = 12000


@functools.lru_cache(maxsize=None)
def _sweep_rows():
    x = Q.envelope_rows(np.random.default_rng(2024), 128, _SWEEP_N)
    x.setflags(write=False)
    return x


def sweep_case(sos, gpu):
    """(E_ref, {rows: E_dev}) of one filter: rows 0 and last of the 128-row batch, which are rows 0 and 3 of the 4-row one."""
    x = _sweep_rows()
    xs = x[[0, 127]]
    ext = Q.sosfiltfilt_ext(sos, xs)
    e_ref = Q.rel_err(scipy.signal.sosfiltfilt(sos, xs, axis=1), ext)
    e_dev = {4: Q.rel_err(_batch(x[[0, 1, 2, 127]], sos, gpu)[[0, 3]], ext),
             128: Q.rel_err(_batch(x, sos, gpu)[[0, 127]], ext)}
    return e_ref, e_dev


@pytest.mark.parametrize("name,design,ui", _SWEEP, ids=[p[0] for p in _SWEEP])
def test_conditioning_sweep(name, design, ui, gpu):
    sos = design()
    e_ref, e_dev = sweep_case(sos, gpu)
    for rows, e in e_dev.items():
        print(f"SWEEP {name} sections {sos.shape[0]} rows {rows} E_ref {e_ref:.2e} E_dev {e:.2e} ratio {e / max(e_ref, 1e-15):.2f}")
    for rows, e in e_dev.items():
        assert e <= R_SWEEP * max(e_ref, 1e-15), (name, rows, e, e_ref)
        if ui:      # the bound the project publishes for applyFilter(filt='iir'): orders <= 8, 12 Hz at up to 48 kHz
            assert e <= 1e-8, (name, rows, e)


# ---------------------------------------------------------------------------------------------------------------------
# B. foreign sections
# ---------------------------------------------------------------------------------------------------------------------
_FOREIGN = Q.foreign_designs()


@pytest.mark.parametrize("name", sorted(_FOREIGN))
def test_foreign_sections(name, gpu):
    """Sections that are not Butterworth's through both entry points, float64 and float32 rows, the shortest length scipy
    admits, one segment exactly, one sample more, several segments; 3 rows (a wave per segment) and 130 (a workgroup per
    row); 1e-10 of the maximum against the extended-precision oracle (scipy's own distance from it on these designs:
    test_sos_host.py)."""
    sos = _FOREIGN[name]
    pad = Q.padlen_of(sos)
    rng = np.random.default_rng(sorted(_FOREIGN).index(name))
    for n in (pad + 1, 1088 - 2 * pad, 1089 - 2 * pad, 5000):
        for dt in (np.float64, np.float32):
            x = Q.envelope_rows(rng, 130, n, dt)
            ext = Q.sosfiltfilt_ext(sos, x[[0, 2, 129]])
            got3, got130 = _batch(x[:3], sos, gpu), _batch(x, sos, gpu)
            assert got3.dtype == got130.dtype == np.float64 and got130.shape == x.shape
            e3, e130 = Q.rel_err(got3[[0, 2]], ext[:2]), Q.rel_err(got130[[0, 2, 129]], ext)
            print(f"FOREIGN {name} n {n} {np.dtype(dt).name} E_dev rows3 {e3:.2e} rows130 {e130:.2e}")
            assert e3 <= 1e-10 and e130 <= 1e-10, (n, dt, e3, e130)
            # applyFilter(coeffs=) is the same launch
            np.testing.assert_array_equal(_via_apply_filter(x[:3], sos, gpu), got3)
            np.testing.assert_array_equal(_via_apply_filter(x, sos, gpu), got130)
            # a row does not depend on its neighbours or on its place in the batch: alone | among 3 (both a wave per
            # segment); among 130 in either order (both a workgroup per row)
            np.testing.assert_array_equal(_batch(x[2], sos, gpu), got3[2])
            np.testing.assert_array_equal(_batch(x[::-1], sos, gpu)[::-1], got130)
    for fn in (_batch, _via_apply_filter):
        with pytest.raises(ValueError, match=f"greater than padlen, which is {pad}\\."):
            fn(x[:3, :pad], sos, gpu)


# ---------------------------------------------------------------------------------------------------------------------
# C. kind x form x segment boundary
# ---------------------------------------------------------------------------------------------------------------------
_SR = 16000.0
_KINDS = {"low": [400.0], "high": [400.0], "band": [300.0, 1200.0]}
_KIND_ORDER = [(k, o) for k in _KINDS for o in (1, 2, 3, 4)] + [("band", 5)]


def _butter(kind, order):
    wn = [f / (_SR / 2) for f in _KINDS[kind]]
    return scipy.signal.butter(order, wn if kind == "band" else wn[0], kind, output="sos")


def _check_rows(sos, rows, n, gpu, seed):
    x = Q.envelope_rows(np.random.default_rng(seed), rows, n)
    pick = sorted({0, rows // 2, rows - 1})
    got = _batch(x, sos, gpu)
    e = Q.rel_err(got[pick], Q.sosfiltfilt_ext(sos, x[pick]))
    print(f"ROWS sections {sos.shape[0]} rows {rows} n {n} E_dev {e:.2e}")
    assert e <= 1e-10, (rows, n, e)


@pytest.mark.parametrize("kind,order", _KIND_ORDER, ids=[f"{k}{o}" for k, o in _KIND_ORDER])
def test_filter_kinds_on_every_form(kind, order, gpu):
    """Butterworth low / high / band-pass, 1 - 4 sections (band order 4: the last segmented case) and band order 5 (five
    sections: time-major): 5 rows of one segment (the apply kernel alone), 5 rows of five segments (state, scan, apply),
    128 rows (a workgroup per row)."""
    sos = _butter(kind, order)
    for rows, n in ((5, 800), (5, 5000), (128, 5000)):
        _check_rows(sos, rows, n, gpu, 100 * order + rows)


_SEGMENTED = [(k, o) for k, o in _KIND_ORDER if _butter(k, o).shape[0] <= 4]


@pytest.mark.parametrize("k", [2, 16, 17])
@pytest.mark.parametrize("kind,order", _SEGMENTED, ids=[f"{k}{o}" for k, o in _SEGMENTED])
def test_workgroup_per_row_at_segment_boundaries(kind, order, k, gpu):
    """128 rows, n + 2 pad = 1088 k and 1088 k + 1: the last segment full | one sample long; 16 segments are one round of
    sos_row_stream_kernel exactly, 17 are a round and one segment.  (Filters of up to four sections: the time-major
    kernels of the fifth have no segments.)"""
    sos = _butter(kind, order)
    for n_ext in (1088 * k, 1088 * k + 1):
        _check_rows(sos, 128, n_ext - 2 * Q.padlen_of(sos), gpu, k)


@pytest.mark.parametrize("k", [64, 65])
@pytest.mark.parametrize("kind,order", _SEGMENTED, ids=[f"{k}{o}" for k, o in _SEGMENTED])
def test_wave_per_segment_scan_at_64_segments(kind, order, k, gpu):
    """2 rows, n + 2 pad = 1088 k and 1088 k + 1: sos_seg_scan_kernel takes 64 segments at a time -- one round exactly,
    one round and a segment, and (k = 65, + 1) a second round of two."""
    sos = _butter(kind, order)
    for n_ext in (1088 * k, 1088 * k + 1):
        _check_rows(sos, 2, n_ext - 2 * Q.padlen_of(sos), gpu, k)


# ---------------------------------------------------------------------------------------------------------------------
# D. the change tail: every parameter set on every form
# ---------------------------------------------------------------------------------------------------------------------
def _tail_sets():
    import test_gpu_parity
    for mark in test_gpu_parity.test_change_tail_on_device.pytestmark:
        if mark.name == "parametrize" and mark.args[0] == "kwargs":
            return list(mark.args[1])
    raise AssertionError("the parameter sets of test_change_tail_on_device are gone")


_TAIL_SETS = _tail_sets() + [
    dict(filtOrd=9, outFiltCutOff=[12]),                    # five sections: time-major even when fused
    dict(filtOrd=6, outFiltLen=1, outFiltCutOff=[12]),      # three sections against one
    dict(filtOrd=2, outFiltLen=8, outFiltCutOff=[12]),      # one against four
]
# shape (n_mfcc, B, T) -> the form mm_mfcc_change_f64 takes when fused (change_form(), mm_tail.hip), 12 rows after c0:
#  (13, 2, 5500)    order 6: pad 21, n1 = 5542, pitch 5543.  Half the LDS: 10240 - 5542 - 1 doubles of room < pitch, no row
#                   fits; all of it: (20480 - 5543) / 5543 = 2 rows at once -> 6 groups > 4: SEGMENTED, 12 | 24 rows (a wave
#                   per segment), curve batch 2.  (Any pad of these sets gives pitch > 5100: at most 2 rows, >= 6 groups.)
#  (13, 3, 3001)    pitch 3043: half the LDS holds 2 rows (6 groups > 2), all of it 17435 / 3043 = 5 -> 3 groups of 4: CLIP
#  (13, 130, 5500)  segmented as the first, 1560 rows and a curve batch of 130: a workgroup per row for both filters
# set_fuse_tail(False) turns each into the time-major kernels.
_TAIL_SHAPES = [(13, 2, 5500), (13, 3, 3001), (13, 130, 5500)]


def _is_big_set(kw):
    return kw == dict(outFiltCutOff=[12]) or kw.get("diffMethod") == "sg" or ("outFilter" in kw and kw["outFilter"] is None)


_TAIL_CASES = [(s, i) for s in _TAIL_SHAPES for i, kw in enumerate(_TAIL_SETS) if s[1] < 128 or _is_big_set(kw)]


@functools.lru_cache(maxsize=2)
def _tail_input(shape):
    n_mfcc, B, T = shape
    m = np.random.default_rng(4).standard_normal((B, n_mfcc, T)).cumsum(axis=2).astype(np.float32)
    m.setflags(write=False)
    return m


@functools.lru_cache(maxsize=4)
def _tail_want(shape, idx):
    m = _tail_input(shape)
    B = shape[1]
    return {i: O.mfcc_change_tail(m[i], tStep=0.005, **_TAIL_SETS[idx]) for i in sorted({0, B // 2, B - 1})}


@contextlib.contextmanager
def _change_form(plan, form):
    prev = plan.set_fuse_tail(form == "fused")
    try:
        yield
    finally:
        plan.set_fuse_tail(prev)


@pytest.mark.parametrize("form", ["fused", "time-major"])
@pytest.mark.parametrize("shape,idx", _TAIL_CASES, ids=[f"{s[1]}x{s[2]}-set{i}" for s, i in _TAIL_CASES])
def test_change_tail_parameters_on_every_form(shape, idx, form, gpu):
    """mm_mfcc_change_f64 with every parameter set of test_change_tail_on_device (and three with unequal section counts)
    where the fused call takes the segmented form, where it takes the clip form with three groups of rows, and on the
    time-major kernels for both; against scipy's sequential tail (wn >= 0.02: scipy is the yardstick), 1e-10 of the
    curve's maximum."""
    from modulation_mfcc_amd import MfccConfig, get_plan, tail
    kw, _, _ = load_golden("c1_am")
    plan = get_plan(MfccConfig(**dict(kw, n_mfcc=shape[0])))
    m = _tail_input(shape)
    with _change_form(plan, form):
        got = tail.mfcc_change_device(plan, _dev(m, gpu), tStep=0.005, **_TAIL_SETS[idx])
    assert tuple(got.shape) == (shape[1], shape[2])
    for i, want in _tail_want(shape, idx).items():
        g = got[i].cpu().numpy()
        e = np.abs(g - want).max() / np.abs(want).max()
        print(f"TAIL {shape} set {idx} {form} clip {i} E {e:.2e}")
        assert e <= 1e-10, (i, e)


# ---------------------------------------------------------------------------------------------------------------------
# E. edges
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sections", [2, 5])
@pytest.mark.parametrize("rows", [6, 130])
def test_non_finite_rows_stay_in_their_rows(rows, sections, gpu):
    """A NaN mid-row, +inf near the start, -inf in the first sample: scipy returns those rows all-NaN (asserted) and so
    does the device; every other row comes out bit for bit as from the same batch without the three values."""
    sos = scipy.signal.butter(2 * sections, 0.05, output="sos")
    clean = Q.envelope_rows(np.random.default_rng(rows), rows, 3000)
    x = clean.copy()
    x[1, 1500], x[2, 7], x[5, 0] = np.nan, np.inf, -np.inf
    bad = np.zeros(rows, dtype=bool)
    bad[[1, 2, 5]] = True
    with np.errstate(all="ignore"):
        assert np.array_equal(np.isnan(scipy.signal.sosfiltfilt(sos, x, axis=1)).all(axis=1), bad)
    got, ref = _batch(x, sos, gpu), _batch(clean, sos, gpu)
    assert np.isnan(got[bad]).all()
    np.testing.assert_array_equal(got[~bad], ref[~bad])
    assert Q.rel_err(ref[[0, rows - 1]], Q.sosfiltfilt_ext(sos, clean[[0, rows - 1]])) <= 1e-10


def test_sos_arguments_are_validated_as_scipy_validates_them(gpu):
    """Sections scaled so that a0 = 2 and a flat vector of twelve numbers: scipy.signal.sosfiltfilt raises ValueError for
    both; sosfiltfilt_batch, applyFilter(coeffs=) and MfccPlan.mfcc_change raise the same before anything is launched."""
    from modulation_mfcc_amd import MfccConfig, get_plan
    sos = scipy.signal.butter(4, 0.2, output="sos")
    x = Q.envelope_rows(np.random.default_rng(0), 3, 200)
    kw, _, _ = load_golden("c1_am")
    plan = get_plan(MfccConfig(**kw))
    m = _dev(np.zeros((2, kw["n_mfcc"], 200), dtype=np.float32), gpu)
    for bad in (sos * 2.0, sos.ravel(), sos[None]):
        with pytest.raises(ValueError) as es:
            scipy.signal.sosfiltfilt(bad, x, axis=1)
        msg = "^" + re.escape(str(es.value)) + "$"
        for fn in (_batch, _via_apply_filter):
            with pytest.raises(ValueError, match=msg):
                fn(x, bad, gpu)
        with pytest.raises(ValueError, match=msg):
            plan.mfcc_change(m, bad)
        with pytest.raises(ValueError, match=msg):
            plan.mfcc_change(m, sos, bad)
    with pytest.raises(ValueError, match=re.escape("sos[:, 3] should be all ones")):
        _batch(x, sos * 2.0, gpu)
    assert tuple(plan.mfcc_change(m, sos, sos).shape) == (2, 200)


def test_sixteen_sections_and_seventeen(gpu):
    """MM_MAX_SEC = 16 sections (a low-pass of order 32, a band-pass of order 16) match the oracle; 17 are refused with
    MMError and the output buffer keeps what it held."""
    import ctypes as C
    import torch
    from modulation_mfcc_amd import _lib
    x = Q.envelope_rows(np.random.default_rng(16), 3, 2000)
    for sos in (scipy.signal.butter(32, 0.3, output="sos"), scipy.signal.butter(16, [0.2, 0.4], "band", output="sos")):
        assert sos.shape == (16, 6)
        e = Q.rel_err(_batch(x, sos, gpu), Q.sosfiltfilt_ext(sos, x))
        print(f"SIXTEEN E_dev {e:.2e}")
        assert e <= 1e-10
    sos17 = np.ascontiguousarray(scipy.signal.butter(33, 0.3, output="sos"))
    assert sos17.shape == (17, 6)
    with pytest.raises(_lib.MMError):
        _batch(x, sos17, gpu)
    with pytest.raises(_lib.MMError):
        _via_apply_filter(x, sos17, gpu)
    lib = _lib.load()
    xd = _dev(x, gpu)
    out = torch.full((3, 2000), 7.25, dtype=torch.float64, device=gpu)
    ws = torch.empty(int(lib.mm_sosfiltfilt_workspace_bytes(3, 2000)), dtype=torch.uint8, device=gpu)
    rc = lib.mm_sosfiltfilt_f64(xd.data_ptr(), 3, 2000, xd.stride(0), sos17.ctypes.data, 17, out.data_ptr(), ws.data_ptr(),
                                ws.numel(), C.c_void_p(torch.cuda.current_stream(gpu).cuda_stream))
    torch.cuda.synchronize()
    assert rc == _lib.MM_ERR_INVALID_ARG      # (the C entry point refuses it as well)
    assert bool((out == 7.25).all())
