"""CPU: the host side of Praat's intensity contour.  The window and the framing arithmetic of modulation_mfcc_amd/pint.py and
of the yardstick (tests/pint_oracle.py) against hand-worked values; the float64 restatement against the long-double one on
the cases of the GPU test (so that its bound is known to be reachable); a constant sound and a sine; the eighth header
against its ctypes table (no size_t parameter: the entries take no workspace); the unit in both builds; every refusal of
mm_pint_check and of the entries before any launch; the module imports without a GPU."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import pint_oracle as O
from conftest import ROOT
from modulation_mfcc_amd import _lib, pint

HEADER = os.path.join(ROOT, "include", "modmfcc_pint.h")
DENSE = dict(minimum_pitch=120.0, time_step=1 / 8000)

# the cases of tests/test_gpu_pint.py: sr, n, keywords
CASES = [(8000, 129, dict(minimum_pitch=400.0)), (8000, 130, dict(minimum_pitch=400.0)), (8000, 1000, dict(minimum_pitch=400.0)),
         (8000, 2180, dict(minimum_pitch=400.0)), (44100, 8820, {}), (8000, 2000, DENSE)]


def test_the_window():
    p = pint.praat_intensity_params(1000, 8000, 400.0)
    w = p.window
    assert w.dtype == np.float64 and w.shape == (129,) and np.array_equal(w, w[::-1])
    assert w[0] >= 1.0 and w[-1] >= 1.0 and (np.diff(w[:65]) > 0).all()
    x0 = 2 * np.pi ** 2 + 0.5
    assert abs(w[64] / np.i0(x0) - 1) < 2e-7 and abs(float(pint.bessel_i0(x0)) / np.i0(x0) - 1) < 2e-7
    for x in (0.0, 0.5, 3.7, 3.75, 3.8, 10.0, 20.0):
        assert abs(float(pint.bessel_i0(x)) / np.i0(x) - 1) < 2e-7, x           # the accuracy A&S state for the polynomials
        assert abs(float(pint.bessel_i0(x)) / O.bessel_i0(x) - 1) < 1e-14, x     # (numpy's exp and math.exp may differ by an ulp)
    assert np.allclose(w, O.geometry(1000, 8000, minimum_pitch=400.0)["w"], rtol=1e-14, atol=0)
    big = pint.praat_intensity_params(8820, 44100)
    assert np.allclose(big.window, O.geometry(8820, 44100)["w"], rtol=1e-14, atol=0) and big.window[0] >= 1.0


def test_the_framing_against_hand_worked_values():
    p = pint.praat_intensity_params(1000, 8000, 400.0)
    assert (p.hw, p.W, p.hops, p.time_step) == (64, 129, [16], 0.002)           # 6.4 / 400 = 16 ms = 128 samples; 2 ms = 16
    assert p.T == 55 == (1000 - 128) // 16 + 1 and p.centres.dtype == np.int32
    p = pint.praat_intensity_params(8820, 44100)
    assert (p.hw, p.W, p.T, p.hops, p.time_step) == (1411, 2823, 18, [352, 353], 0.008)       # a hop of 352.8 samples
    p = pint.praat_intensity_params(2000, 8000, **DENSE)
    assert (p.hw, p.W, p.T, p.hops) == (213, 427, 1574, [1])
    assert pint.praat_intensity_params(129, 8000, 400.0).T == 1
    assert pint.praat_intensity_params(128, 8000, 400.0).T == 1                 # the window takes 128 sample periods, has 129 taps
    with pytest.raises(ValueError, match="sound shorter than the analysis window: 127 samples"):
        pint.praat_intensity_params(127, 8000, 400.0)
    for sr, n, kw in CASES:
        p, g = pint.praat_intensity_params(n, sr, **kw), O.geometry(n, sr, **kw)
        assert (p.hw, p.W, p.T, p.t1, p.time_step) == (g["hw"], g["W"], g["T"], g["t1"], g["dt"]), (sr, n, kw)
        assert np.array_equal(p.centres, g["centres"]) and np.array_equal(p.times, g["times"])
        assert p.centres.min() >= 0 and p.centres.max() < n
        # the frames are centred in the sound
        assert abs((p.times[0] - 0) - (n / sr - p.times[-1])) < 1e-12
    # time_step None, 0 and negative are the default
    assert pint.praat_intensity_params(1000, 8000, 400.0, 0.0) is pint.praat_intensity_params(1000, 8000, 400.0, None)
    assert pint.praat_intensity_params(1000, 8000, 400.0, -1.0).time_step == 0.002


def test_n_equal_to_the_taps_and_one_less():
    """n = W gives one frame and n = W - 1 is refused -- where the window is no whole number of sample periods.  6.4 / 400 s
    are 128 periods of 8 kHz exactly, so there `phys > dur` refuses only from n = 127 down and n = 128 = W - 1 has one frame,
    its window clipped by a sample (test_the_framing_against_hand_worked_values)."""
    assert pint.praat_intensity_params(129, 8000, 400.0).T == 1
    p = pint.praat_intensity_params(2823, 44100)            # 6.4 / 100 s = 2822.4 samples: hw 1411, W 2823
    assert p.W == 2823 and p.T == 1
    with pytest.raises(ValueError, match="sound shorter than the analysis window"):
        pint.praat_intensity_params(2822, 44100)
    with pytest.raises(ValueError):
        O.geometry(2822, 44100)


@pytest.mark.parametrize("case", CASES, ids=lambda c: f"{c[0]}x{c[1]}")
def test_restatement_against_long_double(case):
    sr, n, kw = case
    for ch, dtype in ((1, np.float64), (3, np.float32)):
        x = O.noise(5, n, channels=ch, dtype=dtype)
        P64, r64 = O.references(x, sr, **kw)
        print(f"restatement {case} {ch} ch: r64 {r64:.3e}")
        assert P64.shape == (O.geometry(n, sr, **kw)["T"],) and (P64 > 0).all() and r64 < 1e-12


def test_restatement_at_an_offset_and_under_a_ramp():
    n = 2000
    x = 1000.0 + 0.01 * np.random.default_rng(2).standard_normal(n)
    _, r64 = O.references(x, 8000, minimum_pitch=400.0)
    print(f"offset: r64 {r64:.3e}")
    assert r64 < 1e-9                                                            # the centring loses digits; 16 r64 is the bound
    ramp = O.noise(3, 4000, dtype=np.float64) * 10.0 ** (-3.0 * np.arange(4000) / 4000)
    _, r64 = O.references(ramp, 8000, minimum_pitch=400.0)
    assert r64 < 1e-12


def test_a_constant_sound_and_a_sine():
    P = O.intensity(np.full(1000, 0.25), 8000, minimum_pitch=400.0)
    assert (P == 0).all() and (O.level(P) == -300.0).all()
    assert (O.intensity(np.full(1000, 0.25), 8000, minimum_pitch=400.0, subtract_mean=False) > 0.06).all()
    A = 0.3
    x = A * np.sin(2 * np.pi * 1000.0 * (np.arange(8000) + 0.5) / 8000)
    db = O.level(O.intensity(x, 8000, minimum_pitch=100.0))
    want = 10 * np.log10(A * A / 2 / 4e-10)
    assert db.shape[0] > 50 and np.abs(db[2:-2] - want).max() < 0.01, np.abs(db - want).max()


def test_the_value_lookup_restated():
    y = np.array([1.0, 3.0, 2.0, 5.0, 4.0])
    t1, dt = 0.1, 0.01
    v = lambda t, d: float(O.value(y, t1, dt, t, d))
    for d in (0, 1, 2):
        assert v(t1, d) == 1.0 and v(t1 - 0.004, d) == 1.0 and v(t1 + 4 * dt + 0.004, d) == 4.0
        assert np.isnan(v(t1 - 0.0051, d)) and np.isnan(v(t1 + 4.51 * dt, d))
    assert v(t1 + 0.4 * dt, 0) == 1.0 and v(t1 + 0.6 * dt, 0) == 3.0
    assert abs(v(t1 + 0.5 * dt, 1) - 2.0) < 1e-12 and abs(v(t1 + 0.5 * dt, 2) - 2.0) < 1e-12       # depth 1 at the edge
    # depth 2 in the interior, the midpoint of (3, 2): 2.5 - 0.25 (0.5 (dr - dl)), dl = (2 - 1) / 2, dr = (5 - 3) / 2
    assert abs(v(t1 + 1.5 * dt, 2) - (2.5 - 0.25 * 0.5 * (1.0 - 0.5))) < 1e-12
    assert float(O.value(y[:1], t1, dt, t1 + 0.3 * dt, 2)) == 1.0


# ---- the eighth header ----------------------------------------------------------------------------------------------------------
def _prototypes():
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    txt = re.sub(r"typedef struct.*?\}\s*\w+;", "", txt, flags=re.S)
    return {m.group(1): m.group(2) for m in re.finditer(r"\b(mm_[a-z0-9_]+)\s*\(([^)]*)\)", txt)}


def test_every_symbol_of_the_eighth_header_is_exported_and_bound():
    lib = _lib.load()
    protos = _prototypes()
    assert set(protos) == set(_lib.PROTOTYPES_PINT) and len(protos) == 6, set(protos) ^ set(_lib.PROTOTYPES_PINT)
    others = (_lib.PROTOTYPES, _lib.PROTOTYPES_MODPSD, _lib.PROTOTYPES_MODCSD, _lib.PROTOTYPES_SPLINE, _lib.PROTOTYPES_LOMB,
              _lib.PROTOTYPES_ZOOM, _lib.PROTOTYPES_PSPEC)
    assert not any(set(protos) & set(t) for t in others)
    taking_stream = []
    for name, params in protos.items():
        assert hasattr(lib, name), f"{name} declared in include/modmfcc_pint.h but not exported"
        res, args = _lib.PROTOTYPES_PINT[name]
        n_params = 0 if params.strip() in ("", "void") else params.count(",") + 1
        assert len(args) == n_params, (name, params, args)
        assert getattr(lib, name).argtypes == args and getattr(lib, name).restype is res
        assert "size_t" not in params and C.c_size_t not in args, f"{name}: the entries take no workspace and no size_t"
        # parameter by parameter: pointers, 64-bit counts and strides, 32-bit depth, the double time step
        for param, arg in zip([q.strip() for q in params.split(",")] if n_params else [], args):
            want = (C.c_double if param.startswith("double ") else C.c_int32 if param.startswith("int32_t ") else
                    _lib._i64 if param.startswith("int64_t ") else None)
            if "*" in param:
                assert arg in (C.c_void_p, _lib._pip), (name, param)
            else:
                assert arg is want, (name, param, arg)
        if re.search(r"void\s*\*\s*stream\s*$", params):
            taking_stream.append(name)
            assert args[-1] is C.c_void_p and res is C.c_int, name
    assert sorted(taking_stream) == ["mm_pint_f32", "mm_pint_f64", "mm_pint_value_f64"]
    txt = open(HEADER).read()
    assert lib.mm_pint_version() == int(re.search(r"#define MM_PINT_VERSION (\d+)", txt).group(1)) == 100
    assert int(re.search(r"#define MM_PINT_MAX_HALF (\d+)", txt).group(1)) == _lib.MM_PINT_MAX_HALF == pint.MAX_HALF >= 8192
    assert int(re.search(r"#define MM_PINT_MAX_CHANNELS (\d+)", txt).group(1)) == _lib.MM_PINT_MAX_CHANNELS == pint.MAX_CHANNELS == 8
    assert re.search(r"MM_PINT_LINEAR\s*=\s*1,\s*MM_PINT_KEEP_MEAN\s*=\s*2", txt)
    assert (_lib.MM_PINT_LINEAR, _lib.MM_PINT_KEEP_MEAN) == (pint._LINEAR, pint._KEEP_MEAN) == (1, 2)
    assert re.search(r"MM_PINT_NEAREST\s*=\s*0,\s*MM_PINT_LINEAR_INTERP\s*=\s*1,\s*MM_PINT_CUBIC\s*=\s*2", txt)
    assert pint.INTERPOLATIONS == {"nearest": 0, "linear": 1, "cubic": 2} == O.DEPTHS
    # the struct, field for field, in the header's order
    body = re.search(r"typedef struct mm_pint_params \{(.*?)\} mm_pint_params;", re.sub(r"/\*.*?\*/", "", txt, flags=re.S), flags=re.S)
    fields = re.findall(r"(double|int32_t)\s+(\w+)(?:\[(\d+)\])?\s*;", body.group(1))
    assert [(f[1], f[0]) for f in fields] == [(n, "int32_t") for n, t in _lib.mm_pint_params._fields_]
    assert all(t is C.c_int32 for _, t in _lib.mm_pint_params._fields_) and C.sizeof(_lib.mm_pint_params) == 20
    assert [n for n, _ in _lib.mm_pint_params._fields_] == ["hw", "channels", "span", "flags", "reserved"]
    assert lib.mm_version() == 123                                           # nothing in the other headers changed


def test_the_unit_is_in_both_builds():
    csrc = os.path.join(ROOT, "modulation_mfcc_amd", "csrc")
    mk = open(os.path.join(csrc, "Makefile")).read()
    assert re.search(r"^TUS\s*:=.*\bmm_pint\b", mk, flags=re.M) and re.search(r"^HDRS\s*:=.*modmfcc_pint\.h", mk, flags=re.M)
    assert "#   mm_pint.hip " in mk
    assert '#include "mm_pint.hip"' in open(os.path.join(csrc, "mm_unity.hip")).read()


def _params(**kw):
    d = dict(hw=64, channels=1, span=0, flags=0, reserved=0)
    d.update(kw)
    return _lib.mm_pint_params(**d)


def test_check_and_the_entries_refuse_before_any_launch():
    lib = _lib.load()
    ok = lambda **kw: lib.mm_pint_check(C.byref(_params(**kw)))
    assert ok() == _lib.MM_OK and ok(flags=3) == _lib.MM_OK and ok(channels=8) == _lib.MM_OK and ok(hw=1) == _lib.MM_OK
    assert ok(hw=_lib.MM_PINT_MAX_HALF) == _lib.MM_OK and ok(span=1 << 30) == _lib.MM_OK
    for bad in (dict(hw=0), dict(hw=-1), dict(channels=0), dict(span=-1), dict(flags=4), dict(flags=-1), dict(reserved=1)):
        assert ok(**bad) == _lib.MM_ERR_INVALID_ARG, bad
    for unsupported in (dict(hw=_lib.MM_PINT_MAX_HALF + 1), dict(channels=9)):
        assert ok(**unsupported) == _lib.MM_ERR_UNSUPPORTED, unsupported
    assert lib.mm_pint_check(None) == _lib.MM_ERR_INVALID_ARG
    tile = lambda **kw: lib.mm_pint_tile_frames(C.byref(_params(**kw)))
    t = tile()
    assert t >= 1 and t & (t - 1) == 0 and tile(hw=_lib.MM_PINT_MAX_HALF, channels=8) == t
    assert tile(channels=9) == _lib.MM_ERR_UNSUPPORTED and tile(hw=0) == _lib.MM_ERR_INVALID_ARG
    # the entries refuse bad arguments without touching a device: NULL pointers, short strides
    p = _params()
    a = dict(x=8, rows=1, n_max=1000, xr=1000, xc=1000, w=8, c=8, t=10, cr=0, ln=None, y=8, yr=10)

    def call(fn=lib.mm_pint_f32, **kw):
        v = dict(a, **kw)
        return fn(C.byref(p), v["x"], v["rows"], v["n_max"], v["xr"], v["xc"], v["w"], v["c"], v["t"], v["cr"], v["ln"], v["y"],
                  v["yr"], None)
    for bad in (dict(x=None), dict(w=None), dict(c=None), dict(y=None), dict(rows=0), dict(t=0), dict(n_max=0), dict(xc=999),
                dict(rows=2, xr=999), dict(yr=9), dict(cr=9), dict(n_max=2 ** 31 - 2 ** 15, xc=2 ** 31), dict(t=2 ** 31, yr=2 ** 31)):
        assert call(**bad) == _lib.MM_ERR_INVALID_ARG, bad
        assert call(lib.mm_pint_f64, **bad) == _lib.MM_ERR_INVALID_ARG, bad
    assert lib.mm_pint_f64(C.byref(_params(channels=9)), 8, 1, 1000, 9000, 1000, 8, 8, 10, 0, None, 8, 10, None) == _lib.MM_ERR_UNSUPPORTED
    v = dict(y=8, rows=1, t=10, yr=10, fr=None, t1=8, dt=0.01, q=8, nq=4, qr=0, depth=2, out=8, outr=4)

    def value(**kw):
        u = dict(v, **kw)
        return lib.mm_pint_value_f64(u["y"], u["rows"], u["t"], u["yr"], u["fr"], u["t1"], u["dt"], u["q"], u["nq"], u["qr"],
                                     u["depth"], u["out"], u["outr"], None)
    for bad in (dict(y=None), dict(t1=None), dict(q=None), dict(out=None), dict(rows=0), dict(t=0), dict(nq=0), dict(yr=9),
                dict(outr=3), dict(qr=3), dict(dt=0.0), dict(dt=float("nan")), dict(dt=float("inf")), dict(depth=3), dict(depth=-1)):
        assert value(**bad) == _lib.MM_ERR_INVALID_ARG, bad


def test_the_span_of_a_tile():
    c = np.array([[50, 60, 70, 85, 100, -1, -1], [55, 56, 57, 58, 59, 60, 350]], dtype=np.int32)
    assert pint._span(c[:1], 101, 2) == 116                  # tiles (50, 60), (70, 85), (100): 15 + the window
    assert pint._span(c, 101, 4) == 392                      # row 1, tile (59, 60, 350): 291 + the window
    assert pint._span(np.full((1, 4), -1, np.int32), 101, 2) == 0


def test_the_python_layer_refuses_on_the_host():
    with pytest.raises(TypeError, match="praat_intensity_batch takes a CUDA"):
        pint.praat_intensity_batch(np.zeros(1000, np.float32), 8000)
    with pytest.raises(TypeError, match="praat_intensity_ragged_batch takes a CUDA"):
        pint.praat_intensity_ragged_batch(np.zeros((2, 1000), np.float32), [1000, 500], 8000)
    with pytest.raises(ValueError, match=r"sound shorter than the analysis window: 100 samples .* \(row 2\)"):
        pint._ragged_params(np.array([1000, 500, 100]), 8000, dict(minimum_pitch=400.0), lambda b: b)
    with pytest.raises(ValueError, match=r"\(clip 7\)"):
        pint._ragged_params(np.array([1000, 100]), 8000, dict(minimum_pitch=400.0), lambda b: [4, 7][b], "clip")
    with pytest.raises(NotImplementedError, match=r"a window of 19200 samples on either side is not built \(the limit is 16384\)"):
        pint.praat_intensity_params(480000, 48000, 8.0)
    assert pint.praat_intensity_params(480000, 48000, 25.0).hw == 6144
    with pytest.raises(ValueError, match="must be positive"):
        pint.praat_intensity_params(1000, 8000, 0.0)
    with pytest.raises(ValueError, match="needs their sampling rate"):
        pint.to_intensity(np.zeros(1000))


def test_rmspraat_itself_still_raises():
    from modulation_mfcc_amd import calculate_amplitude_envelope
    with pytest.raises(NotImplementedError):
        calculate_amplitude_envelope(np.zeros(1000), 8000, method="RMSpraat")


def test_the_module_imports_without_a_gpu():
    code = ("import sys, os\nos.environ['HIP_VISIBLE_DEVICES'] = ''\nos.environ['CUDA_VISIBLE_DEVICES'] = ''\n"
            f"sys.path.insert(0, {ROOT!r})\nfrom modulation_mfcc_amd import pint\nimport modulation_mfcc_amd as M\n"
            "p = M.praat_intensity_params(8820, 44100)\nassert p.T == 18 and p.hw == 1411\n"
            "assert 'torch' not in sys.modules\nassert M.to_intensity and M.Intensity and M.praat_rms_envelope\n"
            "assert set(pint.__all__) <= set(dir(pint))\nprint('ok')\n")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stderr[-2000:]
