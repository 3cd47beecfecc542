"""CPU: the Praat-style spectrogram's host side.  The framing arithmetic of modulation_mfcc_amd/pspec.py and of the
yardstick (tests/pspec_oracle.py) against the geometry table of DESIGN.md section 19, value for value; every frame inside
its sound; the FFT restatement against the long-double direct DFT; the six window shapes; the grids; every refusal with its
message; the seventh header against its ctypes table (no size_t parameter: the entries take no workspace); the unit in both
builds; the module imports without a GPU."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import pspec_oracle as O
from conftest import ROOT
from modulation_mfcc_amd import _lib, pspec

HEADER = os.path.join(ROOT, "include", "modmfcc_pspec.h")
NARROW = dict(window_length=0.03, frequency_step=100.0)

# sr, n, keywords -> nw, T, nfft, bw, F, fs (Hz), y1, s_0, hops
TABLE = [
    (44100, 44100, {}, 438, 496, 1024, 1, 116, 43.0664, 0.0, 1, [88, 89]),
    (16000, 16000, {}, 158, 496, 512, 1, 160, 31.25, 0.0, 1, [32]),
    (8000, 8000, {}, 78, 496, 256, 1, 128, 31.25, 0.0, 1, [16]),
    (48000, 48000, {}, 478, 496, 2048, 1, 213, 23.4375, 0.0, 1, [96]),
    (22050, 5000, {}, 218, 109, 512, 1, 116, 43.0664, 0.0, 10, [44, 45]),
    (44100, 44100, NARROW, 2644, 445, 4096, 9, 51, 96.8994, 43.0664, 15, [93, 94]),
    (16000, 16000, NARROW, 958, 445, 1024, 6, 53, 93.75, 39.0625, 6, [33, 34]),
]
SHORT = [(160, 1, 1), (161, 1, 2), (191, 1, 17), (192, 2, 1), (193, 2, 2)]       # n at 16 kHz -> T, s_0


@pytest.mark.parametrize("row", TABLE, ids=lambda r: f"{r[0]}x{r[1]}{'-narrow' if r[2] else ''}")
def test_the_geometry_table(row):
    sr, n, kw, nw, T, nfft, bw, F, fs, y1, s0, hops = row
    p = pspec.praat_spectrogram_params(n, sr, **kw)
    g = O.geometry(n, sr, **kw)
    assert (p.nw, p.n_frames, p.nfft, p.bw, p.n_freqs) == (nw, T, nfft, bw, F) == (g["nw"], g["T"], g["nfft"], g["bw"], g["F"])
    assert abs(p.frequency_step - fs) < 5e-5 and abs(p.y1 - y1) < 5e-5 and p.frequency_step == g["fs"] and p.y1 == g["y1"]
    assert int(p.starts[0]) == s0 and p.hops == hops
    assert p.starts.dtype == np.int32 and np.array_equal(p.starts, g["starts"])
    assert p.t1 == g["t1"] and p.time_step == g["ts"] and p.scale == g["scale"] and np.array_equal(p.window, g["w"])
    if sr == 8000:
        assert p.maximum_frequency == 4000.0 and p.n_freqs * p.bw == p.nfft // 2        # fmax -> Nyquist, the last used bin
    if kw:
        assert abs(p.time_step - 0.002116) < 1e-6                                        # eff_t / 8, not 2 ms
    else:
        assert p.time_step == 0.002 and p.bin_hz == p.frequency_step > 20.0              # a bin per band: eff_f / 8 = 44.3 Hz


def test_frame_counts_at_the_shortest_sounds():
    for n, T, s0 in SHORT:
        p = pspec.praat_spectrogram_params(n, 16000)
        assert (p.n_frames, int(p.starts[0])) == (T, s0) == (O.geometry(n, 16000)["T"], int(O.geometry(n, 16000)["starts"][0])), n
    with pytest.raises(ValueError, match="sound shorter than the analysis window: 159 samples"):
        pspec.praat_spectrogram_params(159, 16000)
    with pytest.raises(ValueError):
        O.geometry(159, 16000)


def test_every_frame_lies_inside_its_sound():
    cases = [(r[0], r[1], r[2]) for r in TABLE] + [(16000, n, {}) for n, _, _ in SHORT]
    cases += [(sr, n, dict(window_shape=s)) for s in O.SHAPES for sr, n in ((16000, 1000), (44100, 3000), (11025, 777))]
    for sr, n, kw in cases:
        p = pspec.praat_spectrogram_params(n, sr, **kw)
        assert p.starts.min() >= 0 and int(p.starts.max()) + p.nw <= n, (sr, n, kw)
        assert (np.diff(p.starts) > 0).all() and p.nw == 2 * p.half and p.nw <= p.nfft
        assert p.n_freqs * p.bw <= p.nfft // 2


@pytest.mark.parametrize("case", [(16000, 700, {}), (22050, 1500, {}), (44100, 3000, {}), (16000, 1500, NARROW), (8000, 600, {})],
                         ids=str)
def test_fft_restatement_against_the_direct_dft(case):
    sr, n, kw = case
    x = O.noise(3, n, channels=2, dtype=np.float64)
    P64, r64, r32 = O.references(x, sr, **kw)
    print(f"restatement {case}: r64 {r64:.3e}, r32 {r32:.3e}")
    assert O.has_dft(O.geometry(n, sr, **kw)) and 0 < r64 < 1e-13
    assert 1e-8 < r32 < 2e-6                          # a few float32 roundings of the maximum
    assert P64.shape == (O.geometry(n, sr, **kw)["F"], O.geometry(n, sr, **kw)["T"]) and (P64 > 0).all()


def test_the_six_window_shapes():
    nw, nspw = 78, 80.0
    i = np.arange(1, nw + 1)
    for shape in O.SHAPES:
        w = pspec.praat_window(shape, nw, nspw)
        assert w.dtype == np.float64 and w.shape == (nw,) and np.array_equal(w, O.window(shape, nw, nspw)), shape
        assert (w >= 0).all() and w.max() <= 1.0
    assert (pspec.praat_window("SQUARE", nw, nspw) == 1).all()
    assert np.allclose(pspec.praat_window("HANNING", nw, nspw), 0.5 - 0.5 * np.cos(2 * np.pi * i / 80.0), rtol=0, atol=1e-15)
    assert np.allclose(pspec.praat_window("HAMMING", nw, nspw)[39], 1.0, atol=1e-15)                 # i = 40: the middle
    assert pspec.praat_window("BARTLETT", nw, nspw)[39] == 1.0 and pspec.praat_window("WELCH", nw, nspw)[39] == 1.0
    g = pspec.praat_window("GAUSSIAN", nw, nspw)
    assert np.array_equal(g, g[::-1]) and g[0] > 0 and abs(g[38] - (np.exp(-48 * (0.5 / 80) ** 2) - np.exp(-12)) / (1 - np.exp(-12))) < 1e-15
    # the physical window of the other shapes is window_length, of the Gaussian twice that
    assert pspec.praat_spectrogram_params(16000, 16000, window_shape="HANNING").nw == 78
    assert pspec.praat_spectrogram_params(16000, 16000, window_shape="hanning").window_shape == "HANNING"


def test_the_grids():
    p = pspec.praat_spectrogram_params(5000, 22050)
    g = O.geometry(5000, 22050)
    for name in ("times", "freqs", "x_grid", "y_grid"):
        assert np.array_equal(getattr(p, name), g[name]), name
    assert p.x_grid.shape == (p.n_frames + 1,) and p.y_grid.shape == (p.n_freqs + 1,)
    assert np.allclose(0.5 * (p.x_grid[:-1] + p.x_grid[1:]), p.times, rtol=0, atol=1e-12)
    assert np.allclose(0.5 * (p.y_grid[:-1] + p.y_grid[1:]), p.freqs, rtol=0, atol=1e-9)
    assert p.y_grid[0] == p.y1 - p.frequency_step / 2 and p.times[0] == p.t1
    # the frames are centred in the sound
    assert abs((p.times[0] - 0) - (5000 / 22050 - p.times[-1])) < 1e-12


def test_every_refusal_with_its_message():
    f = pspec.praat_spectrogram_params
    with pytest.raises(ValueError, match="analysis window too short: less than one sample pair"):
        f(16000, 16000, window_length=0.0001)                             # 3 samples: half = 0
    with pytest.raises(ValueError, match=r"sound shorter than the analysis window: 100 samples are 0\.0062\d* s, the window takes 0\.01 s"):
        f(100, 16000)
    with pytest.raises(ValueError, match="no frequency band: maximum_frequency 10.0 Hz is below the frequency step"):
        f(16000, 16000, maximum_frequency=10.0)
    with pytest.raises(ValueError, match="unknown window_shape 'KAISER': the shapes are SQUARE, HAMMING, BARTLETT, WELCH, HANNING, GAUSSIAN"):
        f(16000, 16000, window_shape="KAISER")
    with pytest.raises(NotImplementedError, match=r"a transform of 8192 points is not built \(the limit is 4096\)"):
        f(44100, 44100, window_length=0.05)
    with pytest.raises(NotImplementedError, match="8192 points"):
        f(44100, 44100, maximum_frequency=0.0, frequency_step=5.0, window_length=0.04)
    with pytest.raises(ValueError, match="must be positive"):
        f(16000, 16000, window_length=0.0)


def test_the_batch_calls_refuse_on_the_host():
    with pytest.raises(TypeError, match="praat_spectrogram_batch takes a CUDA"):
        pspec.praat_spectrogram_batch(np.zeros(1000, np.float32), 16000)
    with pytest.raises(TypeError, match="praat_spectrogram_ragged_batch takes a CUDA"):
        pspec.praat_spectrogram_ragged_batch(np.zeros((2, 1000), np.float32), [1000, 500], 16000)
    with pytest.raises(ValueError, match="needs its sampling rate"):
        class T:                                                            # (duck-typed device tensor: no GPU here)
            is_cuda = True
        T.__module__ = "torch"
        pspec.spectrogram_view(T())
    # a refusal of a ragged batch names its clip
    with pytest.raises(ValueError, match=r"sound shorter than the analysis window: 100 samples .* \(clip 2\)"):
        pspec._ragged_params(np.array([1000, 500, 100]), 16000, {}, lambda b: b)
    with pytest.raises(ValueError, match=r"\(clip 7\)"):
        pspec._ragged_params(np.array([1000, 100]), 16000, {}, lambda b: [4, 7][b])


# ---- the seventh header ----------------------------------------------------------------------------------------------------------
def _prototypes():
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    txt = re.sub(r"typedef struct.*?\}\s*\w+;", "", txt, flags=re.S)
    return {m.group(1): m.group(2) for m in re.finditer(r"\b(mm_[a-z0-9_]+)\s*\(([^)]*)\)", txt)}


def test_every_symbol_of_the_seventh_header_is_exported_and_bound():
    lib = _lib.load()
    protos = _prototypes()
    assert set(protos) == set(_lib.PROTOTYPES_PSPEC) and len(protos) == 5, set(protos) ^ set(_lib.PROTOTYPES_PSPEC)
    others = (_lib.PROTOTYPES, _lib.PROTOTYPES_MODPSD, _lib.PROTOTYPES_MODCSD, _lib.PROTOTYPES_SPLINE, _lib.PROTOTYPES_LOMB,
              _lib.PROTOTYPES_ZOOM)
    assert not any(set(protos) & set(t) for t in others)
    taking_stream = []
    for name, params in protos.items():
        assert hasattr(lib, name), f"{name} declared in include/modmfcc_pspec.h but not exported"
        res, args = _lib.PROTOTYPES_PSPEC[name]
        n_params = 0 if params.strip() in ("", "void") else params.count(",") + 1
        assert len(args) == n_params, (name, params, args)
        assert getattr(lib, name).argtypes == args and getattr(lib, name).restype is res
        assert "size_t" not in params and C.c_size_t not in args, f"{name}: the entries take no workspace and no size_t"
        if re.search(r"void\s*\*\s*stream\s*$", params):
            taking_stream.append(name)
            assert args[-1] is C.c_void_p and res is C.c_int, name
    assert sorted(taking_stream) == ["mm_pspec_f32", "mm_pspec_f64"]
    txt = open(HEADER).read()
    assert lib.mm_pspec_version() == int(re.search(r"#define MM_PSPEC_VERSION (\d+)", txt).group(1)) == 100
    assert int(re.search(r"#define MM_PSPEC_MAX_NFFT (\d+)", txt).group(1)) == _lib.MM_PSPEC_MAX_NFFT == pspec.MAX_NFFT
    assert int(re.search(r"#define MM_PSPEC_MAX_CHANNELS (\d+)", txt).group(1)) == _lib.MM_PSPEC_MAX_CHANNELS == pspec.MAX_CHANNELS
    assert re.search(r"MM_PSPEC_DB\s*=\s*1", txt) and _lib.MM_PSPEC_DB == pspec._DB == 1
    # the struct, field for field, in the header's order
    body = re.search(r"typedef struct mm_pspec_params \{(.*?)\} mm_pspec_params;", re.sub(r"/\*.*?\*/", "", txt, flags=re.S), flags=re.S)
    fields = re.findall(r"(double|int32_t)\s+(\w+)(?:\[(\d+)\])?\s*;", body.group(1))
    assert [(f[1], f[0]) for f in fields] == [(n, "double" if t is C.c_double else "int32_t") for n, t in _lib.mm_pspec_params._fields_]
    assert C.sizeof(_lib.mm_pspec_params) == 40
    assert lib.mm_version() == 123                                           # nothing in the other headers changed


def test_the_unit_is_in_both_builds():
    csrc = os.path.join(ROOT, "modulation_mfcc_amd", "csrc")
    mk = open(os.path.join(csrc, "Makefile")).read()
    assert re.search(r"^TUS\s*:=.*\bmm_pspec\b", mk, flags=re.M) and re.search(r"^HDRS\s*:=.*modmfcc_pspec\.h", mk, flags=re.M)
    assert "#   mm_pspec.hip " in mk
    assert '#include "mm_pspec.hip"' in open(os.path.join(csrc, "mm_unity.hip")).read()
    src = open(os.path.join(csrc, "mm_pspec.hip")).read()
    assert "wave_cfft_lds(" in src and "real_split(" in src, "the transform is the shared one of mm_common.h"


def _params(**kw):
    d = dict(scale=1.0, nw=158, nfft=512, bw=1, n_freqs=160, channels=1, span=0, flags=0, reserved=0)
    d.update(kw)
    return _lib.mm_pspec_params(**d)


def test_check_and_tile_frames_refuse_before_any_launch():
    lib = _lib.load()
    ok = lambda **kw: lib.mm_pspec_check(C.byref(_params(**kw)))
    assert ok() == _lib.MM_OK and ok(flags=1) == _lib.MM_OK and ok(channels=8) == _lib.MM_OK and ok(nfft=4096, nw=4096) == _lib.MM_OK
    for bad in (dict(nw=1), dict(bw=0), dict(n_freqs=0), dict(channels=0), dict(span=-1), dict(scale=0.0), dict(scale=float("nan")),
                dict(scale=float("inf")), dict(flags=2), dict(reserved=1), dict(n_freqs=257), dict(bw=2, n_freqs=129)):
        assert ok(**bad) == _lib.MM_ERR_INVALID_ARG, bad
    for unsupported in (dict(nfft=16, nw=8, n_freqs=8), dict(nfft=8192), dict(nfft=500), dict(nw=514), dict(channels=9)):
        assert ok(**unsupported) == _lib.MM_ERR_UNSUPPORTED, unsupported
    assert lib.mm_pspec_check(None) == _lib.MM_ERR_INVALID_ARG
    tile = lambda **kw: lib.mm_pspec_tile_frames(C.byref(_params(**kw)))
    assert tile() == 32 and tile(nfft=1024, n_freqs=116) == 32 and tile(nfft=2048, n_freqs=213) == 16 and tile(nfft=4096, nw=2644, bw=9, n_freqs=51) == 16
    assert tile(nfft=1024, n_freqs=512) == 16 and tile(nfft=4096, n_freqs=2048) == 1          # a wide image: a smaller tile
    assert tile(nfft=8192) == _lib.MM_ERR_UNSUPPORTED and tile(nw=1) == _lib.MM_ERR_INVALID_ARG
    # the entries refuse bad arguments without touching a device: NULL pointers, short strides
    p = _params()
    a = dict(x=8, rows=1, n_max=1000, xr=1000, xc=1000, w=8, s=8, t=10, sr=0, y=8, yr=1600, yb=10)

    def call(**kw):
        v = dict(a, **kw)
        return lib.mm_pspec_f32(C.byref(p), v["x"], v["rows"], v["n_max"], v["xr"], v["xc"], v["w"], v["s"], v["t"], v["sr"], v["y"],
                                v["yr"], v["yb"], None)
    for bad in (dict(x=None), dict(w=None), dict(s=None), dict(y=None), dict(rows=0), dict(t=0), dict(n_max=157), dict(xc=999),
                dict(rows=2, xr=999), dict(yb=9), dict(yr=1599), dict(sr=9), dict(n_max=2 ** 31 - 4096, xc=2 ** 31)):
        assert call(**bad) == _lib.MM_ERR_INVALID_ARG, bad
    assert lib.mm_pspec_f64(C.byref(_params(nfft=8192)), 8, 1, 1000, 1000, 1000, 8, 8, 10, 0, 8, 1600, 10, None) == _lib.MM_ERR_UNSUPPORTED


def test_the_span_of_a_tile():
    s = np.array([[0, 10, 20, 35, 50, -1, -1], [5, 6, 7, 8, 9, 10, 300]], dtype=np.int32)
    assert pspec._span(s[:1], 100, 2) == 115                 # tiles (0, 10), (20, 35), (50): 15 + the window
    assert pspec._span(s, 100, 4) == 391                     # row 1, tile (9, 10, 300): 291 + the window
    assert pspec._span(s[:1], 100, 32) == 150 and pspec._span(np.full((1, 4), -1, np.int32), 100, 2) == 0


def test_the_module_imports_without_a_gpu():
    code = ("import sys, os\nos.environ['HIP_VISIBLE_DEVICES'] = ''\nos.environ['CUDA_VISIBLE_DEVICES'] = ''\n"
            f"sys.path.insert(0, {ROOT!r})\nfrom modulation_mfcc_amd import pspec\nimport modulation_mfcc_amd as M\n"
            "p = M.praat_spectrogram_params(16000, 16000)\nassert p.n_frames == 496 and p.nfft == 512\n"
            "assert 'torch' not in sys.modules\nassert M.Parselmouth and M.Sound and M.Spectrogram and M.spectrogram_view\nprint('ok')\n")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stderr[-2000:]
