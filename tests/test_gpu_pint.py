"""GPU: praat_intensity_batch / _ragged_batch / _list, to_intensity, Intensity.get_value and praat_rms_envelope (mm_pint_f32 /
_f64 / mm_pint_value_f64, csrc/mm_pint.hip) against the yardstick of tests/pint_oracle.py: the float64 restatement of
DESIGN.md section 20, per frame and relative to the frame's own power, within max(1e-12, 16 r64) -- on one frame, two
frames, a last tile of one frame, a fractional hop, the dense form (a frame per sample), the largest half width, frames
outside the staged copy; float32 samples bit for bit the float64 entry on the widened samples; quiet frames under a 60 dB
ramp; a large offset; silence; dB against the kernel's own linear output; clipped windows, entries the kernel does not
trust and NaN behind a length through the C ABI; bit-for-bit independence of the batch, the strides, the table's form and
the entry's place in it; ragged batches with host and device lengths; guard bands; the lookup at every depth.

Every measured error is printed before it is asserted (pytest -s shows them; docs/experiments.md lists a run)."""
import ctypes as C

import numpy as np
import pytest

import pint_oracle as O

pytestmark = pytest.mark.gpu

DTYPES = [np.float32, np.float64]
IDS = ["f32", "f64"]
P400 = dict(minimum_pitch=400.0)                     # 8 kHz: hw 64, 129 taps, a hop of 16 samples
DENSE = dict(minimum_pitch=120.0, time_step=1 / 8000)     # 8 kHz: hw 213, 427 taps, a frame per sample
MAXHW = dict(minimum_pitch=9.375)                    # 48 kHz: hw 16384 = MM_PINT_MAX_HALF, a hop of 4096 samples
GUARD = 256 * 1024 // 8                              # float64 values of a 256 KiB guard band


def dev(x, gpu):
    import torch
    return torch.from_numpy(np.array(x)).to(gpu)            # (a copy: the references are read-only)


def run(x, sr, gpu, **kw):
    """x numpy [n] or [channels, n] -> the contour [T] as numpy (Pa^2 unless db=True is passed)."""
    from modulation_mfcc_amd import praat_intensity_batch
    kw.setdefault("db", False)
    d = dev(x, gpu)
    _, P = praat_intensity_batch(d if d.dim() == 1 else d.unsqueeze(0), sr, **kw)
    return (P if d.dim() == 1 else P[0]).cpu().numpy()


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def plus_zero(a):
    return not np.ascontiguousarray(a).view(np.uint8).any()


def params(n, sr, **kw):
    from modulation_mfcc_amd import praat_intensity_params
    return praat_intensity_params(n, sr, **kw)


def tile_of(p, channels=1):
    from modulation_mfcc_amd import pint
    return pint._tile_frames(p, channels)


def raw(gpu, x3, p, centres, y, y_row, lens=None, linear=True, span=None):
    """mm_pint_* through ctypes on x3 [rows, channels, n_max] with the table ``centres`` [1 or rows, t_max], into ``y``."""
    import torch
    from modulation_mfcc_amd import _lib, pint
    rows, ch, n_max = x3.shape
    centres = np.ascontiguousarray(centres, dtype=np.int32)
    t_max = centres.shape[1]
    c = pint._c_params(p, ch, pint._span(centres, p.W, tile_of(p, ch)) if span is None else span, linear)
    d_w, d_c = dev(p.window, gpu), dev(centres, gpu)
    d_l = None if lens is None else dev(np.asarray(lens, dtype=np.int64), gpu)
    _lib.call("mm_pint_f32" if x3.dtype == torch.float32 else "mm_pint_f64", gpu, C.byref(c), x3.data_ptr(), rows, n_max,
              x3.stride(0), x3.stride(1), d_w.data_ptr(), d_c.data_ptr(), t_max, 0 if centres.shape[0] == 1 else t_max,
              None if d_l is None else d_l.data_ptr(), y.data_ptr(), y_row)
    torch.cuda.synchronize()


def raw_frames(gpu, x, p, centres, lens=None, linear=True, span=None):
    """x numpy [n] or [channels, n] and one list of centres -> [len(centres)] numpy."""
    import torch
    d = dev(np.atleast_2d(x), gpu).unsqueeze(0)
    y = torch.full((1, len(centres)), 7.0, dtype=torch.float64, device=gpu)
    raw(gpu, d, p, np.asarray(centres)[None, :], y, len(centres), lens, linear, span)
    return y[0].cpu().numpy()


# ---- values -------------------------------------------------------------------------------------------------------------------
SHAPES = [(8000, 129, P400, 1), (8000, 130, P400, 1), (8000, 1000, P400, 55), (8000, 2180, P400, 129), (44100, 8820, {}, 18),
          (8000, 2000, DENSE, 1574)]


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("channels", [1, 2, 3])
@pytest.mark.parametrize("case", SHAPES, ids=lambda c: f"{c[0]}x{c[1]}")
def test_shapes_per_frame(gpu, case, channels, dtype):
    sr, n, kw, T = case
    p = params(n, sr, **kw)
    assert p.T == T
    if n == 2180:
        assert (T - 1) % tile_of(p, channels) == 0                          # the last tile holds one frame
    x = O.noise(n + channels, n, channels=channels, dtype=dtype)
    got = run(x, sr, gpu, **kw)
    O.check(got, x, sr, what=f"{channels} ch", **kw)
    from modulation_mfcc_amd import praat_intensity_batch
    times, db = praat_intensity_batch(dev(x, gpu).unsqueeze(0), sr, **kw)
    assert np.array_equal(times, O.geometry(n, sr, **kw)["times"]) and db.shape == (1, T)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_the_largest_half_width(gpu, dtype):
    from modulation_mfcc_amd import _lib
    n = 32769 + 3 * 4096
    p = params(n, 48000, **MAXHW)
    assert p.hw == _lib.MM_PINT_MAX_HALF == 16384 and p.T == 4 and p.hops == [4096]
    x = O.noise(9, n, channels=2, dtype=dtype)
    O.check(run(x, 48000, gpu, **MAXHW), x, 48000, what="hw 16384", **MAXHW)


def test_frames_outside_the_staged_copy(gpu):
    """A table whose entries lie far apart: the copy holds the frames near the lowest centre, the others are read from
    memory -- the same bits as each frame alone, from the copy (span = the window) and from memory (span = 0)."""
    n = 40000
    p = params(n, 8000, **P400)
    x = O.noise(11, n, channels=2, dtype=np.float64)
    centres = [100, 39000, 20000, 130, 64, 39935, 9000, 9016, 9032, 150, 30000, 30001, 30002, 12000, 166, 182, 198]
    got = raw_frames(gpu, x, p, centres)
    O.check_frames(got, x, n, p.hw, p.window, centres, what="scattered table")
    for span in (0, p.W):
        alone = np.concatenate([raw_frames(gpu, x, p, [c], span=span) for c in centres])
        assert same_bits(got, alone), span


def test_a_dense_table_that_repeats_and_skips_centres(gpu):
    """Where the window is a whole number of sample periods and n - T is odd, (t_k - x1) / dx + 0.5 falls on whole numbers
    and its rounding makes the table of a frame per sample repeat and skip centres (44.1 kHz / 120 Hz does).  Such entries
    take the frame of their centre, with the bits of that frame alone; a centre 8 or more from the group's lowest too."""
    n = 3000
    p = params(n, 8000, **DENSE)
    x = O.noise(12, n, channels=2, dtype=np.float32)
    rng = np.random.default_rng(3)
    centres = 400 + np.arange(256) + rng.integers(0, 2, 256)
    centres[40:48] = [440, 441, 449, 443, 444, 452, 446, 447]            # two entries beyond the eight frames
    centres[48:56] = centres[48:56][::-1]                                 # out of order
    got = raw_frames(gpu, x, p, centres)
    assert set(np.diff(centres[:40]).tolist()) == {0, 1, 2}
    O.check_frames(got, x, n, p.hw, p.window, centres, what="repeats and skips")
    every = raw_frames(gpu, x, p, np.arange(400, 660))                     # a frame per sample, in order
    assert same_bits(got, every[centres - 400])
    alone = np.concatenate([raw_frames(gpu, x, p, [c], span=0) for c in centres[36:60]])
    assert same_bits(got[36:60], alone)


@pytest.mark.parametrize("case", [(8000, 1000, P400), (8000, 2000, DENSE), (44100, 8820, {})], ids=lambda c: f"{c[0]}x{c[1]}")
def test_float32_samples_are_the_float64_entry_on_the_widened_samples(gpu, case):
    sr, n, kw = case
    x = O.noise(21, n, channels=2, dtype=np.float32)
    for db in (False, True):
        assert same_bits(run(x, sr, gpu, db=db, **kw), run(x.astype(np.float64), sr, gpu, db=db, **kw)), db


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("kw", [P400, DENSE], ids=["sparse", "dense"])
def test_quiet_frames_under_a_60_db_ramp(gpu, kw, dtype):
    n = 4000
    x = (O.noise(3, n, dtype=np.float64) * 10.0 ** (-3.0 * np.arange(n) / n)).astype(dtype)
    got = run(x, 8000, gpu, **kw)
    assert got[-1] < got[0] * 1e-4
    O.check(got, x, 8000, what="60 dB ramp", **kw)             # per frame, relative to the frame's own value


@pytest.mark.parametrize("kw", [P400, DENSE], ids=["sparse", "dense"])
def test_a_large_offset(gpu, kw):
    n = 2000
    x = 1000.0 + 0.01 * np.random.default_rng(2).standard_normal(n)
    O.check(run(x, 8000, gpu, **kw), x, 8000, what="offset 1000, centred", **kw)
    keep = dict(kw, subtract_mean=False)
    got = run(x, 8000, gpu, **keep)
    assert (got > 9.9e5).all()
    O.check(got, x, 8000, what="offset 1000, mean kept", **keep)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("kw", [P400, DENSE], ids=["sparse", "dense"])
def test_silence(gpu, kw, dtype):
    x = np.zeros((2, 1500), dtype=dtype)
    assert (run(x, 8000, gpu, db=True, **kw) == -300.0).all()
    assert plus_zero(run(x, 8000, gpu, db=False, **kw))
    const = np.full(1500, 0.25, dtype=dtype)                   # a constant sound, centred: no power either
    assert (run(const, 8000, gpu, db=True, **kw) == -300.0).all()


@pytest.mark.parametrize("kw", [P400, DENSE], ids=["sparse", "dense"])
def test_db_against_the_linear_output(gpu, kw):
    x = O.noise(5, 3000, dtype=np.float64) * 10.0 ** (-3.0 * np.arange(3000) / 3000)
    P, db = run(x, 8000, gpu, db=False, **kw), run(x, 8000, gpu, db=True, **kw)
    want = 10 * np.log10(P / 4e-10)
    ulps = np.abs(db - want) / np.spacing(np.abs(want))
    print(f"pint dB against numpy's log10 of the kernel's own power: {ulps.max():.2f} float64 spacings at the most")
    assert ulps.max() <= 8


# ---- the C ABI: clipped windows, entries the kernel does not trust, lengths -----------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("kw", [P400, dict(minimum_pitch=120.0)], ids=["hw64", "hw213"])
def test_clipped_windows_and_untrusted_entries(gpu, kw, dtype):
    n = 1200
    p = params(n, 8000, **kw)
    hw = p.hw
    x = O.noise(6, n, channels=2, dtype=dtype)
    centres = [0, hw - 1, n - 1, n - hw, -1, n, hw, n - hw - 1, 2 ** 31 - 1, -2 ** 31, 1, n - 2]
    got = raw_frames(gpu, x, p, centres)
    O.check_frames(got, x, n, hw, p.window, centres, what="clipped windows")
    assert plus_zero(got[[4, 5, 8, 9]]) and (got[[0, 1, 2, 3, 6, 7, 10, 11]] > 0).all()
    # a length below n_max: NaN at and behind it changes no bit, centres at or behind it give +0.0
    m = 700
    xn = x.copy()
    xn[:, m:] = np.nan
    cl = [0, hw - 1, m - 1, m - hw, m, m + 5, 300, n - 1]
    a = raw_frames(gpu, xn, p, cl, lens=[m])
    b = raw_frames(gpu, x[:, :m], p, cl)
    assert same_bits(a, b) and plus_zero(a[[4, 5, 7]]) and np.isfinite(a).all()
    O.check_frames(a, x[:, :m], m, hw, p.window, cl, what="a length below n_max")
    # in dB an entry without a frame is +0.0 too
    assert plus_zero(raw_frames(gpu, x, p, [-1, n], linear=False))


def test_guard_bands_and_every_value_written(gpu):
    import torch
    n, rows = 2000, 3
    for kw in (P400, DENSE):
        p = params(n, 8000, **kw)
        t_max = p.T + 5                                          # five entries of -1 behind the frames
        table = np.full((1, t_max), -1, dtype=np.int32)
        table[0, :p.T] = p.centres
        x = dev(O.noise(8, n, channels=rows, dtype=np.float32)[:, None, :], gpu)
        buf = torch.full((2 * GUARD + rows * t_max,), -7.25, dtype=torch.float64, device=gpu)
        y = buf[GUARD:GUARD + rows * t_max]
        raw(gpu, x, p, table, y, t_max)
        out = buf.cpu().numpy()
        assert (out[:GUARD] == -7.25).all() and (out[GUARD + rows * t_max:] == -7.25).all()
        body = out[GUARD:GUARD + rows * t_max].reshape(rows, t_max)
        assert (body[:, :p.T] > 0).all() and plus_zero(body[:, p.T:])


# ---- independence ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("case", [(8000, 1000, P400), (8000, 1500, DENSE), (44100, 8820, {})], ids=lambda c: f"{c[0]}x{c[1]}")
def test_a_row_is_independent_of_the_batch_the_strides_and_the_table(gpu, case, dtype):
    import torch
    from modulation_mfcc_amd import praat_intensity_batch
    sr, n, kw = case
    p = params(n, sr, **kw)
    rows, ch = 70, 2
    x = O.noise(31, n, channels=ch, dtype=dtype)
    alone = run(x, sr, gpu, **kw)
    rng = np.random.default_rng(1)
    batch = (0.1 * rng.standard_normal((rows, ch, n))).astype(dtype)
    batch[41] = x
    d = dev(batch, gpu)
    _, P = praat_intensity_batch(d, sr, db=False, **kw)
    assert same_bits(P[41].cpu().numpy(), alone)
    # padded row and channel strides
    wide = torch.full((rows, ch + 1, n + 37), float("nan"), dtype=d.dtype, device=gpu)
    wide[:, :ch, :n] = d
    _, Pw = praat_intensity_batch(wide[:, :ch, :n], sr, db=False, **kw)
    assert same_bits(Pw.cpu().numpy(), P.cpu().numpy())
    # one shared table or a table per row, through the C ABI
    y1 = torch.empty((rows, p.T), dtype=torch.float64, device=gpu)
    y2 = torch.empty_like(y1)
    raw(gpu, d, p, p.centres[None, :], y1, p.T)
    raw(gpu, d, p, np.repeat(p.centres[None, :], rows, axis=0), y2, p.T)
    assert same_bits(y1.cpu().numpy(), P.cpu().numpy()) and same_bits(y2.cpu().numpy(), P.cpu().numpy())
    # the same frames behind 1, 3 and tile - 1 leading entries of -1: another place in the tile, the same bits
    tile = tile_of(p, ch)
    for shift in (1, 3, tile - 1):
        table = np.concatenate([np.full(shift, -1, dtype=np.int32), p.centres])
        got = raw_frames(gpu, x, p, table)
        assert plus_zero(got[:shift]) and same_bits(got[shift:], alone), shift


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_a_ragged_batch_equals_each_clip_alone(gpu, dtype):
    import torch
    from modulation_mfcc_amd import praat_intensity_ragged_batch, praat_intensity_list
    W = params(1000, 8000, **P400).W
    lens = [W, W + 1, 1000, 2000]
    clips = [O.noise(40 + i, n, dtype=dtype) for i, n in enumerate(lens)]
    x = np.full((4, 2000), np.nan, dtype=dtype)
    for i, c in enumerate(clips):
        x[i, :c.size] = c
    frames, t1, P = praat_intensity_ragged_batch(dev(x, gpu), lens, 8000, db=False, **P400)
    P = P.cpu().numpy()
    Ts = [O.geometry(n, 8000, **P400)["T"] for n in lens]
    assert frames.tolist() == Ts and Ts[:3] == [1, 1, 55] and P.shape == (4, max(Ts))
    for i, c in enumerate(clips):
        g = O.geometry(c.size, 8000, **P400)
        assert same_bits(P[i, :g["T"]], run(c, 8000, gpu, **P400)) and plus_zero(P[i, g["T"]:]) and t1[i] == g["t1"]
        O.check(P[i, :g["T"]], c, 8000, what=f"ragged clip {i}", **P400)
    # lengths on the device: never read back, the same frames, the same bits
    d_len = torch.tensor(lens, dtype=torch.int64, device=gpu)
    fd, td, Pd = praat_intensity_ragged_batch(dev(x, gpu), d_len, 8000, db=False, **P400)
    assert fd.is_cuda and td.is_cuda and fd.cpu().tolist() == frames.tolist() and np.array_equal(td.cpu().numpy(), t1)
    assert same_bits(Pd.cpu().numpy(), P)
    # 64 lengths, those at which (dur - phys) / dt is a whole number in exact arithmetic among them: the device's table is
    # the host's (frame counts, t1, every centre: the same bits out)
    many = np.concatenate([128 + 16 * np.arange(1, 33), np.random.default_rng(7).integers(129, 2001, 32)]).astype(np.int64)
    xm = dev(np.tile(x[3], (64, 1)), gpu)
    fh, th, Ph = praat_intensity_ragged_batch(xm, many, 8000, db=False, **P400)
    fd, td, Pd = praat_intensity_ragged_batch(xm, torch.from_numpy(many).to(gpu), 8000, db=False, **P400)
    assert fd.cpu().tolist() == fh.tolist() and np.array_equal(td.cpu().numpy(), th)
    assert same_bits(Pd.cpu().numpy()[:, :Ph.shape[1]], Ph.cpu().numpy()) and plus_zero(Pd.cpu().numpy()[:, Ph.shape[1]:])
    # a clip shorter than the window: refused with its row (host lengths), a row of NaN (device lengths)
    with pytest.raises(ValueError, match=r"sound shorter than the analysis window: 100 samples .* \(row 1\)"):
        praat_intensity_ragged_batch(xm[:4], [1000, 100, 500, 2000], 8000, **P400)
    d_len = torch.tensor([1000, 100, 500, 2000], dtype=torch.int64, device=gpu)
    fd, _, Pd = praat_intensity_ragged_batch(xm[:4], d_len, 8000, db=False, **P400)       # (rows of 2000 samples, no NaN)
    Pd = Pd.cpu().numpy()
    assert fd.cpu().tolist() == [55, 0, O.geometry(500, 8000, **P400)["T"], Ts[3]] and np.isnan(Pd[1]).all() and np.isfinite(Pd[[0, 2, 3]]).all()
    # the list form: each clip what the single call gives
    out = praat_intensity_list([dev(c, gpu) for c in clips], 8000, db=False, **P400)
    for (times, y), c in zip(out, clips):
        assert same_bits(y.cpu().numpy(), run(c, 8000, gpu, **P400)) and np.array_equal(times, O.geometry(c.size, 8000, **P400)["times"])
    with pytest.raises(ValueError, match=r"\(clip 1\)"):
        praat_intensity_list([dev(clips[2], gpu), dev(clips[0][:50], gpu)], 8000, **P400)


# ---- the lookup -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [1, 2, 3, 50])
@pytest.mark.parametrize("interpolation", ["nearest", "linear", "cubic"])
def test_the_value_lookup(gpu, T, interpolation):
    from modulation_mfcc_amd import Intensity
    y = 60.0 + 10.0 * np.random.default_rng(T).standard_normal(T)
    t1, dt = 0.0321, 0.008
    inten = Intensity(values=dev(y[None, :], gpu), t1=t1, time_step=dt, n_frames=T, xmin=0.0, xmax=1.0)
    k = np.arange(T)
    times = np.concatenate([t1 + k * dt, t1 + (k[:-1] + 0.5) * dt, t1 + (k[:-1] + 0.3) * dt, t1 + (k[:-1] + 0.77) * dt,
                            [t1 - 0.49 * dt, t1 - 0.2 * dt, t1 + (T - 1 + 0.2) * dt, t1 + (T - 1 + 0.49) * dt],      # clamped
                            [t1 - 0.51 * dt, t1 - 3 * dt, t1 + (T - 1 + 0.51) * dt, t1 + (T + 5) * dt, np.nan]])  # outside
    got = inten.get_value(times, interpolation)
    assert isinstance(got, np.ndarray) and got.shape == times.shape and np.isnan(got[-5:]).all() and np.isfinite(got[:-5]).all()
    O.check_values(got, y, t1, dt, times, O.DEPTHS[interpolation], what=interpolation)
    assert np.allclose(got[:T], y, rtol=0, atol=1e-9)           # at a frame's time the frame's value
    on_dev = inten.get_value(dev(times, gpu), interpolation)
    assert on_dev.is_cuda and same_bits(on_dev.cpu().numpy(), got)
    one = inten.get_value(float(times[T]), interpolation) if T > 1 else inten.get_value(t1, interpolation)
    assert isinstance(one, float) and one == (got[T] if T > 1 else got[0])
    with pytest.raises(ValueError, match="unknown interpolation"):
        inten.get_value(t1, "sinc70")


# ---- the Python layer -------------------------------------------------------------------------------------------------------------
def test_to_intensity_and_get_value(gpu):
    from modulation_mfcc_amd import Sound, to_intensity
    sr, n = 8000, 3000
    x = O.noise(50, n, channels=2, dtype=np.float64)
    g = O.geometry(n, sr)
    want = O.level(O.references(x, sr)[0])
    for arg, rate in ((dev(x, gpu), sr), (x, sr), (Sound(None, dev(x, gpu), sr), None)):
        inten = to_intensity(arg, rate)
        assert inten.values.shape == (1, g["T"]) and inten.n_frames == g["T"] and inten.t1 == g["t1"]
        assert inten.get_time_step() == g["dt"] == 0.008 and inten.xmin == 0.0 and inten.xmax == n / sr
        assert np.array_equal(inten.xs(), g["times"])
        db = inten.values[0].cpu().numpy()
        assert np.abs(db - want).max() < 1e-9
    mono = to_intensity(dev(x[0], gpu), sr, 400.0, 0.001, False)
    assert mono.time_step == 0.001 and mono.values.shape == (1, O.geometry(n, sr, minimum_pitch=400.0, time_step=0.001)["T"])
    assert np.abs(mono.values[0].cpu().numpy() - O.level(O.intensity(x[0], sr, minimum_pitch=400.0, time_step=0.001,
                                                                      subtract_mean=False))).max() < 1e-9
    times = np.array([0.1, 0.15, 0.2004, inten.t1, 10.0])
    for kind in ("nearest", "linear", "cubic"):
        got = inten.get_value(times, kind)
        O.check_values(got, db, inten.t1, inten.time_step, times, O.DEPTHS[kind], what="to_intensity " + kind)
        assert inten.get_value(0.15, kind) == got[1] and np.isnan(inten.get_value(10.0, kind))
    assert inten.get_value(0.15) == inten.get_value(0.15, "cubic")


def test_praat_rms_envelope_takes_both_branches(gpu):
    from modulation_mfcc_amd import applyFilter, praat_rms_envelope, to_intensity
    sr, n = 8000, 6000
    x = O.noise(60, n, dtype=np.float64)
    d = dev(x, gpu)
    for min_pitch, floor, step in ((150.0, 150.0, 0.01), (100.0, 120.0, 1 / sr)):
        inten = to_intensity(d, sr, floor, step)
        amp, amp_t = praat_rms_envelope(d, sr, min_pitch, hopLen=0.01)
        assert amp.is_cuda and same_bits(amp.cpu().numpy(), inten.values[0].cpu().numpy())
        amp_sr = 1 / inten.get_time_step()
        assert np.array_equal(amp_t, np.arange(inten.n_frames) / amp_sr)
        assert inten.n_frames == O.geometry(n, sr, minimum_pitch=floor, time_step=step)["T"]
        filt, filt_t = praat_rms_envelope(d, sr, min_pitch, hopLen=0.01, outFilter="iir")
        want = applyFilter(inten.values.flatten(), amp_sr, filt="iir", filtType="low", cutOff=[12], filtLen=6, polyOrd=3)
        assert same_bits(filt.cpu().numpy(), want.cpu().numpy()) and np.array_equal(filt_t, amp_t)
        host, _ = praat_rms_envelope(x, sr, min_pitch, hopLen=0.01)
        assert isinstance(host, np.ndarray) and same_bits(host, amp.cpu().numpy())
