"""GPU: praat_spectrogram_batch / _ragged_batch / _list, Parselmouth and spectrogram_view (mm_pspec_f32 / _f64,
csrc/mm_pspec.hip) against the yardstick of tests/pspec_oracle.py: the float64 restatement of DESIGN.md section 19 within
max(1e-12, 16 r64) of the image's maximum for the float64 entry and max(16 r32, 8 float32 spacings) for the float32 one, in
the power domain, on every shape at which the kernel takes another path -- frame counts 1 and 2, fractional hops, band sums,
the last used bin, the tile edges, more tiles than resident workgroups, channels, window shapes; bit-for-bit independence
of the batch, the strides, the row's index and of what lies behind a length; the table the kernel does not trust; the
stream contract (the checks of tests/test_gpu_streams.py); the chain into zoom_batch.

Every measured error is printed before it is asserted (pytest -s shows them; docs/experiments.md lists a run)."""
import ctypes as C
import wave

import numpy as np
import pytest
import scipy.ndimage

import pspec_oracle as O
import stream_cases as S
import test_gpu_streams as TS
import zoom_oracle as ZO

pytestmark = pytest.mark.gpu

DTYPES = [np.float32, np.float64]
IDS = ["f32", "f64"]
NARROW = O.NARROW


def dev(x, gpu):
    import torch
    return torch.from_numpy(np.array(x)).to(gpu)            # (a copy: the references are read-only)


def run(x, sr, gpu, **kw):
    """x numpy [n] or [channels, n] -> the image [F, T] as numpy."""
    from modulation_mfcc_amd import praat_spectrogram_batch
    d = dev(x, gpu)
    _, _, P = praat_spectrogram_batch(d if d.dim() == 1 else d.unsqueeze(0), sr, **kw)
    return (P if d.dim() == 1 else P[0]).cpu().numpy()


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def plus_zero(a):
    return not np.ascontiguousarray(a).view(np.uint8).any()


def params(n, sr, **kw):
    from modulation_mfcc_amd import praat_spectrogram_params
    return praat_spectrogram_params(n, sr, **kw)


def tile_of(p, channels=1):
    from modulation_mfcc_amd import pspec
    return pspec._tile_frames(p, channels)


def n_for_frames(T, sr, **kw):
    """The shortest sound with T frames."""
    n = 1
    while True:
        try:
            if O.geometry(n, sr, **kw)["T"] >= T:
                return n
        except ValueError:
            pass
        n += 1


def raw(gpu, x3, p, starts, y, y_row, y_band, db=False):
    """mm_pspec_* through ctypes on x3 [rows, channels, n_max] with the table ``starts`` [1 or rows, t_max], into ``y``."""
    import torch
    from modulation_mfcc_amd import _lib, pspec
    rows, ch, n_max = x3.shape
    starts = np.ascontiguousarray(starts, dtype=np.int32)
    t_max = starts.shape[1]
    c = pspec._c_params(p, ch, pspec._span(starts, p.nw, tile_of(p, ch)), 1 if db else 0)
    d_w = dev(p.window.astype(np.float32 if x3.dtype == torch.float32 else np.float64), gpu)
    d_s = dev(starts, gpu)
    _lib.call("mm_pspec_f32" if x3.dtype == torch.float32 else "mm_pspec_f64", gpu, C.byref(c), x3.data_ptr(), rows, n_max,
              x3.stride(0), x3.stride(1), d_w.data_ptr(), d_s.data_ptr(), t_max, 0 if starts.shape[0] == 1 else t_max,
              y.data_ptr(), y_row, y_band)
    torch.cuda.synchronize()


# ---- values -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("n", [160, 161, 191, 192, 193])
def test_frame_count_and_centring(gpu, n, dtype):
    x = O.noise(n, n, dtype=dtype)
    got = run(x, 16000, gpu)
    assert got.shape == (160, 1 if n < 192 else 2)
    O.check(got, x, 16000, what="frame count")
    from modulation_mfcc_amd import praat_spectrogram_batch
    times, freqs, _ = praat_spectrogram_batch(dev(x, gpu), 16000)
    g = O.geometry(n, 16000)
    assert np.array_equal(times, g["times"]) and np.array_equal(freqs, g["freqs"])
    with pytest.raises(ValueError, match="sound shorter than the analysis window"):
        praat_spectrogram_batch(dev(x[:159], gpu), 16000)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("case", [(22050, 5000, 512, [44, 45]), (44100, 6000, 1024, [88, 89])], ids=str)
def test_fractional_hops(gpu, case, dtype):
    sr, n, nfft, hops = case
    p = params(n, sr)
    assert p.nfft == nfft and p.hops == hops
    x = O.noise(1, n, dtype=dtype)
    O.check(run(x, sr, gpu), x, sr, what="fractional hops")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("case", [(16000, 1500, 6, 958, 1024), (44100, 6000, 9, 2644, 4096)], ids=str)
def test_band_sums(gpu, case, dtype):
    sr, n, bw, nw, nfft = case
    p = params(n, sr, **NARROW)
    assert (p.bw, p.nw, p.nfft) == (bw, nw, nfft) and p.y1 > 0
    x = O.noise(2, n, dtype=dtype)
    O.check(run(x, sr, gpu, **NARROW), x, sr, what="band sums", **NARROW)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_the_top_band_on_the_last_used_bin(gpu, dtype):
    p = params(1000, 8000)
    assert p.n_freqs * p.bw == p.nfft // 2 == 128
    x = O.noise(4, 1000, dtype=dtype)
    x += (0.2 * np.cos(np.pi * np.arange(1000) * (1 - 1 / 128))).astype(dtype)      # power in the top band
    O.check(run(x, 8000, gpu), x, 8000, what="top band")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("where", ["tile-1", "tile", "tile+1", "3tiles+1"])
def test_tile_edges(gpu, where, dtype):
    sr = 22050
    tile = tile_of(params(5000, sr))
    T = {"tile-1": tile - 1, "tile": tile, "tile+1": tile + 1, "3tiles+1": 3 * tile + 1}[where]
    n = n_for_frames(T, sr)
    p = params(n, sr)
    assert p.n_frames == T and tile == 32 and p.n_freqs == 116 and (p.n_freqs * tile) % 256
    x = O.noise(T, n, dtype=dtype)
    O.check(run(x, sr, gpu), x, sr, what=f"T = {where}")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_a_thirty_second_clip(gpu, dtype):
    import torch
    sr, n = 44100, 30 * 44100
    p = params(n, sr)
    tiles = -(-p.n_frames // tile_of(p))
    cus = torch.cuda.get_device_properties(gpu).multi_processor_count
    # 469 tiles: more than the float64 kernel's resident workgroups (its LDS admits one per compute unit) and more than one
    # per compute unit for the float32 kernel (three resident at the most); first samples beyond 2^20
    assert tiles > 1.5 * cus and int(p.starts[-1]) > 1 << 20, (tiles, cus)
    x = O.noise(30, n, dtype=dtype)
    O.check(run(x, sr, gpu), x, sr, what="30 s")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("channels", [1, 2, 3])
def test_channels_mean_of_powers(gpu, channels, dtype):
    x = O.noise(channels, 2000, channels=channels, dtype=dtype)
    got = run(x, 16000, gpu)
    e, b = O.check(got, x, 16000, what=f"{channels} channels")
    if channels > 1:                                     # not the power of the mean: that is another image altogether
        mono = O.spectrogram(x.astype(np.float64).mean(axis=0), 16000)
        assert O.error(got, mono) > 1000 * b


@pytest.mark.parametrize("shape", O.SHAPES)
def test_each_window_shape(gpu, shape):
    for dtype in DTYPES:
        x = O.noise(7, 1000, dtype=dtype)
        O.check(run(x, 16000, gpu, window_shape=shape), x, 16000, what=shape, window_shape=shape)


def test_the_db_flag_and_silence(gpu):
    from modulation_mfcc_amd import praat_spectrogram_batch
    for dtype in DTYPES:
        x = O.noise(9, 1000, dtype=dtype)
        P = run(x, 16000, gpu)
        dB = run(x, 16000, gpu, db=True)
        assert dB.dtype == dtype and np.isfinite(dB).all()
        O.check((10.0 ** (dB.astype(np.float64) / 10)).astype(dtype), x, 16000, what="through dB")
        assert np.abs(dB - 10 * np.log10(P.astype(np.float64))).max() <= 2 * np.spacing(dtype(np.abs(dB).max()))
        z = np.zeros(1000, dtype=dtype)
        assert plus_zero(run(z, 16000, gpu)), "a silent clip has exactly no power"
        with np.errstate(divide="ignore"):
            assert same_bits(run(z, 16000, gpu, db=True), (10 * np.log10(np.zeros((160, 27)))).astype(dtype))     # -inf


# ---- independence ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_strides(gpu, dtype):
    import torch
    from modulation_mfcc_amd import praat_spectrogram_batch
    sr, n = 16000, 1200
    x = O.noise(11, 1500, channels=6, dtype=dtype).reshape(2, 3, 1500)
    wide = dev(x, gpu)
    want = praat_spectrogram_batch(wide[:, :, :n].contiguous(), sr)[2].cpu().numpy()
    for b in range(2):
        O.check(want[b], x[b, :, :n], sr, what="strides, contiguous")
    view = wide[:, :, :n]                                    # a channel stride larger than n
    assert view.stride() == (4500, 1500, 1)
    assert same_bits(praat_spectrogram_batch(view, sr)[2].cpu().numpy(), want)
    rows = wide[:, 1, :n]                                    # a row view of a wider tensor: [2, n] with a pitch of 4500
    assert rows.stride() == (4500, 1)
    mono = praat_spectrogram_batch(rows, sr)[2].cpu().numpy()
    assert same_bits(mono, praat_spectrogram_batch(rows.contiguous(), sr)[2].cpu().numpy())
    assert same_bits(mono[1], run(x[1, 1, :n], sr, gpu))
    t = wide[0, :, :n].t().contiguous().t()                  # a strided last axis: copied
    assert t.stride(1) != 1
    assert same_bits(praat_spectrogram_batch(t.unsqueeze(0), sr)[2][0].cpu().numpy(), want[0])
    # the row's index and the batch do not matter
    many = torch.cat([wide[:, :, :n]] * 3)[[5, 0, 3, 1]]
    got = praat_spectrogram_batch(many, sr)[2].cpu().numpy()
    assert same_bits(got[0], want[1]) and same_bits(got[1], want[0]) and same_bits(got[2], want[1]) and same_bits(got[3], want[1])


RAG_SR = 22050


def _ragged_lengths():
    return [n_for_frames(97, RAG_SR), n_for_frames(1, RAG_SR), n_for_frames(32, RAG_SR), n_for_frames(33, RAG_SR),
            n_for_frames(2, RAG_SR) - 1]


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_ragged(gpu, dtype):
    import torch
    from modulation_mfcc_amd import praat_spectrogram_batch, praat_spectrogram_ragged_batch, praat_spectrogram_list
    lens = _ragged_lengths()
    n_max = max(lens)
    x = O.noise(13, n_max, channels=len(lens), dtype=dtype)
    d = dev(x, gpu)
    frames, t1, freqs, P = praat_spectrogram_ragged_batch(d, lens, RAG_SR)
    assert frames.tolist() == [97, 1, 32, 33, 1] and P.shape == (5, 116, 97) and P.dtype == d.dtype
    P = P.cpu().numpy()
    alone = []
    for b, n in enumerate(lens):
        times, f1, Pb = praat_spectrogram_batch(d[b, :n], RAG_SR)
        alone.append(Pb.cpu().numpy())
        assert same_bits(P[b, :, :frames[b]], alone[b]), f"clip {b} is not the clip alone"
        assert plus_zero(P[b, :, frames[b]:]), f"clip {b}: +0.0 behind its frames"
        assert t1[b] == times[0] == O.geometry(n, RAG_SR)["t1"] and np.array_equal(freqs, f1)
        O.check(alone[b], x[b, :n], RAG_SR, what=f"ragged clip {b}")
    # any batch order
    perm = [3, 1, 4, 0, 2]
    f2, _, _, P2 = praat_spectrogram_ragged_batch(d[perm], [lens[i] for i in perm], RAG_SR)
    assert f2.tolist() == [frames[i] for i in perm] and same_bits(P2.cpu().numpy(), P[perm])
    # NaN behind every length changes nothing
    xn = x.copy()
    for b, n in enumerate(lens):
        xn[b, n:] = np.nan
    assert same_bits(praat_spectrogram_ragged_batch(dev(xn, gpu), np.array(lens), RAG_SR)[3].cpu().numpy(), P)
    # guard rows and guard columns around the output come back intact
    p = params(n_max, RAG_SR)
    starts = np.full((5, 97), -1, np.int32)
    for b, n in enumerate(lens):
        starts[b, :frames[b]] = params(n, RAG_SR).starts
    pitch = 97 + 3
    buf = torch.empty((7, 116, pitch), dtype=d.dtype, device=gpu)
    buf.view(torch.uint8).fill_(0xFF)
    raw(gpu, dev(xn, gpu).unsqueeze(1), p, starts, buf[1], 116 * pitch, pitch)
    out = buf.cpu().numpy()
    assert same_bits(out[1:6, :, :97], P)
    guards = np.ascontiguousarray(out).view(np.uint8).reshape(7, 116, pitch, -1)
    assert (guards[0] == 0xFF).all() and (guards[6] == 0xFF).all() and (guards[1:6, :, 97:] == 0xFF).all()
    # the list front end: each clip what it is alone
    res = praat_spectrogram_list([d[b, :n] for b, n in enumerate(lens)], RAG_SR)
    for b, (times, f1, Pb) in enumerate(res):
        assert same_bits(Pb.cpu().numpy(), alone[b]) and np.array_equal(times, O.geometry(lens[b], RAG_SR)["times"])
    # refusals name the clip, before any launch
    with pytest.raises(ValueError, match=r"sound shorter than the analysis window: 100 samples .*\(clip 2\)"):
        praat_spectrogram_ragged_batch(d, [lens[0], lens[1], 100, lens[3], lens[4]], RAG_SR)
    with pytest.raises(ValueError, match=r"\(clip 1\)"):
        praat_spectrogram_list([d[0, :lens[0]], d[1, :50]], RAG_SR)
    with pytest.raises(NotImplementedError, match="host lengths: the frame table"):
        praat_spectrogram_ragged_batch(d, dev(np.array(lens, dtype=np.int64), gpu), RAG_SR)
    with pytest.raises(ValueError, match=r"lengths must lie in \[1, "):
        praat_spectrogram_ragged_batch(d, [lens[0] + 1] + lens[1:], RAG_SR)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_a_nan_sample_reaches_its_frames_and_no_others(gpu, dtype):
    n, at = 3000, 1234
    x = O.noise(17, n, dtype=dtype)
    clean = run(x, 16000, gpu)
    x[at] = np.nan
    got = run(x, 16000, gpu)
    p = params(n, 16000)
    hit = (p.starts <= at) & (at < p.starts + p.nw)
    assert 3 <= hit.sum() < p.n_frames // 2
    assert not np.isfinite(got[:, hit]).any() and same_bits(got[:, ~hit], clean[:, ~hit])


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_the_kernel_trusts_no_table_entry(gpu, dtype):
    import torch
    n = 3000
    x = O.noise(19, n, dtype=dtype)
    clean = run(x, 16000, gpu)
    p = params(n, 16000)
    assert p.n_frames == 89                                  # three tiles
    starts = p.starts.copy()[None, :]
    bad = {5: -7, 40: -1, 41: n - p.nw + 1, 70: 2 ** 31 - 1, 71: n}
    for k, s in bad.items():
        starts[0, k] = s
    starts[0, 20] = 0                                        # a valid entry out of order: the frame at sample 0
    y = torch.empty((1, p.n_freqs, p.n_frames), dtype=dev(x, gpu).dtype, device=gpu)
    y.view(torch.uint8).fill_(0xFF)
    raw(gpu, dev(x, gpu).reshape(1, 1, n), p, starts, y, p.n_freqs * p.n_frames, p.n_frames)
    got = y[0].cpu().numpy()
    keep = np.ones(p.n_frames, bool)
    keep[list(bad) + [20]] = False
    assert plus_zero(got[:, list(bad)]), "a refused entry is +0.0 in every band"
    assert same_bits(got[:, keep], clean[:, keep]), "the neighbours are intact"
    first = p.starts.copy()[None, :]
    first[0, 0] = 0
    raw(gpu, dev(x, gpu).reshape(1, 1, n), p, first, y, p.n_freqs * p.n_frames, p.n_frames)
    assert same_bits(got[:, 20], y[0, :, 0].cpu().numpy())   # the same frame in another place: the same bits
    # a table whose every entry is refused
    raw(gpu, dev(x, gpu).reshape(1, 1, n), p, np.full((1, p.n_frames), -1, np.int32), y, p.n_freqs * p.n_frames, p.n_frames)
    assert plus_zero(y.cpu().numpy())


# ---- the stream contract of mm_pspec_f32 / _f64 -----------------------------------------------------------------------------------
# Built with the registry's Case class, NOT appended to stream_cases.CASES (pinned to include/modmfcc.h); the checks are those
# of test_gpu_streams.py.  3 clips of 2 channels, 3000 samples at 22 050 Hz: 64 frames, two tiles, fractional hops.
S_B, S_C, S_N, S_SR = 3, 2, 3000, 22050
S_LENS = [3000, 221, 1700]


def _data(name, dtype):
    return {"x": tuple(S._seed(name, k).standard_normal((S_B, S_C, S_N)).astype(dtype) for k in (0, 1))}


def _wrapper_case(ragged, dtype):
    name = f"pspec/{'ragged-' if ragged else ''}wrapper-{np.dtype(dtype).name}"
    entry = "mm_pspec_" + ("f32" if dtype == np.float32 else "f64")

    def setup(env):
        from modulation_mfcc_amd import praat_spectrogram_batch, praat_spectrogram_ragged_batch
        if ragged:
            return lambda: praat_spectrogram_ragged_batch(env.buf["x"], S_LENS, S_SR)[3]
        return lambda: praat_spectrogram_batch(env.buf["x"], S_SR)[2]
    return S.Case(name, entry, "pspec", lambda: _data(name, dtype), setup)


def _ctypes_case(dtype):
    name = f"pspec/ctypes-{np.dtype(dtype).name}"
    entry = "mm_pspec_" + ("f32" if dtype == np.float32 else "f64")

    def setup(env):
        from modulation_mfcc_amd import _lib, pspec
        lib = _lib.load()
        x = env.buf["x"]
        p = pspec.praat_spectrogram_params(S_N, S_SR, **NARROW)
        c = pspec._c_params(p, S_C, pspec._span(p.starts[None, :], p.nw, pspec._tile_frames(p, S_C)), 0)
        d_w = dev(p.window.astype(dtype), env.gpu)
        d_s = dev(p.starts, env.gpu)
        env.keep += [d_w, d_s, c]
        y = env.out((S_B, p.n_freqs, p.n_frames), x.dtype)
        fn = getattr(lib, entry)

        def call():
            _lib.check(fn(C.byref(c), x.data_ptr(), S_B, S_N, S_C * S_N, S_N, d_w.data_ptr(), d_s.data_ptr(), p.n_frames, 0,
                          y.data_ptr(), p.n_freqs * p.n_frames, p.n_frames, S.stream()), entry)
            return y
        return call
    return S.Case(name, entry, "pspec", lambda: _data(name, dtype), setup, threads=True)


STREAM_CASES = [_wrapper_case(False, np.float32), _wrapper_case(True, np.float64), _ctypes_case(np.float64),
                _ctypes_case(np.float32)]
_SESSION = []


@pytest.fixture(scope="module")
def stream_session(gpu):
    if not _SESSION:
        _SESSION.append(TS.Session(gpu, cases=STREAM_CASES))
    return _SESSION[0]


def test_the_stream_cases_are_not_in_the_registry():
    assert not {c.name for c in S.CASES} & {c.name for c in STREAM_CASES}
    assert {c.entry for c in STREAM_CASES} == {"mm_pspec_f32", "mm_pspec_f64"}
    assert O.geometry(S_N, S_SR)["T"] == 64 and [O.geometry(n, S_SR)["T"] for n in S_LENS] == [64, 1, 34]


@pytest.mark.parametrize("case", STREAM_CASES, ids=lambda c: c.name)
def test_behind_a_gate_on_a_side_stream(case, stream_session):
    e = stream_session.get(case)
    assert e.reproducible, "two eager calls on the same data differ in a bit"
    TS.test_side_stream_order_and_asynchrony(case, stream_session)


@pytest.mark.parametrize("case", STREAM_CASES, ids=lambda c: c.name)
def test_captured_and_replayed_four_times(case, stream_session):
    TS.test_capture_and_replay(case, stream_session)


@pytest.mark.parametrize("case", [c for c in STREAM_CASES if c.threads], ids=lambda c: c.name)
def test_two_threads(case, stream_session, gpu):
    TS.test_one_plan_two_threads(case, stream_session, gpu)


def test_the_stream_cases_compute_what_the_yardstick_says(gpu, stream_session):
    for case, dtype, kw in ((STREAM_CASES[0], np.float32, {}), (STREAM_CASES[2], np.float64, NARROW)):
        e = stream_session.get(case)
        x = _data(case.name, dtype)["x"][1]
        got = e.eager[1][0].cpu().numpy()
        for b in range(S_B):
            O.check(got[b], x[b], S_SR, what=case.name, **kw)


# ---- the chain --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_spectrogram_view_is_the_chain(gpu, dtype):
    from modulation_mfcc_amd import praat_spectrogram_batch, spectrogram_view, zoom_batch
    sr, n = 16000, 1000
    x = O.noise(23, n, dtype=dtype)
    d = dev(x, gpu)
    P = praat_spectrogram_batch(d, sr)[2]
    xg, yg, img = spectrogram_view(d, sr)
    g = O.geometry(n, sr)
    assert np.array_equal(xg, g["x_grid"]) and np.array_equal(yg, g["y_grid"])
    assert same_bits(img.cpu().numpy(), zoom_batch(P, 6, order=4, db=True).cpu().numpy())
    raw_img = spectrogram_view(d, sr, zoom_blur=False)[2]
    assert same_bits(raw_img.cpu().numpy(), praat_spectrogram_batch(d, sr, db=True)[2].cpu().numpy())
    # against scipy on the entry's own power, within the zoom's bound
    db64 = 10 * np.log10(P.cpu().numpy().astype(np.float64))
    want64 = scipy.ndimage.zoom(db64, 6, order=4)
    _, outside, _, sp = ZO.reference(db64, 6, 4)
    bound = ZO.bound_of(sp, dtype, float(np.abs(want64).max()))
    got = img.cpu().numpy()
    assert got.dtype == dtype and got.shape == want64.shape == (960, 6 * g["T"])
    c = ZO.measure(got[~outside], want64.astype(dtype)[~outside])
    print(f"spectrogram_view {np.dtype(dtype).name}: c = {c:.3e}, bound = {bound:.3e}")
    assert c <= bound
    stereo = O.noise(29, n, channels=2, dtype=dtype)
    v2 = spectrogram_view(dev(stereo, gpu), sr)[2]
    assert same_bits(v2.cpu().numpy(), zoom_batch(praat_spectrogram_batch(dev(stereo, gpu).unsqueeze(0), sr)[2][0], 6, order=4,
                                                  db=True).cpu().numpy())


def test_parselmouth_on_a_stereo_wave_file(gpu, tmp_path):
    from modulation_mfcc_amd import Parselmouth, Sound, Spectrogram, spectrogram_view, zoom_batch
    sr, n = 22050, 4000
    pcm = np.clip(O.noise(31, n, channels=2, dtype=np.float64, amp=0.2) * 32768, -32768, 32767).astype("<i2")
    path = tmp_path / "stereo.wav"
    with wave.open(str(path), "wb") as f:
        f.setnchannels(2)
        f.setsampwidth(2)
        f.setframerate(sr)
        f.writeframes(np.ascontiguousarray(pcm.T).tobytes())
    decoded = (pcm.astype(np.float32) / np.float32(32768))               # the decoder's samples (tests/test_gpu_pcm.py)
    pm = Parselmouth(str(path))
    snd = pm.get_sound()
    assert isinstance(snd, Sound) and snd.sample_rate == sr and tuple(snd.amplitudes.shape) == (2, n)
    assert same_bits(snd.amplitudes.cpu().numpy(), decoded)
    assert np.array_equal(snd.timestamps, 0.5 / sr + np.arange(n) / sr) or np.allclose(snd.timestamps, (np.arange(n) + 0.5) / sr,
                                                                                         rtol=0, atol=1e-15)
    sp = pm.get_spectrogram()
    g = O.geometry(n, sr)
    assert isinstance(sp, Spectrogram) and np.array_equal(sp.timestamps, g["x_grid"]) and np.array_equal(sp.frequencies, g["y_grid"])
    dB = sp.data_matrix.cpu().numpy()
    assert dB.dtype == np.float32 and dB.shape == (g["F"], g["T"])
    O.check((10.0 ** (dB.astype(np.float64) / 10)).astype(np.float32), decoded, sr, what="Parselmouth.get_spectrogram")
    xg, yg, img = spectrogram_view(path)
    assert np.array_equal(xg, g["x_grid"]) and tuple(img.shape) == (6 * g["F"], 6 * g["T"])
