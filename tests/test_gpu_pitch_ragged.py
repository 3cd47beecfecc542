"""GPU: the ragged pYIN path -- pyin_ragged_batch (mm_pyin_ragged_f32 / _f64), interp_nan_ragged_batch
(mm_interp_nan_linear_ragged_f64 / mm_interp_nan_ragged_f64) and get_f0_batch.

The criterion is exactness: a ragged row runs the kernels and the arithmetic of the clip alone, so every comparison with
the single-clip call is torch.equal after nan_to_num, with no tolerance.  The single-clip call is pinned to the oracle
by tests/test_gpu_pitch.py and tests/test_gpu_pitch_params.py; test_oracle_anchor repeats that anchor on ragged rows.

Shapes: C5 of tests/test_gpu_pitch_params.py (frame_length 512, hop 40, 100..500 Hz at 8 kHz, 16 frames per CMND tile)
unless stated.  Every single-clip result is computed once (``_alone``) and shared."""
import ctypes as C

import numpy as np
import pytest
import torch

import pyin_oracle as O
import test_gpu_pitch_params as P
from modulation_mfcc_amd import (_lib, get_f0, get_f0_batch, interp_nan_batch, interp_nan_ragged_batch, pitch, pyin_batch,
                                 pyin_ragged_batch, pyin_ragged_frames)

pytestmark = pytest.mark.gpu

C5, SR = P.C5, P.C5_SR
DTYPES = [np.float32, np.float64]
NAMES = ("f0", "voiced", "voiced_prob", "states")
LENGTHS = [4000, 1, 39, 40, 80, 599, 600, 640, 3999]
FRAMES = [101, 1, 1, 2, 3, 15, 16, 17, 100]
VOICED = {599: 14, 600: 15, 640: 16, 3999: 74, 4000: 75}          # voiced frames of the glide clips (the oracle's)


def _dev(y, gpu):
    return torch.from_numpy(np.ascontiguousarray(y)).to(gpu)


def _nn(t):
    return torch.nan_to_num(t.double(), nan=-1.0, posinf=-2.0, neginf=-3.0)


def _clips(dtype, lengths=LENGTHS):
    """The lengths cut from the glide at offset 2000, then from noise."""
    g = O.synth("glide", SR, 1.0, dtype)
    z = O.synth("noise", SR, 1.0, dtype, seed=5)
    return [g[2000:2000 + n] for n in lengths] + [z[:n] for n in lengths]


def _packed(clips, gpu, fill=0.0, extra=0):
    """[B, n_max + extra] with ``fill`` behind every clip ('next': the samples of the next clip, repeated)."""
    n_max = max(len(c) for c in clips) + extra
    rows = np.empty((len(clips), n_max), dtype=clips[0].dtype)
    for b, c in enumerate(clips):
        rows[b, :len(c)] = c
        rows[b, len(c):] = np.resize(clips[(b + 1) % len(clips)], n_max - len(c)) if isinstance(fill, str) else fill
    return _dev(rows, gpu)


_ALONE = {}


def _alone(gpu, clip, **kw):
    """pyin_batch of one clip with its states; cached, callers must not modify the result."""
    key = (clip.dtype.str, clip.tobytes(), tuple(sorted((k, str(v)) for k, v in kw.items())))
    if key not in _ALONE:
        _ALONE[key] = pyin_batch(_dev(clip, gpu), SR, return_states=True, **kw)
    return _ALONE[key]


def _assert_rows_equal_alone(gpu, out, clips, frames=None, **kw):
    """out = (f0, voiced, voiced_prob, frames, states) of a ragged call: every row is the clip alone, zeros behind."""
    f0, v, vp, fr, s = out
    fr = fr.cpu().numpy()
    for b, c in enumerate(clips):
        one = _alone(gpu, c, **kw)
        T = one[0].shape[0]
        assert fr[b] == T and (frames is None or T == frames[b]), (b, fr[b], T)
        for name, a, w in zip(NAMES, (f0, v, vp, s), one):
            d = torch.nonzero(_nn(a[b, :T]) != _nn(w)).flatten()
            assert d.numel() == 0, f"row {b} ({len(c)} samples) {name}: {d.numel()} frames differ, first {d[:5].tolist()}"
            assert not a[b, T:].any(), f"row {b} {name}: the tail is not zero"


# ---------------------------------------------------------------------------------------------------------------------
# 1, 2, 4: every clip equals the clip alone, whatever the padding holds; the oracle anchor
# ---------------------------------------------------------------------------------------------------------------------
_RAGGED = {}


def _ragged(gpu, dtype, fill=0.0):
    key = (np.dtype(dtype).str, str(fill))
    if key not in _RAGGED:
        _RAGGED[key] = pyin_ragged_batch(_packed(_clips(dtype), gpu, fill), LENGTHS * 2, SR, return_states=True, **C5)
    return _RAGGED[key]


@pytest.mark.parametrize("dtype", DTYPES)
def test_every_clip_equals_the_clip_alone(gpu, dtype):
    clips = _clips(dtype)
    out = _ragged(gpu, dtype)
    f0, v, vp, fr, s = out
    assert f0.shape == v.shape == vp.shape == s.shape == (18, 101) and fr.shape == (18,)
    assert f0.dtype == torch.float64 and v.dtype == torch.bool and s.dtype == torch.int32 and fr.dtype == torch.int64
    assert fr.is_cuda and fr.cpu().tolist() == FRAMES * 2
    _assert_rows_equal_alone(gpu, out, clips, FRAMES * 2, **C5)
    for b, n in enumerate(LENGTHS):                  # the glide clips have voiced frames: the comparison is not empty
        if n in VOICED:
            got = int(v[b].sum())
            print(f"{n} samples: {got} voiced frames")
            assert got == VOICED[n]


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_padding_never_matters(gpu, dtype):
    base = _ragged(gpu, dtype)
    for fill in (float("nan"), float("inf"), "next"):
        got = _ragged(gpu, dtype, fill)
        for name, a, w in zip(NAMES + ("frames",), (got[0], got[1], got[2], got[4], got[3]),
                              (base[0], base[1], base[2], base[4], base[3])):
            assert torch.equal(_nn(a), _nn(w)), (fill, name)
    # the test can see a difference: the padded batch as one length differs on the frames near a clip's end
    clips = _clips(dtype)
    whole = pyin_batch(_packed(clips, gpu, float("nan")), SR, return_states=True, **C5)
    b = LENGTHS.index(640)
    assert not torch.equal(_nn(whole[2][b, :17]), _nn(base[2][b, :17]))
    assert not torch.equal(_nn(whole[0][b, :17]), _nn(base[0][b, :17]))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", [4000, 640])
def test_oracle_anchor(gpu, n, dtype):
    b = LENGTHS.index(n)
    y = _clips(dtype)[b]
    wf, wv, wvp, ws = O.pyin_banded(y, sr=SR, return_states=True, **C5)
    f0, v, vp, fr, s = (a[b].cpu().numpy() for a in _ragged(gpu, dtype, "next"))
    T = len(wf)
    assert fr == T and wv.sum() == VOICED[n]
    assert np.array_equal(v[:T], wv)
    np.testing.assert_array_equal(f0[:T], wf)
    assert np.array_equal(s[:T][wv], ws[wv])
    err = np.abs(vp[:T] - wvp).max()
    print(f"voiced_prob err {err:.3e}")
    assert err <= 1e-12


# ---------------------------------------------------------------------------------------------------------------------
# 3: the C entry writes the tails and d_frames
# ---------------------------------------------------------------------------------------------------------------------
def test_c_entry_writes_the_tails(gpu):
    clips = _clips(np.float32)
    x = _packed(clips, gpu, float("nan"))
    B, n = x.shape
    p, z = pitch.pyin_params(n, SR, **C5)
    tabs = pitch._tables(p, z, 0.01, (2, 18), 2, gpu)
    p.band_h = tabs.H
    T = z["n_frames"]
    assert T == 101
    lib = _lib.load()

    def ff(dtype):
        return torch.full((B * T * torch.empty((), dtype=dtype).element_size(),), 0xFF, dtype=torch.uint8,
                          device=gpu).view(dtype).view(B, T)

    f0, voiced, vp, states = ff(torch.float64), ff(torch.uint8), ff(torch.float64), ff(torch.int32)
    frames = torch.full((B * 8,), 0xFF, dtype=torch.uint8, device=gpu).view(torch.int64)
    assert int(frames[0]) == -1 and bool(torch.isnan(f0).all())
    lens = torch.tensor(LENGTHS * 2, dtype=torch.int64, device=gpu)
    ws = torch.empty(int(lib.mm_pyin_ragged_workspace_bytes(C.byref(p), B, n)), dtype=torch.uint8, device=gpu)
    with torch.cuda.device(gpu):
        _lib.check(lib.mm_pyin_ragged_f32(C.byref(p), C.byref(tabs.c), x.data_ptr(), B, n, n, lens.data_ptr(),
                                          f0.data_ptr(), voiced.data_ptr(), vp.data_ptr(), states.data_ptr(),
                                          frames.data_ptr(), ws.data_ptr(), ws.numel(),
                                          C.c_void_p(torch.cuda.current_stream(gpu).cuda_stream)), "mm_pyin_ragged_f32")
    assert frames.cpu().tolist() == FRAMES * 2
    base = _ragged(gpu, np.float32)
    for b, Tb in enumerate(FRAMES * 2):
        for name, a in zip(NAMES, (f0, voiced, vp, states)):
            tail = a[b, Tb:].contiguous().view(torch.uint8)
            assert not tail.any(), f"row {b} {name}: bytes behind frame {Tb} are not zero"
        assert torch.equal(_nn(f0[b, :Tb]), _nn(base[0][b, :Tb])) and torch.equal(states[b, :Tb], base[4][b, :Tb])
    # d_frames may be NULL
    f2 = ff(torch.float64)
    with torch.cuda.device(gpu):
        _lib.check(lib.mm_pyin_ragged_f32(C.byref(p), C.byref(tabs.c), x.data_ptr(), B, n, n, lens.data_ptr(),
                                          f2.data_ptr(), voiced.data_ptr(), vp.data_ptr(), states.data_ptr(), None,
                                          ws.data_ptr(), ws.numel(),
                                          C.c_void_p(torch.cuda.current_stream(gpu).cuda_stream)), "mm_pyin_ragged_f32")
    assert torch.equal(_nn(f2), _nn(f0))


# ---------------------------------------------------------------------------------------------------------------------
# 5 - 8: center=False, pad modes, fill_na, layouts
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_center_false(gpu, dtype):
    kw = dict(C5, center=False)
    lengths = [4000, 512, 551, 552]
    clips = _clips(dtype, lengths)[:4]
    out = pyin_ragged_batch(_packed(clips, gpu, float("nan")), lengths, SR, return_states=True, **kw)
    assert out[0].shape == (4, 88)
    _assert_rows_equal_alone(gpu, out, clips, [88, 1, 1, 2], **kw)
    # a clip without a frame: host lengths name it, device lengths give it a zero row
    short = [4000, 512, 511, 552]
    with pytest.raises(ValueError, match=r"511 samples is shorter than frame_length=512 \(clip 2\)"):
        pyin_ragged_batch(_packed(clips, gpu), short, SR, **kw)
    dl = torch.tensor(short, dtype=torch.int64, device=gpu)
    got = pyin_ragged_batch(_packed(clips, gpu, float("nan")), dl, SR, return_states=True, **kw)
    assert got[3].cpu().tolist() == [88, 1, 0, 2]
    for name, a, w in zip(NAMES, (got[0], got[1], got[2], got[4]), (out[0], out[1], out[2], out[4])):
        assert not a[2].any(), name
        for b in (0, 1, 3):
            assert torch.equal(_nn(a[b]), _nn(w[b])), (name, b)


@pytest.mark.parametrize("pad_mode,dtype", [("reflect", np.float32), ("edge", np.float64), ("wrap", np.float32)])
def test_pad_modes(gpu, pad_mode, dtype):
    kw = dict(C5, pad_mode=pad_mode)
    lengths = [4000, 2500, 700]
    clips = _clips(dtype, lengths)[:3]
    out = pyin_ragged_batch(_packed(clips, gpu, float("nan")), lengths, SR, return_states=True, **kw)
    assert out[0].shape == (3, 101)
    _assert_rows_equal_alone(gpu, out, clips, [101, 63, 18], **kw)
    assert out[1][0].any() and out[1][1].any()
    # the padding mode matters: the zero-padded track of the same clip differs
    assert not torch.equal(_nn(out[2][1, :63]), _nn(_alone(gpu, clips[1], **C5)[2]))
    with pytest.raises(ValueError, match="host"):
        pyin_ragged_batch(_packed(clips, gpu), torch.tensor(lengths, device=gpu), SR, **kw)


@pytest.mark.parametrize("fill_na", [None, 0.0])
def test_fill_na(gpu, fill_na):
    kw = dict(C5, fill_na=fill_na)
    clips = _clips(np.float32)
    out = pyin_ragged_batch(_packed(clips, gpu, float("nan")), LENGTHS * 2, SR, return_states=True, **kw)
    _assert_rows_equal_alone(gpu, out, clips, FRAMES * 2, **kw)
    assert bool(torch.isfinite(out[0]).all())
    if fill_na is None:                              # unvoiced frames keep the decoded bin's frequency, dead frames are 0
        assert bool((out[0][0] >= 100).all()) and not out[1][0].all()
        assert bool((out[0][1, :1] >= 100).all()) and not out[0][1, 1:].any()


def test_layouts_and_length_checks(gpu, monkeypatch):
    clips = _clips(np.float32)
    base = _ragged(gpu, np.float32)
    wide = _packed(clips, gpu, float("nan"), extra=7)
    view = wide[:, :4000]
    assert view.stride() == (4007, 1) and not view.is_contiguous()
    lib = _lib.load()
    real, seen = lib.mm_pyin_ragged_f32, []

    def spy(*a):
        seen.append((a[2], a[4], a[5]))
        return real(*a)

    monkeypatch.setattr(lib, "mm_pyin_ragged_f32", spy)
    got = pyin_ragged_batch(view, LENGTHS * 2, SR, return_states=True, **C5)
    assert seen == [(view.data_ptr(), 4000, 4007)]           # used in place
    for a, w in zip(got, base):
        assert torch.equal(_nn(a), _nn(w))
    # rows two pitches apart, a numpy / CPU-tensor / int32 lengths argument
    every = torch.full((36, 4000), float("inf"), dtype=torch.float32, device=gpu)
    every[::2] = _packed(clips, gpu)
    for lens in (np.array(LENGTHS * 2, dtype=np.int32), torch.tensor(LENGTHS * 2)):
        got = pyin_ragged_batch(every[::2], lens, SR, return_states=True, **C5)
        for a, w in zip(got, base):
            assert torch.equal(_nn(a), _nn(w))
    # device lengths are clamped into [1, n_max] by the kernels
    wild = torch.tensor(LENGTHS * 2, dtype=torch.int64, device=gpu)
    wild[0], wild[8], wild[1], wild[10] = 10 ** 12, 4001, 0, -7
    want = list(LENGTHS * 2)
    want[0], want[8], want[1], want[10] = 4000, 4000, 1, 1
    got = pyin_ragged_batch(_packed(clips, gpu, float("nan"))[:, :4000], wild, SR, return_states=True, **C5)
    x8 = _packed(clips, gpu)                               # row 8 holds 3999 samples and a zero: as 4000 samples
    ref = pyin_ragged_batch(x8, want, SR, return_states=True, **C5)
    for b in range(18):
        if b != 8:
            for a, w in zip(got, ref):
                assert torch.equal(_nn(a[b]), _nn(w[b])), b
    assert got[3].cpu().tolist() == ref[3].cpu().tolist() and int(got[3][8]) == 101
    # host lengths outside the range are refused
    for bad in ([0] + LENGTHS[1:] + LENGTHS, [4001] + LENGTHS[1:] + LENGTHS, LENGTHS):
        with pytest.raises(ValueError):
            pyin_ragged_batch(x8, bad, SR, **C5)
    with pytest.raises(TypeError):
        pyin_ragged_batch(x8, torch.tensor(LENGTHS * 2, dtype=torch.int32, device=gpu), SR, **C5)
    with pytest.raises(ValueError):
        pyin_ragged_batch(x8[0], LENGTHS[:1], SR, **C5)


# ---------------------------------------------------------------------------------------------------------------------
# 9, 10: two CMND chunks, row cuts
# ---------------------------------------------------------------------------------------------------------------------
TWO_CHUNK = [100000, 60000, 100000, 31, 100000, 100000, 90000]
_TWO = {}


def _two_chunk(gpu, last):
    if last not in _TWO:
        rows, z, at = P._c5_rows()
        assert rows.shape == (7, 100000) and z["n_frames"] == 2501 and at == 1378
        lengths = TWO_CHUNK[:6] + [last]
        x = _dev(rows, gpu).clone()
        for b, n in enumerate(lengths):
            x[b, n:] = float("nan")
        _TWO[last] = (x, lengths, pyin_ragged_batch(x, lengths, SR, return_states=True, **C5))
    return _TWO[last]


@pytest.mark.parametrize("last", [90000, 40000])
def test_two_cmnd_chunks(gpu, last):
    """Flat frame 16 384 = frame 1378 of row 6, inside a tile: a live frame of the 90 000-sample row (2251 frames), a dead
    one of the 40 000-sample row (1001 frames)."""
    rows, _, at = P._c5_rows()
    x, lengths, out = _two_chunk(gpu, last)
    frames = pyin_ragged_frames(lengths, 512, 40)
    assert frames.tolist() == [2501, 1501, 2501, 1, 2501, 2501, 2251 if last == 90000 else 1001]
    assert (at < frames[6]) == (last == 90000) and 7 * 2501 > P.CHUNK_FRAMES
    _assert_rows_equal_alone(gpu, out, [rows[b, :n] for b, n in enumerate(lengths)], frames, **C5)
    assert out[1][0].sum() > 500 and out[1][6].sum() > 200          # the glides are voiced


def test_row_cuts(gpu, monkeypatch):
    x, lengths, whole = _two_chunk(gpu, 90000)
    lib = _lib.load()
    p, _ = pitch.pyin_params(x.shape[1], SR, **C5)
    # room for three rows of scratch, not for four
    monkeypatch.setattr(pitch, "PYIN_WS_BYTES", int(lib.mm_pyin_ragged_workspace_bytes(C.byref(p), 4, x.shape[1])) - 1)
    real, calls = lib.mm_pyin_ragged_f32, []

    def counted(*a):
        calls.append(a[3])
        return real(*a)

    monkeypatch.setattr(lib, "mm_pyin_ragged_f32", counted)
    parts = pyin_ragged_batch(x, lengths, SR, return_states=True, **C5)
    assert calls == [3, 3, 1]
    for a, b in zip(whole, parts):
        assert torch.equal(_nn(a), _nn(b))


# ---------------------------------------------------------------------------------------------------------------------
# 11: ragged interp_NAN
# ---------------------------------------------------------------------------------------------------------------------
KINDS = ["linear", "pchip", "nearest", "nearest-up", "previous", "next", "zero", "slinear"]
COUNTS = [2500, 1024, 1025, 2, 1, 700]


def _curves():
    """[6, 2500]: a NaN run that swallows segment 1 (row 0), NaN first and last sample below the count (rows 0, 5), a
    NaN exactly at c_b - 1 (rows 1, 2), rows of two and of one valid sample."""
    rng = np.random.default_rng(11)
    x = np.cumsum(rng.standard_normal((6, 2500)), axis=1)
    x[rng.random(x.shape) < 0.3] = np.nan
    x[0, 1000:2100] = np.nan
    x[0, 0] = x[0, 2499] = np.nan
    x[0, 1] = x[0, 2498] = 1.5
    x[1, 1023], x[1, 1022], x[1, 0] = np.nan, 0.25, -1.0
    x[2, 1024], x[2, 1023], x[2, 0], x[2, 1] = np.nan, 4.0, np.nan, 2.0
    x[3, :2] = (3.0, -2.0)
    x[4, 0] = 9.0
    x[5, 0] = x[5, 699] = np.nan
    x[5, 1] = x[5, 698] = 0.5
    return x


def _garbage(x, counts, what):
    x = x.copy()
    for b, c in enumerate(counts):
        x[b, c:] = np.nan if what == "nan" else (7.5 if what == "finite" else x[b, c:])
    return x


@pytest.mark.parametrize("method", KINDS)
def test_ragged_interp_nan(gpu, method):
    x = _curves()
    # interp1d needs two points under 'linear', NaN or not: the one-sample row is its error case (below)
    keep = [b for b, c in enumerate(COUNTS) if not (method == "linear" and c < 2)]
    counts = [COUNTS[b] for b in keep]
    got = None
    for what in ("nan", "finite", "as it is"):
        xd = _dev(_garbage(x[keep], counts, what), gpu)
        y = interp_nan_ragged_batch(xd, counts, method)
        assert y.shape == xd.shape and y.dtype == torch.float64
        if got is not None:
            assert torch.equal(_nn(y), _nn(got)), what
        got = y
    filled = 0
    for k, b in enumerate(keep):
        c = COUNTS[b]
        want = interp_nan_batch(_dev(x[b, :c], gpu), method)
        d = torch.nonzero(_nn(got[k, :c]) != _nn(want)).flatten()
        assert d.numel() == 0, f"row {b} (count {c}): {d.numel()} samples differ, first {d[:5].tolist()}"
        assert not got[k, c:].contiguous().view(torch.uint8).any(), f"row {b}: not zero behind the count"
        filled += int((~torch.isnan(want)).sum()) - int((~np.isnan(x[b, :c])).sum())
    assert filled > 2000
    # device counts, clamped by the kernels; a float32 batch; a row pitch of its own
    dc = torch.tensor(counts, dtype=torch.int64, device=gpu)
    dc2 = dc.clone()
    dc2[0] = 10 ** 9
    for cc in (dc, dc2):
        assert torch.equal(_nn(interp_nan_ragged_batch(_dev(_garbage(x[keep], counts, "nan"), gpu), cc, method)), _nn(got))
    wide = torch.full((len(keep), 2600), 3.25, dtype=torch.float64, device=gpu)
    wide[:, :2500] = _dev(x[keep], gpu)
    assert torch.equal(_nn(interp_nan_ragged_batch(wide[:, :2500], counts, method)), _nn(got))
    y32 = interp_nan_ragged_batch(_dev(x[keep].astype(np.float32), gpu), counts, method)
    assert y32.dtype == torch.float32
    for k, b in enumerate(keep):
        want = interp_nan_batch(_dev(x[b, :COUNTS[b]].astype(np.float32), gpu), method)
        assert torch.equal(_nn(y32[k, :COUNTS[b]]), _nn(want))


@pytest.mark.parametrize("method", KINDS)
def test_ragged_interp_nan_refusals(gpu, method):
    x = _curves()
    xd = _dev(x, gpu)
    # (counts, row at fault): no valid sample below the count; one valid sample and a NaN; one sample without a NaN
    cases = [([2500, 1024, 1, 2, 1, 700], 2), ([2500, 1024, 2, 2, 1, 700], 2), (COUNTS, 4)]
    for counts, b in cases:
        alone = None
        try:
            interp_nan_batch(xd[b, :counts[b]], method)
        except (ValueError, IndexError) as e:
            alone = e
        if alone is None:
            if all(c == COUNTS[i] or i == b for i, c in enumerate(counts)) and not (method == "linear" and 1 in counts):
                interp_nan_ragged_batch(xd, counts, method)
            continue
        with pytest.raises(type(alone)) as ei:
            interp_nan_ragged_batch(xd, counts, method)
        assert str(ei.value) == str(alone)
    assert isinstance(alone, ValueError) == (method == "linear")       # the last case: a lone valid sample
    with pytest.raises(NotImplementedError):
        interp_nan_ragged_batch(xd, COUNTS, "cubic")
    with pytest.raises(NotImplementedError):
        interp_nan_ragged_batch(xd, COUNTS, "quadratic")
    with pytest.raises(ValueError):
        interp_nan_ragged_batch(xd, COUNTS, "spline")
    with pytest.raises(ValueError):
        interp_nan_ragged_batch(xd, [2501] + COUNTS[1:], method)
    with pytest.raises(ValueError):
        interp_nan_ragged_batch(xd, COUNTS[1:], method)


# ---------------------------------------------------------------------------------------------------------------------
# 12: get_f0_batch
# ---------------------------------------------------------------------------------------------------------------------
F0_SR = 16000


def _f0_clips(gpu):
    g = [O.synth("glide", F0_SR, s, np.float64, seed=i) for i, s in enumerate((1.0, 0.7, 0.5, 0.8, 0.6))]
    return [g[0].astype(np.float32), g[1], np.round(g[2] * 20000).astype(np.int16), _dev(g[3].astype(np.float32), gpu),
            _dev(g[4], gpu)]


_F0_CASES = [(i, f, q) for i in ("linear", "pchip", None) for f in (None, "iir") for q in (None, [0.1, 0.9])
             if not (i is None and f is not None)]


@pytest.mark.parametrize("interp,filt,quant", _F0_CASES)
def test_get_f0_batch_equals_get_f0(gpu, interp, filt, quant):
    kw = dict(method="pyin", interpUnvoiced=interp, outFilter=filt, outFiltCutOff=[10], minMaxQuant=quant)
    clips = _f0_clips(gpu)
    got = get_f0_batch(clips, F0_SR, **kw)
    assert isinstance(got, list) and len(got) == 5
    lens = set()
    for i, (c, (f0, f0t)) in enumerate(zip(clips, got)):
        wf, wt = get_f0(c, F0_SR, **kw)
        assert type(f0) is type(wf) and isinstance(f0t, np.ndarray) and f0t.dtype == wt.dtype
        np.testing.assert_array_equal(f0t, wt)
        if isinstance(c, torch.Tensor):
            assert f0.is_cuda and f0.dtype == wf.dtype and f0.shape == wf.shape
            assert torch.equal(_nn(f0), _nn(wf)), f"clip {i}"
        else:
            assert f0.dtype == wf.dtype
            np.testing.assert_array_equal(f0, wf, err_msg=f"clip {i}")
        lens.add(len(wt))
        if interp is None:
            assert np.isnan(np.asarray(wf.cpu() if isinstance(c, torch.Tensor) else wf)).any()      # unvoiced gaps stay
    assert len(lens) == 5


@pytest.mark.parametrize("interp", ["linear", "cubic"])
def test_get_f0_batch_filters_clips_of_one_frame_count_together(gpu, interp):
    """Three float64 clips of one frame count and one of another: applyFilter sees [3, T] and [1, T'].  'cubic' takes the
    per-clip scipy route of interp_NAN."""
    g = [O.synth("glide", F0_SR, 0.7, np.float64, seed=i) for i in range(3)]
    clips = [g[0][:11100], g[1][:11050], g[2][:5000], g[1][:11199]]      # 70, 70, 32 and 70 frames (hop 160)
    kw = dict(method="pyin", interpUnvoiced=interp, outFilter="iir", outFiltCutOff=[10])
    got = get_f0_batch(clips, F0_SR, **kw)
    assert [len(t) for _, t in got] == [70, 70, 32, 70]
    for i, (c, (f0, f0t)) in enumerate(zip(clips, got)):
        wf, wt = get_f0(c, F0_SR, **kw)
        np.testing.assert_array_equal(f0, wf, err_msg=f"clip {i}")
        np.testing.assert_array_equal(f0t, wt)


def test_get_f0_batch_refusals(gpu):
    clips = _f0_clips(gpu)
    with pytest.raises(NotImplementedError):
        get_f0_batch(clips, F0_SR, method="praatac")
    with pytest.raises(NotImplementedError):
        get_f0(clips[0], F0_SR, method="praatac")
    assert get_f0_batch([], F0_SR, method="pyin") == []
    # one clip at fault is named: too short without centring, a two-dimensional clip
    with pytest.raises(ValueError, match=r"2047 samples is shorter than frame_length=2048 \(clip 1\)"):
        get_f0_batch([clips[0], np.zeros(2047)], F0_SR, method="pyin", pyincenter=False)
    with pytest.raises(ValueError, match=r"\(clip 2\)"):
        get_f0_batch([clips[0], clips[1], np.zeros((2, 4000))], F0_SR, method="pyin")
    # a steady tone: the quantiles of the first pass leave no room for the transition band (get_f0 raises the same); the
    # glides pass, and the index is the clip's place in the list, not in its float64 group
    tone = O.synth("sine200", F0_SR, 1.0, np.float64)
    kw = dict(method="pyin", outFiltCutOff=[12], minMaxQuant=[0.05, 0.95])
    with pytest.raises(ValueError) as one:
        get_f0(tone, F0_SR, **kw)
    with pytest.raises(ValueError) as many:
        get_f0_batch([clips[0], clips[1], tone], F0_SR, **kw)
    assert str(many.value) == str(one.value) + " (clip 2)"
    assert len(get_f0_batch([clips[0], clips[1]], F0_SR, **kw)) == 2
