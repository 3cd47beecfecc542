"""GPU: the amplitude envelopes of a ragged batch -- mm_hilbert_envelope_ragged / hilbert_envelope_ragged_batch against
scipy.signal.hilbert at every clip's OWN length, mm_rms_ragged_f32 / rms_ragged_batch bit for bit against rms_batch on the
clip alone, and calculate_amplitude_envelope_batch against the single call.  The Hilbert bounds are those of
tests/test_gpu_parity.py::test_hilbert_envelope_on_device (2e-5 / 1e-11 of the row's maximum); every figure is printed
before it is asserted (-s shows them)."""
import functools

import numpy as np
import pytest
import scipy.signal
import torch

import mfcc_oracle as O
from modulation_mfcc_amd import _lib, calc
from modulation_mfcc_amd.batch import rms_batch, rms_ragged_batch, rms_ragged_frames
from modulation_mfcc_amd.calc import (calculate_amplitude_envelope, calculate_amplitude_envelope_batch,
                                      hilbert_envelope_ragged_batch)

pytestmark = pytest.mark.gpu

TOL = {np.float32: 2e-5, np.float64: 1e-11}
SMALL = (11, 4097, (1, 2, 3, 16, 17, 255, 256, 257, 1000, 4096, 4097))      # M = 16 .. 16384
LARGE = (3, 70001, (70001, 65537, 12345))                                   # M = 262144: radix 256, 256, 4


@functools.lru_cache(maxsize=None)
def _case(which, dt):
    """(x [B, n_max] with NaN behind every clip's end, lengths, [|hilbert| of each clip in float64]) -- computed once."""
    B, n_max, lens = SMALL if which == "small" else LARGE
    rng = np.random.default_rng(B)
    x = np.full((B, n_max), np.nan, dtype=dt)
    want = []
    for b, n in enumerate(lens):
        x[b, :n] = (rng.standard_normal(n) * np.linspace(0.2, 1.0, n)).astype(dt)
        want.append(np.abs(scipy.signal.hilbert(x[b, :n].astype(np.float64))))
    x.setflags(write=False)
    return x, np.array(lens, dtype=np.int64), want


def _dev(x, gpu):
    return torch.from_numpy(np.array(x)).to(gpu)


def _check_rows(got, lens, want, tol, what):
    for b, n in enumerate(lens):
        err = np.abs(got[b, :n] - want[b]).max()
        print(f"hilbert-ragged {what} row {b} n {n}: err {err:.3e} max {want[b].max():.3e} -> {err / max(want[b].max(), 1e-300):.3e}")
        assert err <= tol * want[b].max() + 1e-300, (what, b, n, err, want[b].max())
        tail = got[b, n:]
        assert (tail == 0).all() and not np.signbit(tail).any(), (what, b, n)


@pytest.mark.parametrize("device_lengths", [False, True])
@pytest.mark.parametrize("which", ["small", "large"])
@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_hilbert_against_scipy(dt, which, device_lengths, gpu):
    x, lens, want = _case(which, dt)
    lengths = _dev(lens, gpu) if device_lengths else lens
    got = hilbert_envelope_ragged_batch(_dev(x, gpu), lengths)
    assert got.is_cuda and got.shape == x.shape and got.cpu().numpy().dtype == dt
    _check_rows(got.cpu().numpy(), lens, want, TOL[dt], f"{which} {np.dtype(dt).name} {'dev' if device_lengths else 'host'}")


@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_the_padding_never_matters(dt, gpu):
    x, lens, _ = _case("small", dt)
    B, n_max = x.shape
    base = hilbert_envelope_ragged_batch(_dev(x, gpu), lens).cpu().numpy()          # NaN behind every clip's end
    zeros = np.where(np.isnan(x), 0, x)
    perm = np.random.default_rng(3).permutation(B)
    wide = np.full((B, n_max + 333), 7.0, dtype=dt)
    wide[:, :n_max] = zeros
    runs = {"zero padding": hilbert_envelope_ragged_batch(_dev(zeros, gpu), lens).cpu().numpy(),
            "permuted": hilbert_envelope_ragged_batch(_dev(x[perm], gpu), lens[perm]).cpu().numpy()[np.argsort(perm)],
            "wider": hilbert_envelope_ragged_batch(_dev(wide, gpu), lens).cpu().numpy()[:, :n_max]}
    for what, got in runs.items():
        for b, n in enumerate(lens):
            assert np.array_equal(got[b, :n], base[b, :n]), (what, b, n)
    for b, n in enumerate(lens):
        alone = hilbert_envelope_ragged_batch(_dev(x[b:b + 1, :n], gpu), [n]).cpu().numpy()
        assert np.array_equal(alone[0], base[b, :n]), (b, n)


@pytest.mark.parametrize("device_lengths", [False, True])
@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_rows_are_independent(dt, device_lengths, gpu):
    x, lens, _ = _case("small", dt)
    lengths = _dev(lens, gpu) if device_lengths else lens
    base = hilbert_envelope_ragged_batch(_dev(x, gpu), lengths).cpu().numpy()
    bad = x.copy()
    bad[8, 500] = np.nan          # the clip of 1000 samples
    bad[5, 0] = np.inf            # 255 samples
    bad[10, 4096] = -np.inf       # 4097 samples: its last one
    got = hilbert_envelope_ragged_batch(_dev(bad, gpu), lengths).cpu().numpy()
    for b, n in enumerate(lens):
        if b in (5, 8, 10):
            assert np.isnan(got[b, :n]).all(), b
        else:
            assert np.array_equal(got[b, :n], base[b, :n]), b
        assert (got[b, n:] == 0).all() and not np.signbit(got[b, n:]).any(), b


@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_amplitude_scaling(dt, gpu):
    rng = np.random.default_rng(12)
    lens = np.array([1000, 777, 1000, 900, 12])
    amp = [1.0, 1e-6, 1e3, 0.0, 1e-6]
    x = np.full((5, 1000), np.nan, dtype=dt)
    want = []
    for b, n in enumerate(lens):
        x[b, :n] = (rng.standard_normal(n) * amp[b]).astype(dt)
        want.append(np.abs(scipy.signal.hilbert(x[b, :n].astype(np.float64))))
    got = hilbert_envelope_ragged_batch(_dev(x, gpu), lens).cpu().numpy()
    _check_rows(got, lens, want, TOL[dt], f"scaling {np.dtype(dt).name}")
    assert (got[3] == 0).all() and not np.signbit(got[3]).any()            # the clip of zeros


@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_one_class_in_a_wider_batch(dt, gpu):
    """Host lengths of ONE power-of-two class in a batch padded far beyond what that class's transform length covers
    (M = 256 takes 128 samples, n_max is 4096; equal short clips in a wide buffer): the call is cut to the longest clip."""
    rng = np.random.default_rng(5)
    for lens, n_max in (([128, 128, 128], 129), ([1, 1], 1000), ([70, 70], 70), ([100, 100, 90, 120], 4096)):
        lens = np.array(lens)
        x = np.full((len(lens), n_max), np.nan, dtype=dt)
        want = []
        for b, n in enumerate(lens):
            x[b, :n] = rng.standard_normal(n).astype(dt)
            want.append(np.abs(scipy.signal.hilbert(x[b, :n].astype(np.float64))))
        got = hilbert_envelope_ragged_batch(_dev(x, gpu), lens)
        assert got.shape == x.shape
        got = got.cpu().numpy()
        _check_rows(got, lens, want, TOL[dt], f"one class {np.dtype(dt).name} n_max {n_max}")
        for b, n in enumerate(lens):       # a row's bits depend on its own length only
            alone = hilbert_envelope_ragged_batch(_dev(x[b:b + 1, :n], gpu), [n]).cpu().numpy()
            assert np.array_equal(alone[0], got[b, :n]), (n_max, b)
    # the same through the list call's route
    env, out_len, _ = calc.amplitude_envelope_ragged_batch(_dev(x, gpu), lens, 8000.0, method="Hilb")
    assert np.array_equal(env.cpu().numpy(), got) and out_len.tolist() == lens.tolist()


def test_float32_range(gpu):
    """No per-clip scaling: the transforms reach max(envelope) n M, finite in float32 far beyond audio's [-1, 1]."""
    rng = np.random.default_rng(6)
    lens = np.array([1000, 900])
    x = np.zeros((2, 1000), dtype=np.float32)
    want = []
    for b, (n, amp) in enumerate(zip(lens, (1e20, 1e-20))):
        x[b, :n] = (rng.standard_normal(n) * amp).astype(np.float32)
        want.append(np.abs(scipy.signal.hilbert(x[b, :n].astype(np.float64))))
    got = hilbert_envelope_ragged_batch(_dev(x, gpu), lens).cpu().numpy()
    _check_rows(got, lens, want, TOL[np.float32], "range float32")


def test_limits(gpu, monkeypatch):
    x, lens, want = _case("small", np.float32)
    B, n_max = x.shape
    xd = _dev(x, gpu)
    base = hilbert_envelope_ragged_batch(xd, _dev(lens, gpu)).cpu().numpy()
    # device lengths are clamped into [1, n_max]
    odd = lens.copy()
    odd[0], odd[1], odd[10] = 0, -5, n_max + 9
    got = hilbert_envelope_ragged_batch(xd, _dev(odd, gpu)).cpu().numpy()
    assert np.array_equal(got[0, :1], base[0, :1]) and (got[0, 1:] == 0).all()              # 0 -> 1 (the row's own length)
    assert got[1, 0] == np.abs(x[1, 0]) and (got[1, 1:] == 0).all()                         # -5 -> 1: |x[0]|
    assert np.array_equal(got[10], base[10])                                                # n_max + 9 -> n_max
    assert got[0, 0] == np.abs(x[0, 0])                                                     # n_b = 1 gives |x[0]|
    # host lengths outside [1, n_max]
    for bad in (0, -5, n_max + 9):
        with pytest.raises(ValueError, match=r"lengths must lie in"):
            hilbert_envelope_ragged_batch(xd, [bad] + list(lens[1:]))
    with pytest.raises(TypeError):
        hilbert_envelope_ragged_batch(xd.half(), lens)
    with pytest.raises(TypeError, match="int64"):
        hilbert_envelope_ragged_batch(xd, _dev(lens.astype(np.int32), gpu))
    # a strided view: every second column of a wider batch, and rows with a pitch beyond n_max
    wide = torch.zeros((B, 2 * n_max), dtype=torch.float32, device=gpu)
    wide[:, ::2] = xd
    assert np.array_equal(hilbert_envelope_ragged_batch(wide[:, ::2], _dev(lens, gpu)).cpu().numpy(), base)
    pitch = torch.full((B, n_max + 77), float("nan"), dtype=torch.float32, device=gpu)
    pitch[:, :n_max] = xd
    assert np.array_equal(hilbert_envelope_ragged_batch(pitch[:, :n_max], _dev(lens, gpu)).cpu().numpy(), base)
    # a workspace bound that forces several calls: the same bits
    lib = _lib.load()
    plan = calc._hilbert_ragged_plan(calc.hilbert_ragged_fft_size(n_max), 0, gpu)
    per_row = int(lib.mm_hilbert_ragged_workspace_bytes(plan.h, 1, n_max))
    monkeypatch.setattr(calc, "HILBERT_WS_BYTES", 3 * per_row + 100)
    assert np.array_equal(hilbert_envelope_ragged_batch(xd, _dev(lens, gpu)).cpu().numpy(), base)
    monkeypatch.undo()
    # the C entry's checks that need a handle; they answer before any launch
    need = int(lib.mm_hilbert_ragged_workspace_bytes(plan.h, B, n_max))
    assert need > 3 * B * 16384 * 8 + B * n_max * 8
    assert lib.mm_hilbert_ragged_workspace_bytes(plan.h, 0, n_max) == 0
    assert lib.mm_hilbert_ragged_workspace_bytes(plan.h, B, 8193) == 0                      # 2 n_max - 1 > M
    ws = torch.empty(need, dtype=torch.uint8, device=gpu)
    out = torch.empty((B, n_max), dtype=torch.float32, device=gpu)
    ld = _dev(lens, gpu)

    def call(h=plan.h, rows=B, n=n_max, xs=n_max, ys=n_max, wsb=need):
        return lib.mm_hilbert_envelope_ragged(h, xd.data_ptr(), rows, n, xs, ld.data_ptr(), out.data_ptr(), ys, ws.data_ptr(),
                                              wsb, None)
    assert call(xs=n_max - 1) == -1 and call(ys=n_max - 1) == -1 and call(n=8193, xs=8193, ys=8193) == -1
    assert call(rows=0) == -1 and call(rows=65536) == -1
    assert call(wsb=need - 1) == _lib.MM_ERR_WORKSPACE
    single = calc._hilbert_plan(4097, 0, gpu)
    assert call(h=single.h) == -1                                                           # not a ragged handle
    assert lib.mm_hilbert_envelope(plan.h, xd.data_ptr(), B, n_max, out.data_ptr(), n_max, ws.data_ptr(), need, None) == -1
    assert call() == 0
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), base)


# ---- RMS ----
def _fpt(frame, hop):
    """Frames per tile of rms_tile_kernel (mm_rms_f32's rule), None where the frame leaves the tiled kernel."""
    want = frame + 15 * hop
    lds = min(max(want, 4096), 16384)
    return min((lds - frame) // hop + 1, 64) if frame <= lds else None


def _len_for_frames(T, frame, hop, center):
    """The shortest clip with T frames."""
    return max(1, (T - 1) * hop + frame - (2 * (frame // 2) if center else 0))


@pytest.mark.parametrize("center", [True, False])
@pytest.mark.parametrize("frame,hop", [(400, 80), (401, 80), (64, 1), (5000, 100), (16385, 100)])
def test_rms_rows_equal_the_clip_alone(frame, hop, center, gpu):
    fpt = _fpt(frame, hop)
    assert (fpt is None) == (frame == 16385)             # 16385: the first frame length of the wave-per-frame kernel
    f = fpt or 16
    # clips that end on a tile boundary, one frame before it and one frame after it; one tile further; a single sample
    frames = [f, f - 1, f + 1, 2 * f, 2 * f + 1]
    lens = [_len_for_frames(T, frame, hop, center) for T in frames] + [1 if center else frame]
    n_max = _len_for_frames(2 * f + 3, frame, hop, center) + 5
    lens = np.array(lens + [n_max], dtype=np.int64)
    B = len(lens)
    rng = np.random.default_rng(frame + hop)
    x = np.full((B, n_max), np.nan, dtype=np.float32)
    for b, n in enumerate(lens):
        x[b, :n] = rng.standard_normal(n).astype(np.float32)
    xd = _dev(x, gpu)
    T = rms_ragged_frames(lens, frame, hop, center)
    assert T[:5].tolist() == frames and (T >= 1).all()
    for lengths in (lens, _dev(lens, gpu)):
        got = rms_ragged_batch(xd, lengths, frame, hop, center).cpu().numpy()
        assert got.shape == (B, T.max()) and got.dtype == np.float32
        for b, n in enumerate(lens):
            alone = rms_batch(xd[b, :n], frame, hop, center).cpu().numpy()[0]
            assert alone.shape == (T[b],)
            assert np.array_equal(got[b, :T[b]], alone), (b, n)
            assert (got[b, T[b]:] == 0).all() and not np.signbit(got[b, T[b]:]).any(), (b, n)
            np.testing.assert_allclose(got[b, :T[b]], O.rms_envelope(x[b, :n], frame, hop, center), rtol=2e-6, atol=1e-7)


def test_rms_clip_without_a_frame(gpu):
    frame, hop = 400, 80
    lens = np.array([1000, 399, 400, 1], dtype=np.int64)
    x = np.random.default_rng(1).standard_normal((4, 1000)).astype(np.float32)
    xd = _dev(x, gpu)
    got = rms_ragged_batch(xd, _dev(lens, gpu), frame, hop, center=False).cpu().numpy()
    assert got.shape == (4, 8)
    assert np.isnan(got[1]).all() and np.isnan(got[3]).all()
    assert np.array_equal(got[0], rms_batch(xd[0], frame, hop, False).cpu().numpy()[0])
    assert np.array_equal(got[2, :1], rms_batch(xd[2, :400], frame, hop, False).cpu().numpy()[0]) and (got[2, 1:] == 0).all()
    with pytest.raises(ValueError, match=r"399 samples is shorter than frame_length=400 \(clip 1\)"):
        rms_ragged_batch(xd, lens, frame, hop, center=False)
    with pytest.raises(ValueError, match="lengths must lie in"):
        rms_ragged_batch(xd, [1000, 0, 400, 1], frame, hop)
    with pytest.raises(TypeError):
        rms_ragged_batch(xd.double(), lens, frame, hop)
    # device lengths are clamped; a strided view
    odd = _dev(np.array([1009, 0, -5, 400], dtype=np.int64), gpu)
    got = rms_ragged_batch(xd, odd, frame, hop).cpu().numpy()
    assert np.array_equal(got[0], rms_batch(xd[0], frame, hop).cpu().numpy()[0])
    assert np.array_equal(got[1, :1], rms_batch(xd[1, :1], frame, hop).cpu().numpy()[0]) and (got[1, 1:] == 0).all()
    assert np.array_equal(got[2, :1], rms_batch(xd[2, :1], frame, hop).cpu().numpy()[0]) and (got[2, 1:] == 0).all()
    wide = torch.zeros((4, 2000), dtype=torch.float32, device=gpu)
    wide[:, ::2] = xd
    assert np.array_equal(rms_ragged_batch(wide[:, ::2], odd, frame, hop).cpu().numpy(), got)


# ---- calculate_amplitude_envelope_batch ----
SR = 8000.0
FILTERS = [None, "iir", "sg", "fir"]


def _clips(method, gpu):
    """Five clips of 3 distinct lengths, numpy and device mixed ('Hilb': float32 and float64 mixed): the oracle's synthetic
    recordings, amplitude-modulated tones in [-1, 1] as the envelope is meant for."""
    lens = [4000, 2500, 4000, 3210, 2500]
    dts = [np.float32, np.float64, np.float64, np.float32, np.float32] if method == "Hilb" else [np.float32] * 5
    host = [np.asarray(O.synth_clip(seed, n, int(SR), "am")).astype(dt) for seed, (n, dt) in enumerate(zip(lens, dts))]
    on_device = [True, False, True, True, False]
    return [_dev(c, gpu) if d else c for c, d in zip(host, on_device)], on_device


@pytest.mark.parametrize("filt", FILTERS)
@pytest.mark.parametrize("method", ["RMS", "Hilb"])
def test_list_call_equals_the_single_call(method, filt, gpu):
    from modulation_mfcc_amd.mfcc import get_amplitude_batch
    clips, on_device = _clips(method, gpu)
    kw = dict(method=method, winLen=0.05, hopLen=0.01, outFilter=filt, outFiltCutOff=[12], outFiltLen=7 if filt == "sg" else 6)
    got = calculate_amplitude_envelope_batch(clips, SR, **kw)
    again = get_amplitude_batch(clips, SR, **kw)
    assert len(got) == len(again) == 5
    for i, (c, d) in enumerate(zip(clips, on_device)):
        amp, t = got[i]
        want, want_t = calculate_amplitude_envelope(c, SR, **kw)
        assert np.array_equal(t, want_t) and isinstance(t, np.ndarray), i
        if d:
            assert isinstance(amp, torch.Tensor) and amp.is_cuda and amp.dtype == want.dtype and amp.shape == want.shape, i
            a, w = amp.cpu().numpy(), want.cpu().numpy()
            assert np.array_equal(again[i][0].cpu().numpy(), a)
        else:
            assert isinstance(amp, np.ndarray) and amp.shape == want.shape and amp.dtype == want.dtype, (i, amp.dtype, want.dtype)
            a, w = amp, want
            assert np.array_equal(again[i][0], a)
        if method == "RMS" and d:
            assert np.array_equal(a, w), (i, np.abs(a - w).max())
        elif method == "Hilb" and d:
            tol = TOL[np.float32 if c.dtype == torch.float32 else np.float64]
            err = np.abs(a.astype(np.float64) - w.astype(np.float64)).max()
            print(f"envelope-list Hilb {filt} clip {i}: err {err:.3e} max {np.abs(w).max():.3e}")
            assert err <= tol * np.abs(w).max(), (i, err, np.abs(w).max())
        else:
            np.testing.assert_allclose(a, w, rtol=1e-5, atol=1e-7)


def test_list_call_errors(gpu):
    rng = np.random.default_rng(2)
    long_, short = rng.standard_normal(4000).astype(np.float32), rng.standard_normal(1500).astype(np.float32)
    f = calculate_amplitude_envelope_batch
    # 1500 samples at hop 80: 19 frames, below sosfiltfilt's padlen of 21
    with pytest.raises(ValueError, match=r"greater than padlen, which is 21\. \(clip 1\)"):
        f([_dev(long_, gpu), _dev(short, gpu), long_], SR, winLen=0.05, hopLen=0.01, outFilter="iir")
    with pytest.raises(ValueError, match=r"\(clip 2\)"):
        f([long_, long_, short[:300]], SR, winLen=0.05, hopLen=0.01, center=False)          # shorter than the frame
    with pytest.raises(TypeError, match=r"\(clip 1\)"):
        f([_dev(long_, gpu), _dev(long_, gpu).half()], SR, method="Hilb")
    with pytest.raises(ValueError, match=r"\(clip 0\)"):
        f([_dev(long_, gpu)[None, :]], SR)
    with pytest.raises(NotImplementedError):
        f([long_], SR, method="RMSpraat")
    assert f([], SR) == []
