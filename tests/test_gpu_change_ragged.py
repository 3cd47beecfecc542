"""GPU (-m gpu): the MFCC-change tail with a frame count per clip (mm_mfcc_change_ragged_f64, MfccPlan.mfcc_change_ragged,
tail.mfcc_change_ragged_device, mfcc_change_ragged_batch, get_MFCCS_change_batch).

The expected value is always scipy's arithmetic on the clip ALONE, O.mfcc_change_tail(m[b, :, :T_b], ...), within the
project's tolerance for this tail: 1e-10 of the curve's maximum (test_change_tail_on_device).  Inputs are float32 random
walks as test_change_tail_many_rows_and_long_batches builds them; the columns behind T_b hold NaN unless a test says
otherwise."""
import contextlib
import ctypes as C
import functools

import numpy as np
import pytest

import mfcc_oracle as O

pytestmark = pytest.mark.gpu

C1 = dict(sr=16000, n_fft=512, win_length=400, hop_length=160, n_mels=40, n_mfcc=13, fmin=100.0, fmax=8000.0)
TOL = 1e-10
KW = dict(tStep=0.01, outFiltCutOff=[12])      # order-6 Butterworth twice: three sections, padlen 21


def _plan():
    from modulation_mfcc_amd import MfccConfig, get_plan
    return get_plan(MfccConfig(**C1))


def _dev(x, gpu):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).to(gpu)


@functools.lru_cache(maxsize=None)
def _walk(seed, B, T):
    m = np.random.default_rng(seed).standard_normal((B, 13, T)).cumsum(axis=2).astype(np.float32)
    m.setflags(write=False)
    return m


def _ragged(m, frames, fill=np.nan):
    a = m.copy()
    for b, T in enumerate(frames):
        a[b, :, T:] = fill
    return a


def _key(kw):
    return tuple(sorted((k, tuple(v) if isinstance(v, list) else v) for k, v in kw.items()))


@functools.lru_cache(maxsize=None)
def _want(seed, B, Tm, b, T, key):
    """The reference curve of clip b of _walk(seed, B, Tm) cut to T frames, alone (computed once, shared, read-only)."""
    kw = {k: list(v) if isinstance(v, tuple) else v for k, v in key}
    w = O.mfcc_change_tail(_walk(seed, B, Tm)[b, :, :T], **kw)
    w.setflags(write=False)
    return w


def _check(got, seed, Tm, frames, kw, what):
    """Every clip against the reference on the clip alone, no NaN inside [0, T_b), exact +0.0 behind it."""
    B = len(frames)
    assert got.shape == (B, Tm) and got.dtype == np.float64
    for b, T in enumerate(frames):
        want = _want(seed, B, Tm, b, T, _key(kw))
        assert want.shape == (T,)
        assert not np.isnan(got[b, :T]).any(), f"{what} clip {b} T={T}: NaN inside the clip"
        err = np.abs(got[b, :T] - want).max()
        assert err <= TOL * np.abs(want).max(), f"{what} clip {b} T={T}: {err:.3e} vs {TOL * np.abs(want).max():.3e}"
        tail = got[b, T:]
        assert (tail == 0.0).all() and not np.signbit(tail).any(), f"{what} clip {b} T={T}: columns behind T_b are not +0.0"


@contextlib.contextmanager
def _single_length_calls(plan):
    """Counts the plan's mfcc_change() calls: the per-length fallback of mfcc_change_ragged() goes through them."""
    calls, orig = [], plan.mfcc_change

    def counted(mfcc, *a, **k):
        calls.append(tuple(mfcc.shape))
        return orig(mfcc, *a, **k)
    plan.mfcc_change = counted
    try:
        yield calls
    finally:
        del plan.mfcc_change


def test_every_length_of_a_small_shape(gpu):
    """T_max = 76, one clip for every T_b from padlen + 1 = 22 to 76: the filters' chunk is 3 samples here (118 extended
    samples over 64 chunks), so the clips end at every position of a chunk.  And the motivation: the single-length call on
    the zero-padded batch is NOT the curve of a shorter clip."""
    from modulation_mfcc_amd import tail
    plan = _plan()
    Tm, frames = 76, list(range(22, 77))
    m = _walk(1, len(frames), Tm)
    with _single_length_calls(plan) as calls:
        got = tail.mfcc_change_ragged_device(plan, _dev(_ragged(m, frames), gpu), frames, **KW).cpu().numpy()
    assert not calls
    _check(got, 1, Tm, frames, KW, "every length")
    padded = tail.mfcc_change_device(plan, _dev(_ragged(m, frames, 0.0), gpu), **KW).cpu().numpy()
    worst = 0.0
    for b, T in enumerate(frames[:-1]):
        want = _want(1, len(frames), Tm, b, T, _key(KW))
        worst = max(worst, np.abs(padded[b, :T] - want).max() / np.abs(want).max())
    assert worst > TOL, "the zero-padded single-length call equals the per-clip curve: these inputs cannot tell them apart"
    want = _want(1, len(frames), Tm, len(frames) - 1, Tm, _key(KW))            # the full-length clip: the same call is right
    assert np.abs(padded[-1] - want).max() <= TOL * np.abs(want).max()


def test_rows_in_groups(gpu):
    """T_max = 3001: the 12 rows of a clip do not fit LDS at once (three groups of four), clips from the shortest scipy
    takes to the full row."""
    from modulation_mfcc_amd import tail
    plan = _plan()
    Tm, frames = 3001, [22, 1500, 2999, 3000, 3001, 64]
    m = _walk(2, len(frames), Tm)
    with _single_length_calls(plan) as calls:
        got = tail.mfcc_change_ragged_device(plan, _dev(_ragged(m, frames), gpu), frames, **KW).cpu().numpy()
    assert not calls
    _check(got, 2, Tm, frames, KW, "groups")


@pytest.mark.parametrize("kwargs,in_kernel", [
    (dict(outFilter=None), True),
    (dict(outFiltCutOff=[12]), True),
    (dict(outFiltType="band", outFiltCutOff=[2, 20], outFiltLen=4), True),       # four sections, padlen 27
    (dict(outFiltType="high", outFiltCutOff=[3]), True),
    (dict(removeFirst=0, outFiltCutOff=[20]), True),
    (dict(diffMethod="sg", outFiltCutOff=[12]), True),
    (dict(diffMethod="sg", outFilter=None, removeFirst=0), True),
    (dict(filtOrd=5, filtCutoff=8, outFiltCutOff=[10], outFiltLen=3), True),      # odd orders: a section with a zero
    (dict(outFilter="fir", outFiltCutOff=[12]), True),
    (dict(outFilter="sg", outFiltCutOff=[12], outFiltLen=7, outFiltPolyOrd=3), True),
    (dict(outFiltType="band", outFiltCutOff=[2, 20]), False),                     # six sections: the per-length route
])
def test_filters_and_differentiators(kwargs, in_kernel, gpu):
    from modulation_mfcc_amd import tail
    plan = _plan()
    Tm, frames = 300, [300, 40, 211, 64, 123]
    kw = dict(tStep=0.01, **kwargs)
    m = _walk(3, len(frames), Tm)
    with _single_length_calls(plan) as calls:
        got = tail.mfcc_change_ragged_device(plan, _dev(_ragged(m, frames), gpu), frames, **kw).cpu().numpy()
    assert (not calls) == in_kernel, calls
    _check(got, 3, Tm, frames, kw, str(kwargs))


def test_row_independence(gpu):
    """The same clip at the same T_b in two batches of one T_max, other neighbours, other neighbour lengths, and NaN, zeros
    or another clip's values behind T_b: equal bits.  Against the single-length call on the clip alone: rounding only (the
    chunk length differs, so not bit for bit)."""
    import torch
    from modulation_mfcc_amd import tail
    plan = _plan()
    Tm, T = 200, 137
    m = _walk(4, 4, Tm)
    x = m[0]

    def run(rows, frames, pos):
        return tail.mfcc_change_ragged_device(plan, _dev(np.stack(rows), gpu), frames, **KW)[pos].clone()
    nan, zero = (_ragged(x[None], [T], f)[0] for f in (np.nan, 0.0))
    other = x.copy()
    other[:, T:] = m[3][:, T:] * 7.0
    a = run([nan, m[1], _ragged(m[2][None], [30])[0]], [T, Tm, 30], 0)
    b = run([_ragged(m[3][None], [64])[0], _ragged(m[1][None], [199])[0], zero], [64, 199, T], 2)
    c = run([m[2], other], [Tm, T], 1)
    assert not torch.isnan(a[:T]).any()
    assert torch.equal(a, b) and torch.equal(a, c)
    alone = tail.mfcc_change_device(plan, _dev(np.ascontiguousarray(x[None, :, :T]), gpu), **KW)[0].cpu().numpy()
    assert np.abs(a[:T].cpu().numpy() - alone).max() <= TOL * np.abs(alone).max()
    # and the whole call again: reproducible bit for bit
    assert torch.equal(a, run([nan, m[1], _ragged(m[2][None], [30])[0]], [T, Tm, 30], 0))


def test_device_lengths(gpu):
    """An int64 device tensor goes through with no read-back: the same bits as host lengths; 0 and T_max + 5 are clamped,
    a clip of 10 frames (<= padlen 21) comes out NaN in [0, 10) and zero behind, its neighbours stay right."""
    import torch
    from modulation_mfcc_amd import tail
    plan = _plan()
    Tm = 150
    dev_frames = [150, 0, 77, Tm + 5, 10, 22]
    eff_frames = [150, 1, 77, Tm, 10, 22]
    host_frames = [150, 30, 77, Tm, 30, 22]                  # valid stand-ins in the rows a host call would refuse
    m = _dev(_ragged(_walk(5, 6, Tm), eff_frames), gpu)
    fr = torch.tensor(dev_frames, dtype=torch.int64, device=gpu)
    got = tail.mfcc_change_ragged_device(plan, m, fr, **KW)
    host = tail.mfcc_change_ragged_device(plan, m, host_frames, **KW)
    g = got.cpu().numpy()
    for b in (0, 2, 3, 5):
        assert torch.equal(got[b], host[b])
        want = _want(5, 6, Tm, b, eff_frames[b], _key(KW))
        assert np.abs(g[b, :eff_frames[b]] - want).max() <= TOL * np.abs(want).max()
        assert (g[b, eff_frames[b]:] == 0.0).all() and not np.signbit(g[b, eff_frames[b]:]).any()
    for b in (1, 4):
        T = eff_frames[b]
        assert np.isnan(g[b, :T]).all()
        assert (g[b, T:] == 0.0).all() and not np.signbit(g[b, T:]).any()
    with pytest.raises(TypeError):
        plan.mfcc_change_ragged(m, fr.to(torch.int32), tail.design_lowpass(6, 12, 0.01))
    with pytest.raises(ValueError, match="padlen, which is 21"):
        tail.mfcc_change_ragged_device(plan, m, eff_frames, **KW)        # the same lengths on the host: scipy's refusal


@pytest.mark.parametrize("Tm,frames,kwargs", [
    (150, [150, 34, 90, 90], dict(filtOrd=10, outFiltCutOff=[12])),       # five sections, padlen 33
    (12001, [12001, 40, 5000], dict(outFiltCutOff=[12])),                 # one row and the curve do not fit LDS
])
def test_fallback_per_distinct_length(Tm, frames, kwargs, gpu):
    from modulation_mfcc_amd import tail
    plan = _plan()
    kw = dict(tStep=0.01, **kwargs)
    m = _walk(6, len(frames), Tm)
    with _single_length_calls(plan) as calls:
        got = tail.mfcc_change_ragged_device(plan, _dev(_ragged(m, frames), gpu), frames, **kw).cpu().numpy()
    assert sorted(c[2] for c in calls) == sorted(set(frames))
    _check(got, 6, Tm, frames, kw, f"fallback T_max={Tm}")


def test_c_entry_checks_fire_before_any_launch(gpu):
    """The checks of mm_mfcc_change_ragged_f64 behind a valid plan: the output keeps its sentinel in every refused call."""
    import torch
    from modulation_mfcc_amd import _lib, tail
    plan = _plan()
    lib, h = plan._lib, plan._h
    B, Tm = 3, 100
    s3 = np.ascontiguousarray(tail.design_lowpass(6, 12, 0.01))
    s5 = np.ascontiguousarray(tail.design_lowpass(10, 12, 0.01))
    assert s3.shape == (3, 6) and s5.shape == (5, 6)
    q = lib.mm_change_ragged_workspace_bytes_for
    need = int(q(h, B, Tm, 1, s3.ctypes.data, 3, s3.ctypes.data, 3))
    assert 0 < need < (1 << 16)
    assert q(h, 0, Tm, 1, s3.ctypes.data, 3, s3.ctypes.data, 3) == 0
    assert q(h, B, 0, 1, s3.ctypes.data, 3, s3.ctypes.data, 3) == 0
    assert q(h, B, Tm, 13, s3.ctypes.data, 3, s3.ctypes.data, 3) == 0
    assert q(h, B, Tm, 1, s3.ctypes.data, 0, s3.ctypes.data, 3) == 0
    m = torch.zeros((B, 13, Tm), dtype=torch.float32, device=gpu)
    big = torch.zeros((1, 13, 30000), dtype=torch.float32, device=gpu)
    fr = torch.full((B,), Tm, dtype=torch.int64, device=gpu)
    out = torch.full((B, 30000), 7.0, dtype=torch.float64, device=gpu)
    ws = torch.empty(1 << 20, dtype=torch.uint8, device=gpu)
    st = C.c_void_p(torch.cuda.current_stream(gpu).cuda_stream)

    def call(mf=m, n=Tm, frames=fr.data_ptr(), rf=1, dm=0, s1=s3, s2=s3, n2=None, wsb=ws.numel()):
        return lib.mm_mfcc_change_ragged_f64(h, mf.data_ptr(), mf.shape[0], n, frames, rf, dm, s1.ctypes.data, s1.shape[0],
                                             s2.ctypes.data, s2.shape[0] if n2 is None else n2, out.data_ptr(), ws.data_ptr(),
                                             wsb, st)
    assert call(frames=None) == _lib.MM_ERR_INVALID_ARG
    assert call(dm=2) == _lib.MM_ERR_INVALID_ARG and call(dm=-1) == _lib.MM_ERR_INVALID_ARG
    assert call(rf=13) == _lib.MM_ERR_INVALID_ARG
    assert call(n=21) == _lib.MM_ERR_INVALID_ARG                    # not even the longest clip exceeds padlen
    assert call(wsb=need - 1) == _lib.MM_ERR_WORKSPACE
    assert call(s1=s5) == _lib.MM_ERR_UNSUPPORTED and call(s2=s5) == _lib.MM_ERR_UNSUPPORTED
    assert call(mf=big, n=30000) == _lib.MM_ERR_UNSUPPORTED         # 12 rows x 30 000 frames: not one row fits LDS
    assert int(q(h, 1, 30000, 1, s3.ctypes.data, 3, s3.ctypes.data, 3)) > 0
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    assert call(wsb=need) == _lib.MM_OK
    torch.cuda.synchronize()
    flat = out.view(-1)                                             # the call writes [B][Tm] doubles from the start
    assert not bool((flat[:B * Tm] == 7.0).any()) and bool((flat[B * Tm:] == 7.0).all())


def test_fuse_tail_switch_does_not_affect_the_ragged_call(gpu):
    import torch
    from modulation_mfcc_amd import tail
    plan = _plan()
    Tm, frames = 300, [300, 40, 211, 64, 123]
    m = _dev(_ragged(_walk(3, len(frames), Tm), frames), gpu)
    a = tail.mfcc_change_ragged_device(plan, m, frames, **KW)
    prev = plan.set_fuse_tail(False)
    try:
        with _single_length_calls(plan) as calls:
            b = tail.mfcc_change_ragged_device(plan, m, frames, **KW)
    finally:
        plan.set_fuse_tail(prev)
    assert not calls and torch.equal(a, b)


LENGTHS_E2E = (3521, 3680, 5000, 10240, 10241, 12001)      # 23 .. 76 frames at hop 160: every clip longer than padlen 21


def test_end_to_end_from_audio(gpu):
    """Audio -> ragged MFCC -> ragged tail with nothing leaving the device, and the list form, against the reference's
    whole function on each clip alone (O.get_MFCCS_change).  Tolerance: that of test_drop_in_get_MFCCS_change for a
    float32 MFCC feeding the float64 tail, 1e-4 of the curve's maximum."""
    import torch
    from modulation_mfcc_amd import MfccConfig, get_MFCCS_change_batch, mfcc_change_ragged_batch
    sr, n_max = 16000, 12001
    ref = dict(tStep=0.01, winLen=0.025, n_mfcc=13, n_fft=512, minFreq=100, maxFreq=8000)
    clips = [O.synth_clip(b, n_max, sr, "am")[:L] for b, L in enumerate(LENGTHS_E2E)]
    want = [O.get_MFCCS_change(y, sr, outFiltCutOff=[12], **ref) for y in clips]
    audio = np.full((len(clips), n_max), np.nan, dtype=np.float32)
    for b, y in enumerate(clips):
        audio[b, :len(y)] = y
    cfg = MfccConfig.from_reference_call(sr, **ref)
    change, frames = mfcc_change_ragged_batch(_dev(audio, gpu), list(LENGTHS_E2E), cfg, tStep=0.01, outFiltCutOff=[12])
    assert change.is_cuda and change.dtype == torch.float64 and frames.is_cuda and frames.dtype == torch.int64
    assert frames.tolist() == [len(w[0]) for w in want] == [1 + L // 160 for L in LENGTHS_E2E]
    got = change.cpu().numpy()
    assert got.shape == (len(clips), 1 + n_max // 160)
    for b, (tot, _) in enumerate(want):
        T = len(tot)
        assert np.abs(got[b, :T] - tot).max() <= 1e-4 * np.abs(tot).max(), (b, np.abs(got[b, :T] - tot).max() / np.abs(tot).max())
        assert (got[b, T:] == 0.0).all() and not np.signbit(got[b, T:]).any()
    pairs = get_MFCCS_change_batch([clips[0], _dev(clips[1], gpu), np.stack([clips[2], 0 * clips[2]])] + clips[3:], sr,
                                   channelN=0, outFiltCutOff=[12], **ref)
    assert len(pairs) == len(clips)
    for b, ((tot, anchors), (wtot, wanchors)) in enumerate(zip(pairs, want)):
        assert isinstance(tot, np.ndarray) and tot.dtype == np.float64 and tot.shape == wtot.shape
        np.testing.assert_array_equal(tot, got[b, :len(wtot)])
        np.testing.assert_array_equal(anchors, wanchors)
    with pytest.raises(ValueError, match=r"padlen, which is 21\. \(clip 1 "):
        get_MFCCS_change_batch([clips[0], clips[1][:3200]], sr, outFiltCutOff=[12], **ref)       # 21 frames
