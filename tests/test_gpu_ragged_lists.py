"""GPU (-m gpu): the four list front ends on ONE mixed list -- get_f0_batch, calculate_amplitude_envelope_batch,
get_MFCCS_change_batch, applyFilter_batch.  Five clips at 16 kHz of 4000, 2500, 4000, 3100 and 2500 samples, given as numpy
float32, numpy float64, numpy int16, device float32 and device float64: two dtype groups, a length repeated within a group
and across the groups, and both return types.  Entry i of every result is the single call on clip i alone, under the
comparison that front end's own batch-versus-single test uses; a clip too short for the output filter raises the single
call's error with its index."""
import numpy as np
import pytest
import torch

import mfcc_oracle as O
from modulation_mfcc_amd import (applyFilter, applyFilter_batch, calculate_amplitude_envelope,
                                 calculate_amplitude_envelope_batch, get_f0, get_f0_batch, get_MFCCS_change,
                                 get_MFCCS_change_batch)

pytestmark = pytest.mark.gpu

SR = 16000
LENGTHS = [4000, 2500, 4000, 3100, 2500]
# a hop of 32 samples: the shortest clip has 79 frames, more than sosfiltfilt's padlen of 21
F0 = dict(method="pyin", hopSize=0.002, minPitch=100, maxPitch=500, pyinframe_length=512, interpUnvoiced="linear",
          outFilter="iir", outFiltCutOff=[10])                         # (the cut-off of test_get_f0_batch_equals_get_f0)
ENV = dict(winLen=0.01, hopLen=0.002, outFilter="iir")
CHANGE = dict(outFiltCutOff=[12])      # the defaults; outFiltCutOff has none that applyFilter takes ([None])
HILBERT_TOL = {torch.float32: 2e-5, torch.float64: 1e-11}             # test_gpu_envelope_ragged.TOL, of the envelope's maximum


def _clips(gpu, lengths=LENGTHS):
    x = [np.asarray(O.synth_clip(seed, n, SR, "am"), dtype=np.float64) for seed, n in enumerate(lengths)]
    return [x[0].astype(np.float32), x[1], np.round(x[2] * 20000).astype(np.int16),
            torch.from_numpy(x[3].astype(np.float32)).to(gpu), torch.from_numpy(x[4]).to(gpu)]


def _same_kind(got, want, clip, i):
    """numpy for a numpy clip, a device tensor for a device clip; the single call's dtype and length"""
    if isinstance(clip, torch.Tensor):
        assert isinstance(got, torch.Tensor) and got.is_cuda and got.dtype == want.dtype and got.shape == want.shape, i
        return got.cpu().numpy(), want.cpu().numpy()
    assert isinstance(got, np.ndarray) and got.dtype == want.dtype and got.shape == want.shape, i
    return got, want


def _refusal(batch_call, single_call, suffix=" (clip 3)"):
    with pytest.raises(ValueError) as one:
        single_call()
    with pytest.raises(ValueError) as many:
        batch_call()
    assert str(many.value) == str(one.value) + suffix


def test_get_f0_batch(gpu):
    clips = _clips(gpu)
    got = get_f0_batch(clips, SR, **F0)
    assert len(got) == 5
    for i, (c, (f0, f0t)) in enumerate(zip(clips, got)):
        wf, wt = get_f0(c, SR, **F0)
        a, w = _same_kind(f0, wf, c, i)
        assert isinstance(f0t, np.ndarray) and f0t.dtype == wt.dtype
        np.testing.assert_array_equal(f0t, wt)
        np.testing.assert_array_equal(a, w, err_msg=f"clip {i}")      # bit for bit (NaN in the same places)
    assert [len(t) for _, t in got] == [1 + n // 32 for n in LENGTHS]
    short = _clips(gpu, LENGTHS[:3] + [600] + LENGTHS[4:])              # 19 frames
    _refusal(lambda: get_f0_batch(short, SR, **F0), lambda: get_f0(short[3], SR, **F0))


@pytest.mark.parametrize("method", ["RMS", "Hilb"])
def test_calculate_amplitude_envelope_batch(method, gpu):
    clips = _clips(gpu)
    got = calculate_amplitude_envelope_batch(clips, SR, method=method, **ENV)
    assert len(got) == 5
    for i, (c, (amp, t)) in enumerate(zip(clips, got)):
        want, want_t = calculate_amplitude_envelope(c, SR, method=method, **ENV)
        a, w = _same_kind(amp, want, c, i)
        assert isinstance(t, np.ndarray) and np.array_equal(t, want_t), i
        on_device = isinstance(c, torch.Tensor)
        if method == "RMS" and on_device:
            assert np.array_equal(a, w), (i, np.abs(a - w).max())
        elif method == "Hilb" and on_device:
            err = np.abs(a.astype(np.float64) - w.astype(np.float64)).max()
            print(f"list envelope Hilb clip {i}: err {err:.3e} max {np.abs(w).max():.3e}")
            assert err <= HILBERT_TOL[c.dtype] * np.abs(w).max(), (i, err, np.abs(w).max())
        else:                              # a numpy clip: its single call filters with scipy on the host
            np.testing.assert_allclose(a, w, rtol=1e-5, atol=1e-7)
    n_short = 600 if method == "RMS" else 20                            # 19 frames; 20 samples of envelope
    short = _clips(gpu, LENGTHS[:3] + [n_short] + LENGTHS[4:])
    _refusal(lambda: calculate_amplitude_envelope_batch(short, SR, method=method, **ENV),
             lambda: calculate_amplitude_envelope(short[3], SR, method=method, **ENV))


def test_get_MFCCS_change_batch(gpu):
    clips = _clips(gpu)
    got = get_MFCCS_change_batch(clips, SR, **CHANGE)
    assert len(got) == 5
    for i, (c, (tot, anchors)) in enumerate(zip(clips, got)):
        want, want_anchors = get_MFCCS_change(c, SR, **CHANGE)          # numpy pairs for every kind of clip
        assert isinstance(tot, np.ndarray) and tot.dtype == want.dtype == np.float64 and tot.shape == want.shape, i
        np.testing.assert_array_equal(anchors, want_anchors)
        # test_end_to_end_from_audio's bound for a float32 MFCC feeding the float64 tail: 1e-4 of the curve's maximum.  (The
        # single call takes the MFCC from the kernel with the DCT fused in, the ragged one from the separate clamp + DCT
        # launch, DESIGN 12: equal to float32 rounding, not bit for bit -- 7.6e-8 of the maximum here.)
        err = np.abs(tot - want).max()
        print(f"list change clip {i}: err {err:.3e} max {np.abs(want).max():.3e}")
        assert err <= 1e-4 * np.abs(want).max(), (i, err)
    assert [len(t) for t, _ in got] == [1 + n // 16 for n in LENGTHS]
    short = _clips(gpu, LENGTHS[:3] + [300] + LENGTHS[4:])              # 19 frames at the default step of 1 ms
    _refusal(lambda: get_MFCCS_change_batch(short, SR, **CHANGE), lambda: get_MFCCS_change(short[3], SR, **CHANGE),
             " (clip 3 has 19 frames)")


@pytest.mark.parametrize("kw", [dict(filt="sg", cutOff=[1000], filtLen=7), dict(filt="iir", cutOff=[1000])], ids=["sg", "iir"])
def test_applyFilter_batch(kw, gpu):
    clips = _clips(gpu)
    try:                                   # the int16 clip stays in the list unless applyFilter itself refuses it
        applyFilter(clips[2], float(SR), **kw)
    except Exception:
        del clips[2]
    at = len(clips) - 2                    # the place of the device float32 clip
    got = applyFilter_batch(clips, float(SR), **kw)
    assert len(got) == len(clips)
    for i, (c, g) in enumerate(zip(clips, got)):
        a, w = _same_kind(g, applyFilter(c, float(SR), **kw), c, i)
        np.testing.assert_array_equal(a, w, err_msg=f"{kw} curve {i}")
    short = clips[:at] + [clips[at][:5]] + clips[at + 1:]
    _refusal(lambda: applyFilter_batch(short, float(SR), **kw), lambda: applyFilter(short[at], float(SR), **kw), f" (curve {at})")
