"""GPU: the pYIN path (modulation_mfcc_amd.pitch, csrc/mm_pitch.hip) against the oracle's restatement of librosa.pyin
and of the reference's get_f0 / interp_NAN (tests/pyin_oracle.py)."""
import numpy as np
import pytest
import torch
from scipy import interpolate

import pyin_oracle as O
from modulation_mfcc_amd import pitch, get_f0, interp_NAN, pyin_batch
from modulation_mfcc_amd import calc

pytestmark = pytest.mark.gpu

RATES = [(16000, 160), (22050, int(0.005 * 22050)), (44100, int(0.005 * 44100))]
KINDS = ["glide", "sine200", "noise", "silence", "fade", "sine50", "sine800"]
DTYPES = [np.float32, np.float64]


def _dev(y, gpu):
    return torch.from_numpy(np.ascontiguousarray(y)).to(gpu)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("sr,hop", RATES)
@pytest.mark.parametrize("kind", ["glide", "noise", "fade"])
def test_cmnd_stage_matches_oracle(gpu, dtype, sr, hop, kind):
    y = O.synth(kind, sr, 1.0, dtype)
    st = O.pyin_stages(y, fmin=75, fmax=600, sr=sr, hop_length=hop)
    got = pitch.pyin_cmnd(_dev(y, gpu), sr, fmin=75, fmax=600, hop_length=hop).cpu().numpy()
    want = st["cmnd"]
    assert got.shape == want.shape
    assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max() + 1e-300


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("sr,hop", RATES)
@pytest.mark.parametrize("kind", KINDS)
def test_pyin_batch_decodes_oracle_states(gpu, dtype, sr, hop, kind):
    y = O.synth(kind, sr, 1.5, dtype)
    f0w, vw, vpw, sw = O.pyin_dense(y, fmin=75, fmax=600, sr=sr, hop_length=hop, return_states=True)
    f0, v, vp, s = pyin_batch(_dev(y, gpu), sr, fmin=75, fmax=600, hop_length=hop, return_states=True)
    assert f0.device.type == "cuda" and f0.dtype == torch.float64
    s = s.cpu().numpy()
    # voicing, f0 and every voiced state are librosa's
    assert np.array_equal(v.cpu().numpy(), vw)
    np.testing.assert_array_equal(f0.cpu().numpy(), f0w)
    bad = np.nonzero((s != sw) & vw)[0]
    assert len(bad) == 0, f"{len(bad)} voiced frames differ, first {bad[:5]}"
    assert np.abs(vp.cpu().numpy() - vpw).max() <= 1e-12
    # the observations agree to rounding (the ACF is a direct float64 sum, numpy's an FFT) ...
    st = O.pyin_stages(y, fmin=75, fmax=600, sr=sr, hop_length=hop)
    cm = pitch.pyin_cmnd(_dev(y, gpu), sr, fmin=75, fmax=600, hop_length=hop)
    cnt, bins, probs, vp2 = (a.cpu().numpy() for a in pitch.pyin_records(cm, sr, fmin=75, fmax=600, hop_length=hop))
    nb = st["sizes"]["n_bins"]
    obs = np.zeros_like(st["obs"])
    for t in range(len(cnt)):
        obs[bins[t, :cnt[t]], t] = probs[t, :cnt[t]]
    obs[nb:] = (1 - vp2)[None] / nb
    assert np.abs(obs - st["obs"]).max() <= 1e-12
    # ... and the device decode is librosa's dense Viterbi of the device observations, state for state (the bin of an
    # unvoiced frame inside a flat stretch is decided by those last-bit differences, so it is pinned here)
    np.testing.assert_array_equal(s, O.viterbi_dense(obs, st["A"], st["p_init"]))
    if kind == "sine200":
        assert (vpw == 1).any()                          # the fixture really has certain frames


def test_mixed_batch_equals_single_rows(gpu):
    sr = 16000
    rows = np.stack([O.synth(k, sr, 1.2, np.float32, seed=i) for i, k in
                     enumerate(["silence", "noise", "glide", "sine200", "fade"])])
    fb, vb, pb, sb = pyin_batch(_dev(rows, gpu), sr, fmin=75, fmax=600, hop_length=160, return_states=True)
    for i in range(len(rows)):
        f1, v1, p1, s1 = pyin_batch(_dev(rows[i], gpu), sr, fmin=75, fmax=600, hop_length=160, return_states=True)
        assert torch.equal(sb[i], s1) and torch.equal(vb[i], v1) and torch.equal(pb[i], p1)
        assert torch.equal(torch.nan_to_num(fb[i], nan=-1.0), torch.nan_to_num(f1, nan=-1.0))


def test_chunked_batch_equals_unchunked(gpu, monkeypatch):
    sr = 16000
    rows = np.stack([O.synth(k, sr, 1.0, np.float64, seed=i) for i, k in
                     enumerate(["glide", "noise", "sine200", "fade"] * 3)])
    x = _dev(rows, gpu)
    whole = pyin_batch(x, sr, fmin=75, fmax=600, hop_length=160, return_states=True)
    # one row of scratch per call: 12 calls
    monkeypatch.setattr(pitch, "PYIN_WS_BYTES", 1)
    parts = pyin_batch(x, sr, fmin=75, fmax=600, hop_length=160, return_states=True)
    for a, b in zip(whole, parts):
        assert torch.equal(torch.nan_to_num(a.double(), nan=-1.0), torch.nan_to_num(b.double(), nan=-1.0))


def test_long_recording_against_banded_oracle(gpu):
    sr, hop = 16000, int(0.005 * 16000)
    y = O.synth("glide", sr, 60.0, np.float32)
    st = O.pyin_stages(y, fmin=75, fmax=600, sr=sr, hop_length=hop)
    assert st["sizes"]["n_frames"] == 12001
    sw = O.viterbi_banded(st["obs"], st["A"], st["p_init"], st["sizes"]["n_bins"])
    f0, v, vp, s = pyin_batch(_dev(y, gpu), sr, fmin=75, fmax=600, hop_length=hop, return_states=True)
    s = s.cpu().numpy()
    assert np.array_equal(v.cpu().numpy(), sw < st["sizes"]["n_bins"])
    assert np.array_equal(s[sw < st["sizes"]["n_bins"]], sw[sw < st["sizes"]["n_bins"]])
    assert np.abs(vp.cpu().numpy() - st["voiced_prob"]).max() <= 1e-12


def _nan_curve(n, lead, tail, seed=0):
    rng = np.random.default_rng(seed)
    x = 100 + np.cumsum(rng.standard_normal(n))
    x[rng.random(n) < 0.3] = np.nan
    x[:lead] = np.nan
    if tail:
        x[-tail:] = np.nan
    x[n // 3:n // 3 + 50] = np.nan
    return x


@pytest.mark.parametrize("lead,tail", [(0, 0), (7, 0), (0, 9), (13, 21)])
def test_interp_nan_linear_matches_scipy(gpu, lead, tail):
    x = _nan_curve(3001, lead, tail, seed=lead + tail)
    m = np.isnan(x)
    want = x.copy()
    f = interpolate.interp1d(np.where(~m)[0], x[~m], "linear", fill_value="extrapolate")
    want[m] = f(np.where(m)[0])
    got = interp_NAN(x, "linear")
    assert isinstance(got, np.ndarray)
    assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()
    d = interp_NAN(_dev(x, gpu), "linear")
    assert d.device.type == "cuda"
    np.testing.assert_array_equal(d.cpu().numpy(), got)
    rows = np.stack([_nan_curve(3001, lead, tail, seed=s) for s in range(5)])
    dr = interp_NAN(_dev(rows, gpu), "linear").cpu().numpy()
    for r in range(5):
        np.testing.assert_array_equal(dr[r], interp_NAN(rows[r], "linear"))


def test_interp_nan_other_methods_are_the_reference(gpu):
    x = _nan_curve(500, 3, 4)
    for method in ("pchip", "nearest", "cubic"):
        np.testing.assert_array_equal(interp_NAN(x, method), O.interp_NAN(x, method))


@pytest.mark.parametrize("mmq", [None, [0.05, 0.95]])
@pytest.mark.parametrize("dtype", DTYPES)
def test_get_f0_pyin_end_to_end(gpu, mmq, dtype):
    sr = 16000
    y = O.synth("glide", sr, 3.0, dtype)
    f0, f0t = get_f0(y, sr, method="pyin", interpUnvoiced="linear", outFilter="iir", outFiltCutOff=[12],
                     minMaxQuant=mmq)
    wf, wt = O.get_f0(y, sr, interpUnvoiced="linear", outFilter="iir", outFiltCutOff=[12], minMaxQuant=mmq)
    assert isinstance(f0, np.ndarray) and f0.shape == wf.shape
    np.testing.assert_array_equal(f0t, wt)
    assert np.abs(f0 - wf).max() <= 1e-9 * np.abs(wf).max()
    assert calc.get_f0 is get_f0


def test_get_f0_integer_pcm_and_device_input(gpu):
    sr = 16000
    y = np.round(O.synth("glide", sr, 2.0) * 20000).astype(np.int16)
    f0, f0t = get_f0(y, sr, method="pyin", outFiltCutOff=[12])
    wf, _ = O.get_f0(y.astype(np.float64), sr, outFiltCutOff=[12])
    assert np.abs(f0 - wf).max() <= 1e-9 * np.abs(wf).max()
    d, dt = get_f0(_dev(y.astype(np.float64), gpu), sr, method="pyin", outFiltCutOff=[12])
    assert isinstance(d, torch.Tensor) and d.device.type == "cuda"
    np.testing.assert_array_equal(dt, f0t)
    assert np.abs(d.cpu().numpy() - f0).max() <= 1e-12 * np.abs(f0).max()


def test_get_f0_error_paths(gpu):
    y = O.synth("glide", 16000, 1.0)
    for m in ("praatac", "praatcc"):
        with pytest.raises(NotImplementedError):
            get_f0(y, 16000, method=m)
    with pytest.raises(Exception, match="unvoiced regions are not interpolated"):
        get_f0(y, 16000, method="pyin", interpUnvoiced=None, outFilter="iir")
    f0, _ = get_f0(y, 16000, method="pyin", interpUnvoiced=None, outFilter=None)
    assert np.isnan(f0).any()
