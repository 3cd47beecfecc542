"""Host only: the per-bin / per-filter bound of the STFT power and log-mel stages (stage_oracle) means something.  The float32
host pipeline sits within a small factor of the modelled floor on every configuration; the float64 reference transform agrees
with a direct long-double DFT; every deliberate break of framing, window, transform, pre-emphasis and mel walk is rejected on the case set of every
configuration of a short list; a mel weight off by 1e-4 is rejected wherever n_fft <= 2048; and the assertions the suite had
before (power to 1e-5 of the clip maximum, log-mel to 2e-3 dB) let a weight off by 1e-3 through on the c1_am golden clip."""
import numpy as np
import pytest
import scipy.signal

import mfcc_oracle as O
import modspec_oracle as M
import stage_oracle as S
from conftest import load_golden
from test_gpu_parity import _ANY_NFFT, _HALFBAND_CFGS

REF_DEFAULT = dict(sr=10000, n_fft=512, win_length=250, hop_length=50, n_mels=128, n_mfcc=13, fmin=100.0, fmax=10000.0)


def _golden(name):
    kw = load_golden(name)[0]
    return {k: kw[k] for k in ("sr", "n_fft", "win_length", "hop_length", "n_mels", "n_mfcc", "fmin", "fmax")}


def _by_nfft(n_fft):
    return next(kw for kw, _ in _ANY_NFFT if kw["n_fft"] == n_fft)


SHORT_LIST = {
    "refdefault": REF_DEFAULT,
    "c1": _golden("c1_am"),
    "c1+preemph": dict(_golden("c1_am"), preemph=0.97),
    "c4": _golden("c4_am"),
    "nfft400": _by_nfft(400),
    "nfft499": _by_nfft(499),
}
ALL_CFGS = list(SHORT_LIST.values()) + [kw for kw, _ in _ANY_NFFT] + [kw for kw, _ in _HALFBAND_CFGS]


def _cfg_id(cfg):
    return f"nfft{cfg['n_fft']}-hop{cfg['hop_length']}-mel{cfg['n_mels']}" + ("-pre" if cfg.get("preemph") else "")


@pytest.mark.parametrize("cfg", ALL_CFGS, ids=_cfg_id)
def test_float32_pipeline_sits_near_the_model(cfg):
    """C_ref per configuration (printed, shown with -s): measured 0.24 .. 5.6 for c_A and 0.6 .. 1.3 for c_L.  What is
    asserted is that range: an honest float32 pipeline lies within a small factor of the floor the measure models, so the
    bound MARGIN * max(C_ref, 1) is neither slack by orders nor below float32 round-off.  (That the pipeline itself uses at
    most half of its bound holds by the bound's definition, MARGIN = 4 >= 2, and is not a finding.)  The aligned lengths,
    which C_ref is not taken over, stay inside the bound as well."""
    cA, cL = S.c_ref(cfg)
    bA, bL = S.bounds(cfg)
    print(f"stage-cref n_fft={cfg['n_fft']} hop={cfg['hop_length']} C_A={cA:.2f} C_L={cL:.2f} bound={bA:.2f}/{bL:.2f}")
    assert (bA, bL) == (M.MARGIN * max(cA, 1.0), M.MARGIN * max(cL, 1.0)) and M.MARGIN == 4.0
    assert 0.2 <= cA <= 8.0 and 0.5 <= cL <= 2.0, (cA, cL)
    for n in S.aligned_lengths(cfg):
        assert n % 4 == 0 and n not in S.lengths(cfg)
        P, lm = S.host(cfg, n)
        ref = S.reference(cfg, n)
        assert S.power_error(P, ref).max() <= bA / 2 and S.logmel_error(lm, ref).max() <= bL / 2, n


def test_case_set():
    cfg = SHORT_LIST["c1"]
    n, n_fft, hop = 64 * cfg["hop_length"], cfg["n_fft"], cfg["hop_length"]
    x = S.cases(n, cfg)
    assert x.shape == (S.N_CASES, n) and x.dtype == np.float32 and np.array_equal(x, S.cases(n, cfg))
    assert np.array_equal(x[S.ROW_AM], O.synth_clip(1, n, cfg["sr"], "am"))
    rms = np.sqrt((x.astype(np.float64) ** 2).mean(-1))
    assert rms[S.ROW_LOUD] > 5e2 and rms[S.ROW_QUIET] < 2e-6
    assert [int(np.flatnonzero(r)[0]) for r in x[S.ROW_IMP_LAST:S.ROW_IMP_LAST + 4]] == [n - 1, 0, 1, n // 3]
    assert (x[S.ROW_CONST] == 0.75).all() and (x[S.ROW_ZERO] == 0).all()
    half = x[S.ROW_STEP].astype(np.float64)
    assert np.sqrt((half[:n // 2] ** 2).mean()) > 5e2 and np.sqrt((half[n // 2:] ** 2).mean()) < 2e-4
    ref = S.reference(cfg, n)
    assert ref.A.shape == (S.N_CASES, 65, n_fft // 2 + 1) and ref.L.shape == (S.N_CASES, 65, cfg["n_mels"])
    # the tones peak on their bins in a frame that lies inside the clip
    assert ref.A[S.ROW_TONE0:S.ROW_TONE0 + 4, 30].argmax(-1).tolist() == list(S.tone_bins(n_fft))
    # a frame holding one impulse: P[k] = w[i]^2 at every k, i the impulse's slot in the frame
    w = S.window64(cfg)
    t = (n // 3) // hop
    i = n // 3 + n_fft // 2 - t * hop
    assert np.allclose(ref.A[S.ROW_IMP_LAST + 3, t], w[i], rtol=1e-12, atol=0)
    assert S.lengths(cfg) == tuple(sorted({1, 3, 257, 63 * hop - 1, 63 * hop, 64 * hop, 65 * hop + 7}))
    assert S.lengths(_by_nfft(8192)) == (1, 4097, 8007)


def test_zero_frames_must_be_exact_and_nan_is_an_error():
    cfg = SHORT_LIST["c1"]
    ref = S.reference(cfg, 3)
    P, lm = (a.copy() for a in S.host(cfg, 3))
    assert (P[S.ROW_ZERO] == 0).all() and S.power_error(P, ref).max() <= S.bounds(cfg)[0]
    P[S.ROW_ZERO, 0, 5] = 1e-30
    assert np.isinf(S.power_error(P, ref)[S.ROW_ZERO, 0, 5])
    P[S.ROW_ZERO, 0, 5] = 0
    P[S.ROW_AM, 0, 7] = np.nan
    lm[S.ROW_AM, 3, 0] = np.nan
    assert np.isinf(S.power_error(P, ref)[S.ROW_AM, 0, 7]) and np.isinf(S.logmel_error(lm, ref)[S.ROW_AM, 0, 3])
    P[S.ROW_AM, 0, 7] = -1e-12
    assert np.isinf(S.power_error(P, ref)[S.ROW_AM, 0, 7])
    # silent frames and empty filters sit on the amin floor: held to the dB value's own rounding
    assert (ref.L[S.ROW_ZERO] == -100.0).all() and np.allclose(ref.dL[S.ROW_ZERO], 200 * M.EPS)


@pytest.mark.parametrize("n_fft", [32, 128, 256])
def test_reference_transform_agrees_with_the_long_double_dft(n_fft):
    """The windowed frames of the case clips through np.fft.rfft in float64 (what reference_of calls) against the direct
    long-double DFT: the tolerance of test_modspec_host (1e-15 of ||f|| sqrt(n))."""
    cfg = dict(sr=8000, n_fft=n_fft, win_length=n_fft - n_fft // 8, hop_length=n_fft // 4, n_mels=8, n_mfcc=4, fmin=0.0,
               fmax=4000.0, preemph=0.97)
    for n in (n_fft // 2 + 1, 3 * n_fft + 5):
        f = (S.frames_of(S.cases(n, cfg), cfg).astype(np.float64) * S.window64(cfg)).reshape(-1, n_fft)
        X = np.fft.rfft(f, axis=-1)
        # dft_longdouble takes the float32 rows it is given: transform the float64 frames as two float32 parts
        hi = f.astype(np.float32)
        lo = (f - hi).astype(np.float32)
        D = M.dft_longdouble(hi, n_fft) + M.dft_longdouble(lo, n_fft)
        scale = np.sqrt((f ** 2).sum(-1, keepdims=True)) * np.sqrt(n_fft)
        rel = np.abs(X - D) / np.where(scale > 0, scale, 1.0)
        assert float(rel.max()) <= 1e-15, (n, float(rel.max()))
        assert np.allclose(np.abs(X).reshape(S.reference(cfg, n).A.shape), S.reference(cfg, n).A, rtol=0, atol=0)


# ---- mutants: the float32 host pipeline with one defect each --------------------------------------------------------------

def _filter(cfg):
    """The filter the weight mutants touch: the middle one of those that have taps."""
    W = S.mel_weights(cfg)
    full = np.flatnonzero((W != 0).any(-1))
    return W, int(full[len(full) // 2])


def _late_frames(y, cfg):
    """Frames taken one sample late: f[t, i] = padded[t hop + i + 1]."""
    pe = np.asarray(y)
    if cfg.get("preemph"):
        a = np.float32(cfg["preemph"])
        pe = np.concatenate([y[:, :1], y[:, 1:] - a * y[:, :-1]], axis=1).astype(np.float32)
    shifted = np.concatenate([pe[:, 1:], np.zeros((y.shape[0], 1), np.float32)], axis=1)
    return S.frames_of(shifted, dict(cfg, preemph=0.0))


def _preemph_frames(y, cfg, carry):
    """Pre-emphasis done wrong.  carry: y[-1] of a row is the previous row's last sample instead of 0; otherwise sample 1
    (sample 0's successor) is passed through unfiltered."""
    a = np.float32(cfg["preemph"])
    pe = np.concatenate([y[:, :1], y[:, 1:] - a * y[:, :-1]], axis=1).astype(np.float32)
    if carry:
        pe[1:, 0] = y[1:, 0] - a * y[:-1, -1]
    elif y.shape[1] > 1:
        pe[:, 1] = y[:, 1]
    return S.frames_of(pe, dict(cfg, preemph=0.0))


def mutants(cfg, n):
    """{name: (P [B, T, bins], lm [B, n_mels, T])}."""
    y = S.cases(n, cfg)
    n_fft, win = int(cfg["n_fft"]), int(cfg["win_length"])
    P0, _ = S.host(cfg, n)
    W, m = _filter(cfg)
    amin = cfg.get("amin", 1e-10)
    out = {}

    def from_frames(name, **kw):
        out[name] = S.host_pipeline(y, cfg, **kw)

    def from_power(name, P):
        out[name] = (P, S.host_logmel(P, W, amin))

    def from_weights(name, W2):
        out[name] = (P0, S.host_logmel(P0, W2, amin))

    sym = np.zeros(n_fft)
    lpad = (n_fft - win) // 2
    sym[lpad:lpad + win] = scipy.signal.get_window("hann", win, fftbins=False)
    from_frames("symmetric-hann", window=sym)
    from_frames("window+1", window=np.roll(S.window64(cfg), 1))
    from_frames("frame+1", frames=_late_frames(y, cfg))
    k = n_fft // 8 + 3
    swapped = P0.copy()
    swapped[..., [k, k + 1]] = swapped[..., [k + 1, k]]
    from_power("swap-bins", swapped)
    gain = P0.copy()
    gain[..., k] *= np.float32(1 + 1e-3)
    from_power("bin-gain-1e-3", gain)
    if cfg.get("preemph"):
        from_frames("preemph-carry", frames=_preemph_frames(y, cfg, True))
        from_frames("preemph-skip-1", frames=_preemph_frames(y, cfg, False))
    taps = np.flatnonzero(W[m])
    big = int(taps[W[m, taps].argmax()])
    W2 = W.copy()
    W2[m, big] *= np.float32(1 + 1e-3)
    from_weights("weight-1e-3", W2)
    W2 = W.copy()
    other = m + 1 if m + 1 < W.shape[0] else m - 1
    if other >= 0:
        W2[other, big] += W2[m, big]
        W2[m, big] = 0
        from_weights("weight-moved", W2)
    W2 = W.copy()
    W2[m, int(taps[W[m, taps].argmin()])] = 0
    from_weights("smallest-tap-dropped", W2)
    return out


def _worst(cfg, pick):
    """Largest (c_A / bound_A, c_L / bound_L) of mutant `pick(cfg, n)` over the case set at every length."""
    bA, bL = S.bounds(cfg)
    worst = {}
    for n in S.lengths(cfg):
        ref = S.reference(cfg, n)
        for name, (P, lm) in pick(cfg, n).items():
            r = max(float(S.power_error(P, ref).max()) / bA, float(S.logmel_error(lm, ref).max()) / bL)
            worst[name] = max(worst.get(name, 0.0), r)
    return worst


@pytest.mark.parametrize("name", sorted(SHORT_LIST))
def test_every_mutant_is_rejected(name):
    cfg = SHORT_LIST[name]
    worst = _worst(cfg, mutants)
    expected = {"symmetric-hann", "window+1", "frame+1", "swap-bins", "bin-gain-1e-3", "weight-1e-3", "weight-moved",
                "smallest-tap-dropped"} | ({"preemph-carry", "preemph-skip-1"} if cfg.get("preemph") else set())
    assert set(worst) == expected
    for mutant, r in sorted(worst.items()):
        print(f"stage-mutant {name} {mutant}: c / bound = {r:.3g}")
        assert r > 1.0, f"{name}: {mutant} passes (c = {r:.3g} of the bound)"
    # the symmetric window is off by 1 / win_length of the window's value at most samples: orders beyond the bound
    assert worst["symmetric-hann"] > 100.0


def _weight_1e4(cfg, n):
    P0, _ = S.host(cfg, n)
    W, m = _filter(cfg)
    taps = np.flatnonzero(W[m])
    W2 = W.copy()
    W2[m, int(taps[W[m, taps].argmax()])] *= np.float32(1 + 1e-4)
    return {"weight-1e-4": (P0, S.host_logmel(P0, W2, cfg.get("amin", 1e-10)))}


@pytest.mark.parametrize("cfg", ALL_CFGS, ids=_cfg_id)
def test_a_weight_off_by_1e_4(cfg):
    """One mel weight (the largest tap of the middle filter) scaled by 1 + 1e-4 is rejected on every configuration with
    n_fft <= 2048.  Where the line lies: the impulse clips give every bin the same power, so the tap's share of its filter is
    1 / (number of taps), and the error 4.34e-4 dB x share stands against a floor of about (2 log2(n_fft) + 3) 2^-24 x 4.34 dB
    plus the dB value's rounding.  The filters of n_fft 6000, 8190 and 8192 in this suite have tens of taps and a larger
    log2(n_fft): the mutant reaches 0.57 .. 0.98 of the bound there (n_fft 4099: 2.3), and the test says so rather than tuning
    the measure.  The n_fft 2 bank (one filter, no tap on any of the two bins) has no weight to touch."""
    if not S.mel_weights(cfg).any():
        assert cfg["n_fft"] == 2
        return
    r = _worst(cfg, _weight_1e4)["weight-1e-4"]
    print(f"stage-mutant n_fft={cfg['n_fft']} weight-1e-4: c / bound = {r:.3g}")
    if cfg["n_fft"] <= 2048:
        assert r > 1.0, r
    else:
        assert r > 0.05, r            # still visible: a weight off by 2e-3 would be rejected


def test_the_old_form_lets_a_weight_off_by_1e_3_through():
    """The gap: the c1_am golden clip through the float32 pipeline with the largest tap of one filter scaled by 1 + 1e-3.
    test_stage_outputs_match_oracle's assertions (power rtol 2e-4, atol 1e-5 P.max(); log-mel 2e-3 dB; the maximum to 2e-3)
    accept it; the per-filter bound rejects it."""
    kw, y, exp = load_golden("c1_am")
    cfg = SHORT_LIST["c1"]
    assert cfg == {k: kw[k] for k in cfg} and not kw.get("preemph")
    W, m = _filter(cfg)
    taps = np.flatnonzero(W[m])
    W2 = W.copy()
    W2[m, int(taps[W[m, taps].argmax()])] *= np.float32(1 + 1e-3)
    P, lm = S.host_pipeline(y[None, :], cfg, W=W2)
    Pw = O.stft_power(y, kw["n_fft"], kw["hop_length"], kw["win_length"])
    np.testing.assert_allclose(P[0], Pw, rtol=2e-4, atol=1e-5 * Pw.max())          # the old power assertion: passes
    want = exp["logmel_unclamped"].T
    np.testing.assert_allclose(lm[0], want, rtol=0, atol=2e-3)                      # the old log-mel assertion: passes
    assert float(lm[0].max()) == pytest.approx(float(want.max()), abs=2e-3)
    ref = S.reference_of(y[None, :], cfg)
    c = S.logmel_error(lm, ref)
    assert c.max() > S.bounds(cfg)[1], (c.max(), S.bounds(cfg))                    # the per-filter bound: rejected ...
    assert np.unravel_index(c.argmax(), c.shape)[2] == m                            # ... in the filter that was touched
    assert S.logmel_error(S.host_pipeline(y[None, :], cfg)[1], ref).max() <= S.bounds(cfg)[1] / 2
