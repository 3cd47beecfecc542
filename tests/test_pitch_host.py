"""CPU: host side of the pYIN path (modulation_mfcc_amd.pitch) -- its tables and sizes against the oracle's restatement
of librosa, the banded Viterbi rule against the dense decode, oracle sanity on the test signals, and the library's
parameter validation (mm_pyin_check).  No GPU compute is called here."""
import ctypes as C

import numpy as np
import pytest

import pyin_oracle as O
from modulation_mfcc_amd import _lib
from modulation_mfcc_amd import pitch

# (sr, hop): the reference's default hop at 16 kHz, hopSize=0.005 at 22.05 / 44.1 kHz
RATES = [(16000, 160), (22050, int(0.005 * 22050)), (44100, int(0.005 * 44100))]
KINDS = ["glide", "sine200", "noise", "silence", "fade", "sine50", "sine800"]


@pytest.mark.parametrize("sr,hop", RATES)
@pytest.mark.parametrize("fmin,fmax", [(75, 600), (60.5, 410.25)])
def test_sizes_and_tables_match_oracle(sr, hop, fmin, fmax):
    z = pitch.pyin_sizes(sr, sr, fmin=fmin, fmax=fmax, hop_length=hop)
    zo = O.sizes(sr, sr, fmin, fmax, hop_length=hop)
    assert z == zo
    thr, bp, bc = pitch.beta_tables()
    tho, bpo = O.beta_probs()
    assert np.array_equal(thr, tho) and np.array_equal(bp, bpo)
    assert all(bc[k] == np.sum(bpo[:k]) for k in range(len(bc)))
    A = pitch.transition_matrix(z["n_bins"], z["width"], 0.01)
    assert np.array_equal(A, O.transition_full(z["n_bins"], z["width"], 0.01))
    H, same, cross = pitch.banded_log_transitions(z["n_bins"], z["width"], 0.01)
    Ho, so, co = O.banded_tables(A, z["n_bins"])
    assert H == Ho == (z["width"] - 1) // 2
    assert np.array_equal(same, so) and np.array_equal(cross, co)
    f = pitch.pitch_freqs(fmin, z["n_bins"], z["nbps"])
    assert np.array_equal(f, fmin * 2 ** (np.arange(zo["n_bins"]) / (12 * zo["nbps"])))


def test_reference_defaults_sizes():
    # 16 kHz, hopSize 0.01, 75-600 Hz: lags 26..214, 361 bins (722 states), band width 41, 1001 frames per 10 s
    z = pitch.pyin_sizes(160000, 16000, fmin=75, fmax=600, hop_length=160)
    assert (z["min_period"], z["max_period"], z["n_bins"], z["width"], z["n_frames"]) == (26, 214, 361, 41, 1001)


def test_boltzmann_table_matches_scipy_per_call():
    import scipy.stats
    R = pitch.max_troughs(26, 214)
    tab = pitch.boltzmann_table(R, 2)
    for N in (1, 2, 7, R - 1):
        pos = np.arange(N)
        assert np.array_equal(tab[N, :N], scipy.stats.boltzmann.pmf(pos, 2, N))
        assert not tab[N, N:].any()


@pytest.mark.parametrize("sr,hop", RATES)
@pytest.mark.parametrize("kind", KINDS)
def test_banded_viterbi_equals_dense_on_fixtures(sr, hop, kind):
    y = O.synth(kind, sr, 1.0, np.float32)
    st = O.pyin_stages(y, fmin=75, fmax=600, sr=sr, hop_length=hop)
    sd = O.viterbi_dense(st["obs"], st["A"], st["p_init"])
    sb = O.viterbi_banded(st["obs"], st["A"], st["p_init"], st["sizes"]["n_bins"])
    assert np.array_equal(sd, sb)


def test_sine_fixture_has_certain_frames():
    st = O.pyin_stages(O.synth("sine200", 16000, 1.0), fmin=75, fmax=600, sr=16000, hop_length=160)
    assert (st["voiced_prob"] == 1).sum() > 10


@pytest.mark.parametrize("seed", range(12))
def test_banded_viterbi_equals_dense_on_random_observations(seed):
    rng = np.random.default_rng(seed)
    n_bins, width, T = (37, 9, 40) if seed % 2 else (36, 9, 40)
    A = O.transition_full(n_bins, width, 0.01)
    obs = np.zeros((2 * n_bins, T))
    vp = np.zeros(T)
    for t in range(T):
        k = rng.integers(0, 4)
        bins = rng.choice(n_bins, size=k, replace=False)
        p = rng.dirichlet(np.ones(k)) * (1.0 if rng.random() < 0.3 else rng.random()) if k else np.zeros(0)
        if seed % 3 == 0 and k:
            p[:] = p[0]                                   # exact ties between bins
        obs[bins, t] = p
        vp[t] = min(max(obs[:n_bins, t].sum(), 0), 1)
        obs[n_bins:, t] = (1 - vp[t]) / n_bins
    p_init = np.zeros(2 * n_bins)
    p_init[n_bins:] = 1 / n_bins
    assert np.array_equal(O.viterbi_dense(obs, A, p_init), O.viterbi_banded(obs, A, p_init, n_bins))


@pytest.mark.parametrize("sr,hop", RATES)
@pytest.mark.parametrize("kind,f", [("sine200", 200.0), ("glide", None)])
def test_oracle_tracks_tones(sr, hop, kind, f):
    y = O.synth(kind, sr, 1.5)
    f0, voiced, vp = O.pyin_dense(y, fmin=75, fmax=600, sr=sr, hop_length=hop)
    assert voiced.mean() > 0.6
    if f is not None:
        cents = 1200 * np.abs(np.log2(f0[voiced] / f))
        assert np.median(cents) <= 10 and (cents <= 10).mean() > 0.9


@pytest.mark.parametrize("kind", ["noise", "silence"])
def test_oracle_noise_and_silence_mostly_unvoiced(kind):
    f0, voiced, vp = O.pyin_dense(O.synth(kind, 16000, 1.5), fmin=75, fmax=600, sr=16000, hop_length=160)
    assert voiced.mean() < 0.1


def _check(**kw):
    base = dict(fmin=75, fmax=600, frame_length=2048, hop_length=160)
    base.update(kw)
    sr = base.pop("sr", 16000)
    return pitch.pyin_params(16000, sr, **base)


def test_validation_accepts_defaults():
    p, z = _check()
    assert _lib.load().mm_pyin_check(C.byref(p)) == 0
    assert _lib.load().mm_pyin_num_frames(C.byref(p), 160000) == 1001


@pytest.mark.parametrize("kw", [dict(fmin=600, fmax=75), dict(fmin=300, fmax=300), dict(fmax=9000),
                                dict(win_length=2048), dict(win_length=4096)])
def test_validation_rejects_bad_parameters(kw):
    with pytest.raises(ValueError):
        _check(**kw)


def test_library_rejects_bad_parameters_directly():
    lib = _lib.load()
    p, z = _check()
    for field, value in [("fmin", 700.0), ("fmax", 8001.0), ("win_length", 2048), ("max_period", 27)]:
        q = _lib.mm_pyin_params.from_buffer_copy(p)
        setattr(q, field, value)
        assert lib.mm_pyin_check(C.byref(q)) == _lib.MM_ERR_INVALID_ARG, field


def test_validation_rejects_too_few_lags():
    # max_period < min_period + 2: frame_length - win_length - 1 leaves two lags
    with pytest.raises(ValueError):
        _check(fmin=400, fmax=8000, sr=16000, frame_length=1024, win_length=1020)
