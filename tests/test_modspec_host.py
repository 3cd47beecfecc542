"""Host only: the per-bin bound of the modulation spectrum (modspec_oracle) means something.  An independent float32 FFT
passes it at every length and every zero-padding edge; the float64 reference agrees with a direct long-double DFT; every
deliberate break of the transform -- a lost bin, a wrong sign, a gain, a mask off by one, a sample of the next row -- is
rejected on at least one row of the case set at every length, while the former  1e-4 x global maximum  form lets a zeroed
bin of a real MFCC trajectory through."""
import numpy as np
import pytest

import mfcc_oracle as O
import modspec_oracle as M
from conftest import load_golden

LENGTHS = (32, 128, 512, 1024, 2048, 8192)
# the largest margin at which every mutant below is still rejected at every length (measured: the gain and Nyquist mutants at
# n = 8192 reach 33 x max(C_ref, 1)); test_margin_has_room asserts MARGIN stays under it
LARGEST_MARGIN = 33.0
_BINS = lambda n: (1, n // 4 + 1, n // 2 - 1)      # noqa: E731  (bins with an imaginary part and a neighbour above)


def _zero(Y, k):
    Y[:, k] = 0


def _conj(Y, k):
    Y[:, k] = np.conj(Y[:, k])


def _swap(Y, k):
    Y[:, [k, k + 1]] = Y[:, [k + 1, k]]


def mutants(x, n):
    """{name: spectrum complex64 [rows, n / 2 + 1]}: the float32 reference transform of x with one defect each."""
    T = x.shape[-1]
    Y = M.rfft32(x, n)
    out = {}
    for name, fn in (("zero", _zero), ("conj", _conj), ("swap", _swap)):
        for k in _BINS(n):
            out[f"{name}@{k}"] = Y.copy()
            fn(out[f"{name}@{k}"], k)
    out["gain"] = (Y * np.float32(1 + 1e-5)).astype(np.complex64)
    short = x.copy()
    short[:, T - 1] = 0                                 # the mask stops one sample early
    out["mask-1"] = M.rfft32(short, n)
    if T < n:                                           # the mask stops one sample late: sample T is the next row's first
        longer = np.zeros((x.shape[0], T + 1), dtype=np.float32)
        longer[:, :T] = x
        longer[:, T] = np.roll(x[:, 0], -1)
        out["mask+1"] = M.rfft32(longer, n)
    nyq = Y.copy()
    nyq[:, n // 2] += 1j * np.float32(1e-5) * np.abs(nyq[:, n // 2])
    out["nyquist-imag"] = nyq
    return out


@pytest.mark.parametrize("n", LENGTHS)
def test_float32_reference_passes(n):
    assert M.edge_lengths(n) == tuple(sorted({1, 2, 3, n // 2 - 1, n // 2, n // 2 + 1, n - 1, n}))
    for T in M.edge_lengths(n):
        x = M.cases(n, T)
        c = M.check(M.rfft32(x, n), x, n, f"scipy float32, T {T}", margin=1.0)      # C_ref is its own maximum
        assert c <= M.c_ref(n)
    assert 0.5 <= M.c_ref(n) <= 8.0, M.c_ref(n)          # a float32 FFT sits near the model, not orders off it
    assert M.tolerance(n) == M.MARGIN * max(M.c_ref(n), 1.0)


def test_case_set():
    x = M.cases(1024, 1001)
    assert x.shape == (M.N_CASES, 1001) and x.dtype == np.float32
    assert np.array_equal(x, M.cases(1024, 1001))                                   # fixed by the seed
    rms = np.sqrt((x.astype(np.float64) ** 2).mean(-1))
    assert rms[M.ROW_LOUD] > 5e2 and rms[M.ROW_QUIET] < 2e-6 and rms[M.ROW_MEAN1E4] > 9e3
    assert (x[M.ROW_ZERO] == 0).all() and (x[3] == x[3, 0]).all()
    assert [int(np.flatnonzero(x[r])[0]) for r in range(7, 11)] == [0, 333, 500, 1000]
    assert (np.abs(M.rfft64(x[7:11], 1024)).round(12) == 1).all()                   # impulses: every bin has magnitude 1
    X = np.abs(M.rfft64(M.cases(1024, 1024)[11:15], 1024))
    assert X.argmax(-1).tolist() == [1, 256, 511, 512]
    assert M.take(x, 5).shape == (5, 1001) and np.array_equal(M.take(x, 37)[16], x[M.ROW_LOUD])


def test_zero_rows_must_be_exact():
    x = np.zeros((2, 40), dtype=np.float32)
    got = np.zeros((2, 33), dtype=np.complex64)
    assert M.bin_error(got, x, 64).max() == 0
    got[1, 7] = 1e-30
    assert np.isinf(M.bin_error(got, x, 64)[1, 7])
    with pytest.raises(AssertionError):
        M.check(got, x, 64)
    got[1, 7] = np.nan
    assert np.isinf(M.bin_error(got, x, 64)[1, 7])


@pytest.mark.parametrize("n", [32, 128, 256])
def test_rfft64_agrees_with_the_long_double_dft(n):
    """Measured: at most 8.5e-17 of ||x||_2 sqrt(n) over the case set (float64 round-off of a few passes); asserted with a
    tenfold margin."""
    for T in M.edge_lengths(n):
        x = M.cases(n, T)
        X, D = M.rfft64(x, n), M.dft_longdouble(x, n)
        scale = np.sqrt((x.astype(np.float64) ** 2).sum(-1, keepdims=True)) * np.sqrt(n)
        rel = np.abs(X - D) / np.where(scale > 0, scale, 1.0)
        assert (np.abs(D[M.ROW_ZERO]) == 0).all()
        assert float(rel.max()) <= 1e-15, (T, float(rel.max()))


@pytest.mark.parametrize("n", LENGTHS)
def test_every_mutant_is_rejected(n):
    for T in (n // 2 + 1, n - 1, n):
        x = M.cases(n, T)
        muts = mutants(x, n)
        assert ("mask+1" in muts) == (T < n)
        for name, Y in muts.items():
            c = M.bin_error(Y, x, n).max(-1)
            assert c.max() > M.tolerance(n), f"n {n} T {T}: {name} passes (c {c.max():.2f} <= {M.tolerance(n):.2f})"
            with pytest.raises(AssertionError):
                M.check(Y, x, n, name)
            # ... and on the rows where a single wrong bin cannot hide: the impulses (all bins 1) or the tones
            assert c[7:15].max() > M.tolerance(n), f"n {n} T {T}: {name} passes on the impulse and tone rows"


def test_margin_has_room():
    """The mutants are still rejected with the margin at LARGEST_MARGIN, eight times the one in use, and no longer at twice
    that: the bound is neither at the edge of what it must reject nor vacuous."""
    assert M.MARGIN == 4.0 and M.MARGIN < LARGEST_MARGIN
    worst = np.inf
    for n in LENGTHS:
        for T in (n // 2 + 1, n - 1, n):
            x = M.cases(n, T)
            for name, Y in mutants(x, n).items():
                worst = min(worst, M.bin_error(Y, x, n).max() / max(M.c_ref(n), 1.0))
    print(f"largest margin at which every mutant is rejected: {worst:.2f}")
    assert LARGEST_MARGIN <= worst < 2 * LARGEST_MARGIN, worst


def test_the_old_form_lets_a_zeroed_bin_through():
    """The gap: one bin of a real MFCC trajectory's spectrum (c1 configuration, `am` clip, 10 s: T 1001, n_mod 1024) stored
    as zero.  The former assertion -- 1e-4 of the maximum over all thirteen rows, which is c0's DC bin -- accepts it on most
    bins of c1 .. c12; the per-bin bound rejects every one of them."""
    kw, _, _ = load_golden("c1_am")
    m = O.mfcc(O.synth_clip(11, 160000, 16000, "am"), O.OracleConfig(**kw)).astype(np.float32)
    assert m.shape == (13, 1001)
    want = M.rfft64(m, 1024)
    ref = M.rfft32(m, 1024)
    M.check(ref, m, 1024, "float32 transform of the am trajectory")
    old_tol = 1e-4 * np.abs(want).max()
    passed_old = 0
    for row in range(1, 13):
        for k in range(1, 513):
            if abs(want[row, k]) <= old_tol:
                passed_old += 1
    assert passed_old >= 12 * 512 // 200, passed_old                 # (the issue measured 1 % of the bins)
    # the median bin of c1 .. c12 within a factor ten of the old tolerance: a 10 % error there passes the old form
    assert np.median(np.abs(want[1:, 1:])) <= 10 * old_tol
    row, k = np.unravel_index(np.abs(np.where(np.abs(want) <= old_tol, want, 0)).argmax(), want.shape)
    mutant = ref.copy()
    mutant[row, k] = 0
    assert np.abs(mutant - want).max() <= 1e-4 * np.abs(want).max()      # the old modspec assertion: passes
    with pytest.raises(AssertionError):
        M.check(mutant, m, 1024, "zeroed bin")                           # the per-bin bound: rejected
    c = M.bin_error(mutant, m, 1024)
    assert c[row, k] > 1e3 * M.tolerance(1024)
