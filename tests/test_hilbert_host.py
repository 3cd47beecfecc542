"""Host only: the per-sample bound of the Hilbert envelope (hilbert_oracle) means something.  The reference agrees with a
direct long-double DFT and with the rows whose envelope is known in closed form; scipy's same-precision envelope and the host
restatements of the chirp identity and of the pairing define C_ref and sit near the model; the length lists of the GPU tests
reach every kernel instantiation any smooth length up to 200 000 (and any chirp transform of 2^5 .. 2^19 points) reaches; and
subtly wrong transforms -- a long float32 twiddle chain, a doubled Nyquist bin, a doubled bin above n / 2, a pair without its
per-clip scaling, a float32 chirp in the float64 path -- are rejected, most of them where  2e-5 x the batch maximum  (1e-11
for float64) lets them through."""
import numpy as np
import pytest

import hilbert_oracle as H

F32, F64 = np.dtype(np.float32), np.dtype(np.float64)
DTYPES = (F32, F64)


# ---- the reference ----

@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 7, 8, 9, 11, 13, 16, 17, 30, 31, 64, 97, 105, 128])
def test_reference_agrees_with_the_long_double_dft(n):
    """Small smooth and small prime lengths (the latter through pocketfft's own chirp transform).  Asserted:
    8 sqrt(n) eps of the REFERENCE's precision, relative to the row's largest envelope value -- the direct sums add n rounded
    terms twice (a random walk of sqrt(n) eps each), the fast transform a few roundings per level; at most 2^-22 of the eps
    of the clips' precision here, so the reference's own error is no part of any c."""
    assert np.finfo(H.LD).eps < 1e-18
    k = 8 * max(np.sqrt(n), 2.0)
    for dt, tol in ((F32, k * np.finfo(np.float64).eps), (F64, k * float(np.finfo(H.LD).eps))):
        x = H.rows_for(n, dt)
        want, slow = H.envelope_hi(x), H.envelope_dft(x)
        assert want.dtype == (np.float64 if dt == F32 else H.LD)
        scale = np.maximum(slow.max(-1, keepdims=True), np.finfo(np.float32).tiny)
        assert (want[H.ROW_ZERO] == 0).all() and (slow[H.ROW_ZERO] == 0).all()
        assert float((np.abs(want - slow) / scale).max()) <= tol, (n, dt, float((np.abs(want - slow) / scale).max()))


@pytest.mark.parametrize("n", [2, 3, 4, 7, 16, 35, 96, 625, 1000, 4097])
def test_rows_with_a_known_envelope(n):
    t = np.arange(n)
    rows, want = [np.full(n, -37.25)], [37.25]
    if n % 2 == 0:
        rows.append(2.5 * (-1.0) ** t)
        want.append(2.5)
    for k in sorted({1, n // 4, (n - 1) // 2} - {0}):
        if 0 < 2 * k < n:
            rows.append(3.0 * np.cos(2 * np.pi * ((k * t) % n) / n + 0.3))
            want.append(3.0)
    env = H.envelope_hi(np.stack(rows))
    assert env.dtype == H.LD
    assert float(np.abs(env / np.array(want)[:, None] - 1).max()) <= 1e-14      # (the rows are cosines rounded to float64)


def test_mask_and_case_rows():
    assert H.spectrum_mask(1).tolist() == [1] and H.spectrum_mask(2).tolist() == [1, 1]
    assert H.spectrum_mask(5).tolist() == [1, 2, 2, 0, 0] and H.spectrum_mask(6).tolist() == [1, 2, 2, 1, 0, 0]
    for n in (1, 2, 3, 4, 35, 1001):
        x32, x64 = H.rows_for(n, F32), H.rows_for(n, F64)
        assert x32.shape == (18, n) and x64.shape == (16, n) and np.array_equal(x32, H.rows_for(n, F32))
        assert not x32[H.ROW_ZERO].any() and (x32[3] == 37.25).all()
        assert np.abs(x32[H.ROW_1E30]).max() > 1e29 and 0 < np.abs(x32[H.ROW_1EM30]).max() < 1e-29
        assert np.abs(x32[H.ROW_LOUD]).max() > 1e2 and np.abs(x32[H.ROW_QUIET]).max() < 1e-5
    x, idx = H.take(H.rows_for(64, F32), 5)
    assert idx.tolist() == [H.ROW_LOUD, H.ROW_QUIET, H.ROW_MEAN1E4, 7, 8]
    assert (H.take(H.rows_for(64, F32), 37)[1][::2] % 2 == 0).all()            # take() keeps row r beside row r ^ 1


def test_sigma_and_the_rules_for_zero_and_non_finite_rows():
    x = H.rows_for(64, F32)[[H.ROW_LOUD, H.ROW_QUIET, H.ROW_ZERO, 0, 1]].copy()
    s1, s2 = H.sigma(x, False), H.sigma(x, True)
    rms = np.sqrt((x.astype(np.float64) ** 2).mean(-1))
    assert np.allclose(s1, rms)
    assert s2[2] == 0 and np.isclose(s2[3], rms[3]) and np.isclose(s2[4], rms[4])      # a zero partner, no partner
    down, up, kind = H.pair_scale(x)
    assert kind.tolist() == [0, 0, 1, 0, 0] and up[2] == 0 and (down[[0, 1]] * up[[0, 1]] == 1).all()
    assert (0.5 <= np.abs(x[:2]).max(-1) * down[:2]).all() and (np.abs(x[:2]).max(-1) * down[:2] < 1).all()
    # the quiet row beside the loud one: held to ITS scale times the pair's norm, which is of order one for both
    assert s2[1] < 1e-5 and s2[1] > rms[1] and s2[0] > rms[0]
    # the stored value of a pair: the partner's envelope at the row's own scale on top of the row's; none without a partner
    want = H.envelope_hi(x)
    st = H.stored(x, want, True)
    assert np.array_equal(H.stored(x, want, False), want)
    assert np.allclose(st[1], want[1] + up[1] * down[0] * want[0]) and np.allclose(st[0], want[0] + up[0] * down[1] * want[1])
    assert np.array_equal(st[3], want[3]) and np.array_equal(st[4], want[4]) and (st[1] < 1e-4).all()
    bad = x.copy()
    bad[0, 3] = np.inf
    assert np.isnan(H.sigma(bad, True)[0]) and np.isclose(H.sigma(bad, True)[1], rms[1])
    # check(): zero rows exact, non-finite rows NaN throughout
    ref = H.reference(64, F32)
    rows, idx = H.take(ref.rows, 12)                       # case rows 4 .. 15
    an = H.host_analytic(64, F32)
    good = H.paired_envelope(rows, an)
    H.check(good, rows, idx, 64, F32, True, "host restatement")
    z = int(np.flatnonzero(idx == H.ROW_ZERO)[0])
    worse = good.copy()
    worse[z, 5] = 1e-30
    with pytest.raises(AssertionError):
        H.check(worse, rows, idx, 64, F32, True)
    rows2, idx2 = rows.copy(), idx.copy()
    rows2[0, 7], idx2[0] = np.nan, -1
    good2 = H.paired_envelope(rows2, an)
    assert np.isnan(good2[0]).all() and np.isfinite(good2[1:]).all()
    H.check(good2, rows2, idx2, 64, F32, True, "a NaN row beside a finite one")
    good2[0, 9] = 1.0
    with pytest.raises(AssertionError):
        H.check(good2, rows2, idx2, 64, F32, True)


# ---- C_ref ----

C_REF_LENGTHS = (16, 35, 256, 625, 4096, 30240, 144000, 160000, 511, 8193, 131073)


@pytest.mark.parametrize("n", C_REF_LENGTHS)
def test_host_envelopes_define_c_ref(n):
    """scipy's same-precision envelope, the chirp restatement and the paired restatement are within max(C_ref, 1) of themselves
    by construction; what is asserted is that they sit near the model (dense rows below 2, every row below 100) -- the
    per-row table is printed (-s) and kept in docs/experiments.md."""
    for dt in DTYPES:
        ref = H.reference(n, dt)
        for form in ("single", "paired"):
            c = ref.c_ref(form)
            print(f"hilbert-C_ref n={n} {'chirp M=%d' % ref.plan['M'] if ref.plan['bluestein'] else 'direct'} {dt.name} {form}: "
                  + " ".join(f"{v:.2f}" for v in c))
            dense = c[[0, 1, 2, 4, 5, 6]]
            assert np.isfinite(dense).all() and dense.max() <= 2.0, (n, dt, form, dense)
            assert c[H.ROW_ZERO] == 0
            fin = c[np.isfinite(c)]
            assert fin.size >= c.size - 1 and fin.max() <= 100.0, (n, dt, form, c)
            if not np.isfinite(c).all():       # the unnormalised chirp transforms of the 1e30 row overflow float32 on their own
                assert form == "single" and dt == F32 and ref.plan["bluestein"] and not np.isfinite(c[H.ROW_1E30])
    # the host restatement of a call passes check() with margin 1
    ref = H.reference(n, F32)
    x, idx = H.take(ref.rows, 5)
    H.check(H.paired_envelope(x, H.host_analytic(n, F32)), x, idx, n, F32, True, "restatement", margin=1.0)


def test_ragged_restatement():
    x = H.rows_for(100, F64)[0]
    for M in (256, 1024):
        fft = H.scipy_fft(np.complex128)
        a = H.bluestein_analytic(x[None].astype(np.complex128), fft, M, bhat_in_precision=True)
        want = H.envelope_hi(x[None])
        assert float(np.abs(np.abs(a) - want).max()) < 1e-12
        H.check_clip(np.abs(a)[0], x, M, margin=1.0)


# ---- coverage ----

def _reach(lengths, call, rows=(1, 2), dtypes=DTYPES):
    out = set()
    for n in lengths:
        for r in rows:
            for dt in dtypes:
                out |= H.features(n, r, call, dt)
    return out


def test_plan_rule():
    assert H.passes(160000) == {"bluestein": False, "M": 160000, "radix": [256, 625]}
    assert H.passes(441000)["radix"] == [8, 9, 25, 5, 49]
    assert H.passes(144000)["radix"] == [16, 8, 9, 25, 5]
    assert H.passes(1) == {"bluestein": False, "M": 1, "radix": []}
    assert H.passes(11) == {"bluestein": True, "M": 32, "radix": [16, 2]}
    assert H.passes(160001)["M"] == 1 << 19 and H.passes(160001)["radix"] == [256, 256, 8]
    assert H.passes(8, ragged=True) == {"bluestein": True, "M": 16, "radix": [16]}
    assert [H.chirp_fft_size(n) for n in (1, 8, 9, 16, 17, 2049)] == [16, 16, 32, 32, 64, 8192]
    f = H.features(256, 1, "envelope", F32)
    assert f == {("mid2", 256, "Ns1", "partial", "real", "envelope", "single", "float32", "dense")}
    f = H.features(4096, 2, "envelope", F64)
    assert f == {("pass2", 256, "Ns1", "full", "real", "complex", "paired", "float64", "dense"),
                 ("mid", 16, "twiddled", "full", "complex", "complex", "-", "float64", "dense"),
                 ("pass2", 256, "strided", "full", "complex", "envelope", "paired", "float64", "dense")}
    assert len(H.smooth_lengths()) == 842 and H.smooth_lengths()[:8] == [1, 2, 3, 4, 5, 6, 7, 8]


def test_gpu_lengths_reach_every_feature():
    """Coverage is a condition: the envelope lists with row counts 1 and 2-or-more and both dtypes, the forward list, the chirp
    lengths and the ragged transform lengths reach every kernel instantiation -- kernel, radix, position, partial or full
    last workgroup, in- and out-mode, pairing, dtype -- that ANY length in range reaches."""
    smooth = H.smooth_lengths()
    assert max(H.ENVELOPE_LENGTHS + H.FORWARD_LENGTHS + H.BLUESTEIN_LENGTHS) <= H.LIMIT
    universe = _reach(smooth, "envelope")
    got = _reach(H.ENVELOPE_LENGTHS, "envelope")
    assert not universe - got, sorted(universe - got)[:5]
    assert {1 if r == 1 else 2 for r in H.ENVELOPE_ROWS} == {1, 2}
    print(f"envelope: {len(universe)} features of {len(smooth)} smooth lengths reached by {len(H.ENVELOPE_LENGTHS)} lengths")
    even = [n for n in smooth if n % 2 == 0]
    universe = _reach(even, "rfft", rows=(1,), dtypes=(F32,))
    got = _reach(H.FORWARD_LENGTHS, "rfft", rows=(1,), dtypes=(F32,))
    assert not universe - got, sorted(universe - got)[:5]
    print(f"forward: {len(universe)} features of {len(even)} even smooth lengths reached by {len(H.FORWARD_LENGTHS)} lengths")
    # every chirp transform length 2^5 .. 2^19: the features depend on M alone
    assert [H.passes(n)["M"] for n in H.BLUESTEIN_LENGTHS] == [1 << p for p in range(5, 20)]
    assert all(H.passes(n)["bluestein"] for n in H.BLUESTEIN_LENGTHS + H.LONG_CASES[1:])
    assert H.passes(H.LONG_CASES[1])["M"] == 1 << 19 and H.LONG_CASES[1] not in H.BLUESTEIN_LENGTHS
    # alternately the smallest length above M / 4 and the largest with 2 n - 1 <= M that is not smooth
    assert H.BLUESTEIN_LENGTHS[:4] == (11, 31, 33, 127) and H.BLUESTEIN_LENGTHS[-2:] == (131071, 131073)
    assert [H.bluestein_length(32, True), H.bluestein_length(32, False)] == [11, 13]
    universe = _reach([H.bluestein_length(1 << p, True) for p in range(5, 20)], "envelope")
    assert not universe - _reach(H.BLUESTEIN_LENGTHS, "envelope")
    universe = _reach([(1 << p) // 2 for p in range(4, 20)], "ragged", rows=(3,))
    got = _reach([M // 2 for M in H.RAGGED_M], "ragged", rows=(3,))
    assert not universe - got, sorted(universe - got)[:5]
    assert {1 << p for p in (4, 5, 8, 12, 13, 17)} <= set(H.RAGGED_M)


def greedy_cover(candidates, reach):
    """The list the oracle holds: repeatedly the length that reaches most features not yet reached (ties: the shortest)."""
    sets = {n: reach(n) for n in candidates}
    need = set().union(*sets.values())
    chosen = []
    while need:
        best = max(candidates, key=lambda n: (len(sets[n] & need), -n))
        chosen.append(best)
        need -= sets[best]
    return tuple(sorted(chosen))


def test_the_lists_are_the_greedy_covers():
    smooth = H.smooth_lengths()
    assert greedy_cover(smooth, lambda n: _reach([n], "envelope")) == H.ENVELOPE_LENGTHS
    assert greedy_cover([n for n in smooth if n % 2 == 0], lambda n: H.features(n, 1, "rfft")) == H.FORWARD_LENGTHS


# ---- the yardstick bites ----

def _twiddles(Ns, ctype, chain):
    """W_(2 Ns)^k, k < Ns: float64 values rounded once, or (chain > 1) exact at every chain-th k and a running product in
    ctype between."""
    k = np.arange(Ns)
    w = np.exp(-1j * np.pi * k / Ns).astype(ctype)
    if chain > 1 and Ns > 1:
        w1 = w[1]
        for s in range(1, min(chain, Ns)):
            w[s::chain] = (w[s - 1::chain][:len(w[s::chain])] * w1).astype(ctype)
    return w


def stockham_fft(chain=0):
    """A small radix-2 Stockham autosort transform of power-of-two rows in the rows' own precision (numpy keeps complex64)."""
    def fft(z):
        ct = z.dtype
        M = z.shape[-1]
        assert M & (M - 1) == 0
        x = z.reshape(-1, M).copy()
        Ns, half = 1, M // 2
        j = np.arange(half)
        while Ns < M:
            k = j % Ns
            v0, v1 = x[:, :half], x[:, half:] * _twiddles(Ns, ct, chain)[k]
            out = np.empty_like(x)
            base = (j - k) * 2 + k
            out[:, base], out[:, base + Ns] = v0 + v1, v0 - v1
            x, Ns = out, 2 * Ns
        assert x.dtype == ct
        return x.reshape(z.shape)
    return fft


def _rows_beyond(env, x, idx, n, dt, paired):
    """Case rows of the call whose c exceeds the bound."""
    ref = H.reference(n, dt)
    c = H.errors(env, ref.want[idx], H.sigma(x, paired), n, dt, H.stored(x, ref.want[idx], paired)).max(-1)
    tol = H.bound(ref.c_ref("paired" if paired else "single")[idx])
    return idx[c > tol].tolist(), float((c / tol).max())


def _old_form_accepts(env, want, dt):
    tol = 2e-5 if dt == F32 else 1e-11
    return bool(np.abs(env.astype(want.dtype) - want).max() <= tol * want.max())


def test_the_stockham_restatement_passes_and_its_mutants_do_not():
    results = {}
    n = 4096
    ref = H.reference(n, F32)
    x16, i16 = ref.rows[:16], np.arange(16)                    # (without the 1e30 rows: the old form's batch maximum)
    direct = lambda fft, mask=None: (lambda z: H.direct_analytic(z, fft, mask))      # noqa: E731
    # the unmutated transform: one clip and two clips per transform
    good = stockham_fft()
    for paired, env in ((False, H.single_envelope(x16, direct(good))), (True, H.paired_envelope(x16, direct(good)))):
        bad, worst = _rows_beyond(env, x16, i16, n, F32, paired)
        assert not bad, (paired, bad, worst)
        assert _old_form_accepts(env, ref.want[:16], F32)
        results["stockham, exact twiddles, " + ("paired" if paired else "single")] = worst
    # 1: a float32 twiddle chain of 64 steps
    env = H.single_envelope(x16, direct(stockham_fft(chain=64)))
    bad, worst = _rows_beyond(env, x16, i16, n, F32, False)
    assert bad and H.ROW_LOUD in bad, (bad, worst)
    assert _old_form_accepts(env, ref.want[:16], F32)
    results["twiddle chain of 64 steps"] = worst
    # 2: weight 2 at the Nyquist bin -- on the trajectory rows, where the old form accepts it
    nyq = H.spectrum_mask(n)
    nyq[n // 2] = 2.0
    tr = np.array([0, 1, 2, H.ROW_MEAN1E4])
    env = H.single_envelope(ref.rows[tr], direct(good, nyq))
    bad, worst = _rows_beyond(env, ref.rows[tr], tr, n, F32, False)
    assert bad, worst
    assert _old_form_accepts(env, ref.want[tr], F32)
    results["weight 2 at the Nyquist bin"] = worst
    # 3: weight 2 at the first bin above n / 2 of an odd length (the chirp identity over the same Stockham transform)
    n_odd = 4095
    ref_o = H.reference(n_odd, F32)
    M = H.passes(n_odd)["M"]
    assert H.passes(n_odd)["bluestein"] and M == 8192
    up = H.spectrum_mask(n_odd)
    assert up[(n_odd + 1) // 2] == 0 and up[(n_odd - 1) // 2] == 2
    up[(n_odd + 1) // 2] = 2.0
    env = H.single_envelope(ref_o.rows[tr], lambda z: H.bluestein_analytic(z, good, M))
    assert not _rows_beyond(env, ref_o.rows[tr], tr, n_odd, F32, False)[0]
    env = H.single_envelope(ref_o.rows[tr], lambda z: H.bluestein_analytic(z, good, M, mask=up))
    bad, worst = _rows_beyond(env, ref_o.rows[tr], tr, n_odd, F32, False)
    assert bad, worst
    assert _old_form_accepts(env, ref_o.want[tr], F32)
    results["weight 2 above n / 2, odd n"] = worst
    # 4: two clips per transform without the per-clip scaling, the 1e-6 row beside the 1e3 row
    pr = np.array([H.ROW_LOUD, H.ROW_QUIET, H.ROW_MEAN1E4, 7])
    env = H.paired_envelope(ref.rows[pr], direct(good), scaled=False)
    bad, worst = _rows_beyond(env, ref.rows[pr], pr, n, F32, True)
    assert H.ROW_QUIET in bad, (bad, worst)
    assert _old_form_accepts(env, ref.want[pr], F32)
    results["pair without per-clip scaling"] = worst
    # 5: a float64 path whose chirp is rounded to float32
    ref_d = H.reference(n_odd, F64)
    i64 = np.arange(16)
    env = H.single_envelope(ref_d.rows, lambda z: H.bluestein_analytic(z, good, M))
    assert not _rows_beyond(env, ref_d.rows, i64, n_odd, F64, False)[0]
    env = H.single_envelope(ref_d.rows, lambda z: H.bluestein_analytic(z, good, M, chirp_dtype=np.complex64))
    bad, worst = _rows_beyond(env, ref_d.rows, i64, n_odd, F64, False)
    assert len(bad) >= 12, (bad, worst)
    assert not _old_form_accepts(env, ref_d.want, F64) or worst > 1e3      # (this one the old float64 form may catch as well)
    results["float64 path, float32 chirp"] = worst
    for name, worst in results.items():
        print(f"hilbert-mutant {name}: largest c / bound = {worst:.2f}")
