"""GPU (-m gpu): the Lomb-Scargle modulation spectrum (modulation_lombscargle_batch / _ragged_batch, mm_lombscargle_f64)
against the yardstick of tests/lomb_oracle.py: scipy on the valid samples, c = max|got - want| / max|want| within
max(1e-12, 16 x scipy's own rounding), never above 1e-10.  Shapes are the smallest that reach every boundary of the kernel:
the 16-row and 16-frequency MFMA tile, the row tiles a workgroup carries, the sample chunk S = lomb.LOMB_CHUNK (one chunk:
the main kernel runs the epilogue; more: the finish kernel does)."""
import ctypes as C

import numpy as np
import pytest

import lomb_oracle as O
import stream_cases as S
import test_gpu_streams as TS

pytestmark = pytest.mark.gpu

FS = O.FS


def _chunk():
    from modulation_mfcc_amd import lomb
    return lomb.LOMB_CHUNK


def dev(a, gpu):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(gpu)


def run(x, f, gpu, combo=O.COMBOS[0], lengths=None, t=None, fs=FS):
    """-> numpy [rows, F]; x numpy [rows, n] or a device tensor."""
    from modulation_mfcc_amd import modulation_lombscargle_batch, modulation_lombscargle_ragged_batch
    xd = x if not isinstance(x, np.ndarray) else dev(x, gpu)
    kw = dict(t=t, **O._kw(combo))
    if lengths is None:
        return modulation_lombscargle_batch(xd, fs, f, **kw).cpu().numpy()
    return modulation_lombscargle_ragged_batch(xd, lengths, fs, f, **kw).cpu().numpy()


def gapped_rows(rows, n, key, least=37):
    """f0-like rows with NaN stretches, every row with at least `least` valid samples where n allows."""
    r = O._rng("rows", rows, n, key)
    x = np.stack([O.f0_curve(n, (key, b)) for b in range(rows)])
    for b in range(rows):
        for _ in range(3):
            a = int(r.integers(0, max(n - 1, 1)))
            x[b, a:a + int(r.integers(1, max(n // 8, 2)))] = np.nan
        if (~np.isnan(x[b])).sum() < min(least, n):
            x[b] = O.f0_curve(n, (key, b, "again"))
    return x


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else np.ascontiguousarray(a).view(np.float64).view(np.uint64)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


# ---- accuracy: every fixture x floating_mean x precenter x normalisation ----------------------------------------------------------
@pytest.mark.parametrize("combo", O.COMBOS, ids=O.combo_id)
@pytest.mark.parametrize("name", O.NAMES)
def test_every_fixture_against_the_yardstick(name, combo, gpu):
    t, x, f = O.fixture(name)
    got = run(x[None, :], f, gpu, combo)
    assert got.dtype == (np.complex128 if combo[2] == "amplitude" else np.float64)
    O.check(got[0], name, combo)


# ---- shapes: the tile and chunk boundaries ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", (1, 15, 16, 17, 33))
def test_row_counts(rows, gpu):
    n = 160
    x = gapped_rows(rows, n, "rc")
    f = O.grid(n, count=17)
    for combo in (O.COMBOS[0], (True, True, "amplitude")):
        got = run(x, f, gpu, combo)
        for b in range(rows):
            O.check_row(got[b], O.time_axis(n), x[b], f, combo, what=f"rows {rows}, row {b}")


@pytest.mark.parametrize("nf", (1, 15, 16, 17, 65))
def test_frequency_counts(nf, gpu):
    n = 200
    x = gapped_rows(3, n, "fc")
    f = O.grid(n, count=nf) if nf > 1 else np.array([3.7])
    for combo in (O.COMBOS[0], (True, False, "normalize")):
        got = run(x, f, gpu, combo)
        assert got.shape == (3, nf)
        for b in range(3):
            O.check_row(got[b], O.time_axis(n), x[b], f, combo, what=f"{nf} frequencies, row {b}")


def _n_max_cases():
    s = _chunk()
    return (s - 1, s, s + 1, 2 * s + 3)


@pytest.mark.parametrize("which", range(4), ids=("S-1", "S", "S+1", "2S+3"))
@pytest.mark.parametrize("combo", (O.COMBOS[0], (True, True, "normalize"), (True, False, "amplitude")), ids=O.combo_id)
def test_one_two_and_three_chunks(which, combo, gpu):
    n = _n_max_cases()[which]
    x = gapped_rows(3, n, "chunks")
    f = O.grid(n, count=20)
    got = run(x, f, gpu, combo)
    for b in range(3):
        O.check_row(got[b], O.time_axis(n), x[b], f, combo, what=f"n_max {n}, row {b}")


@pytest.mark.parametrize("n", (4, 5))
def test_rows_of_four_and_five_samples(n, gpu):
    """Too few samples for the accuracy grid's ceiling with the floating mean: without it against the bound."""
    x = np.array([[1.0, 2.5, -0.5, 3.0, 0.25][:n], [0.5, -1.0, 2.0, 1.5, -2.0][:n]])
    f = np.array([9.0, 17.0, 31.0])
    for combo in [c for c in O.COMBOS if not c[0]]:
        got = run(x, f, gpu, combo)
        for b in range(2):
            O.check_row(got[b], O.time_axis(n), x[b], f, combo, what=f"n_max {n}, row {b}")


def test_one_sample(gpu):
    """n_max = 1: scipy's own numbers for a single data point (CC = 1, SS clamps)."""
    x = np.array([[2.0], [-3.5]])
    f = np.array([0.0, 7.0])
    got = run(x, f, gpu, O.COMBOS[0])
    for b in range(2):
        O.check_row(got[b], O.time_axis(1), x[b], f, O.COMBOS[0], what=f"one sample, row {b}")


THREE = np.array([[1.0, np.nan, 2.5, -0.5, np.nan], [0.5, -1.0, 2.0, np.nan, np.nan], [np.nan, 4.0, 1.0, np.nan, 3.0]])


@pytest.mark.parametrize("combo", O.COMBOS, ids=O.combo_id)
@pytest.mark.parametrize("n", (3, 5))
def test_three_sample_rows(n, combo, gpu):
    """Rows of three valid samples (n_max 3: no NaN; n_max 5: two NaN each).  Without the floating mean against the bound;
    with it scipy's own spread leaves the ceiling (1e-8): finite where scipy is finite and within 16 x spread, the ceiling
    lifted for this case alone."""
    x = THREE[:, :n] if n == 5 else np.array([[1.0, 2.5, -0.5], [0.5, -1.0, 2.0], [4.0, 1.0, 3.0]])
    f = np.array([9.0, 17.0, 31.0])
    got = run(x, f, gpu, combo)
    for b in range(3):
        want = O.recipe(O.time_axis(n), x[b], f, **O._kw(combo))
        assert np.isfinite(got[b][np.isfinite(want)]).all()
        O.check_row(got[b], O.time_axis(n), x[b], f, combo, what=f"three samples, n_max {n}, row {b}", lift_ceiling=combo[0])


@pytest.mark.parametrize("combo", O.COMBOS, ids=O.combo_id)
def test_frequency_zero(combo, gpu):
    """f = 0 beside two ordinary frequencies.  Without the floating mean against the bound; with it (CC - C C = 0 clamps)
    finite where scipy is finite and within 16 x spread, the ceiling lifted for this case alone."""
    t, x, _ = O.fixture("f0-gaps")
    f = np.array([0.0, 4.0, 11.0])
    got = run(x[None, :], f, gpu, combo)[0]
    want = O.recipe(t, x, f, **O._kw(combo))
    assert np.isfinite(got[np.isfinite(want)]).all()
    O.check_row(got, t, x, f, combo, what="f = 0", lift_ceiling=combo[0])


# ---- masks -------------------------------------------------------------------------------------------------------------------
def test_masks(gpu):
    s = _chunk()
    n = 2 * s + 40
    f = O.grid(n, count=18)
    x = np.stack([O.f0_curve(n, ("mask", b)) for b in range(5)])
    x[0, 0] = x[0, -1] = np.nan                              # NaN at the first and the last sample
    x[1, s:2 * s] = np.nan                                   # a whole chunk of NaN in the middle
    x[2, :] = np.nan                                         # a row of NaN only
    x[3, :] = np.nan
    x[3, 0] = 123.0                                          # one valid sample: at t = 0 (sin = 0, SS clamps) against scipy;
    x = np.concatenate([x, np.full((1, n), np.nan)])         # in the second chunk scipy's own SS is rounding noise (its spread
    x[5, s + 7] = 123.0                                      # is 1e-10): finite, and the bits of the row alone
    t = O.time_axis(n)
    for combo in (O.COMBOS[0], (False, True, "normalize"), (False, False, "amplitude")):
        got = run(x, f, gpu, combo)
        assert np.isnan(got[2]).all(), "a row without a valid sample is NaN in every output"
        for b in (0, 1, 4):
            O.check_row(got[b], t, x[b], f, combo, what=f"mask row {b}")
        if not combo[1] and combo[2] != "amplitude":         # (precentred, one sample is a row of zeros: 0 / 0 in scipy too;
                                                             # its 'amplitude' is rounding noise / rounding noise: b = YS / SS)
            O.check_row(got[3], t, x[3], f, combo, what="one valid sample")
        alone = run(x[[0, 1, 4, 5]], f, gpu, combo)
        assert same_bits(alone, got[[0, 1, 4, 5]]), "the neighbours of a NaN row are untouched"
        if combo == O.COMBOS[0]:
            assert np.isfinite(got[5]).all() and (got[5] >= 0).all()


def test_an_inf_poisons_its_own_row_only(gpu):
    n = 300
    x = gapped_rows(4, n, "inf")
    f = O.grid(n, count=16)
    clean = run(x, f, gpu)
    y = x.copy()
    y[1, 17] = np.inf
    got = run(y, f, gpu)
    assert not np.isfinite(got[1]).any()
    assert same_bits(got[[0, 2, 3]], clean[[0, 2, 3]])


# ---- bit for bit ---------------------------------------------------------------------------------------------------------------
BIT_COMBOS = (O.COMBOS[0], (True, True, "normalize"), (True, False, "amplitude"))


@pytest.mark.parametrize("n", (200, 1100), ids=("one-chunk", "three-chunks"))
def test_a_row_alone_among_33_and_permuted(n, gpu):
    x = gapped_rows(33, n, "perm")
    f = O.grid(n, count=17)
    perm = O._rng("perm").permutation(33)
    for combo in BIT_COMBOS:
        got = run(x, f, gpu, combo)
        for b in (0, 15, 16, 32):
            assert same_bits(run(x[b:b + 1], f, gpu, combo)[0], got[b]), (combo, b)
        assert same_bits(run(x[perm], f, gpu, combo), got[perm]), combo


@pytest.mark.parametrize("n_max", (400, 1100), ids=("one-chunk", "three-chunks"))
def test_what_lies_behind_the_length_never_matters(n_max, gpu):
    import torch
    lens = np.array([n_max, 1, 37, n_max // 2, n_max - 1, 513 if n_max > 513 else 100], dtype=np.int64)
    rows = len(lens)
    x = gapped_rows(rows, n_max, "pad")
    x[:, 0] = 140.0 + np.arange(rows)                   # (every row has a valid sample in front of any length)
    f = O.grid(n_max, count=17)
    other = O.f0_curve(n_max, "other")
    for combo in BIT_COMBOS:
        outs = []
        for fill in (0.0, np.nan, np.inf, None):
            y = x.copy()
            for b, L in enumerate(lens):
                y[b, L:] = other[L:] if fill is None else fill
            outs.append(run(y, f, gpu, combo, lengths=lens))
        for o in outs[1:]:
            assert same_bits(o, outs[0]), combo
        # device lengths = host lengths
        assert same_bits(run(x, f, gpu, combo, lengths=torch.from_numpy(lens).to(gpu)), outs[0])
        # a ragged row of length L = the single-length call on x[:, :L], whatever the chunk plan of n_max
        # (a chunk behind the length adds +0.0)
        for b, L in enumerate(lens):
            if (~np.isnan(x[b, :L])).any():
                alone = run(x[b:b + 1, :L], f, gpu, combo, t=O.time_axis(n_max)[:L])
                assert same_bits(alone[0], outs[0][b]), (combo, b, L)


def test_device_lengths_are_clamped(gpu):
    import torch
    n = 100
    x = gapped_rows(3, n, "clamp")
    f = O.grid(n, count=5)
    got = run(x, f, gpu, lengths=torch.tensor([10 ** 12, 0, -5], dtype=torch.int64, device=gpu))
    want = run(x, f, gpu, lengths=np.array([n, 1, 1]))
    assert same_bits(got[:1], want[:1]) and same_bits(got[1:], want[1:])


def test_a_jittered_time_axis_against_scipy(gpu):
    n = 700
    r = O._rng("jitter")
    t = (np.arange(n) + r.uniform(-0.4, 0.4, size=n)) / FS
    x = gapped_rows(2, n, "jitter")
    f = O.grid(n, count=40)
    for combo in BIT_COMBOS:
        got = run(x, f, gpu, combo, t=t)
        for b in range(2):
            O.check_row(got[b], t, x[b], f, combo, what=f"jittered t, row {b}")
        assert same_bits(run(x, f, gpu, combo, t=dev(t, gpu)), got)


def test_float32_rows_are_widened(gpu):
    n = 300
    x = gapped_rows(2, n, "f32").astype(np.float32)
    f = O.grid(n, count=9)
    assert same_bits(run(x, f, gpu), run(x.astype(np.float64), f, gpu))


def test_row_pitch_and_list_front_end(gpu):
    import torch
    from modulation_mfcc_amd import modulation_lombscargle_batch, modulation_lombscargle_list
    n = 600
    x = gapped_rows(3, n, "pitch")
    f = O.grid(n, count=9)
    wide = torch.full((3, n + 13), float("nan"), dtype=torch.float64, device=gpu)
    wide[:, :n] = dev(x, gpu)
    want = run(x, f, gpu)
    assert same_bits(modulation_lombscargle_batch(wide[:, :n], FS, f).cpu().numpy(), want)
    lens = (n, 37, 513)
    outs = modulation_lombscargle_list([dev(x[b, :L], gpu) for b, L in enumerate(lens)], FS, f)
    for b, L in enumerate(lens):
        assert same_bits(outs[b].cpu().numpy(), run(x[b:b + 1, :L], f, gpu)[0])
    with pytest.raises(ValueError, match=r"equal non-zero length! \(curve 1\)"):
        modulation_lombscargle_list([dev(x[0], gpu), torch.full((5,), float("nan"), dtype=torch.float64, device=gpu)], FS, f)


def test_a_row_without_a_valid_sample_host_lengths_raise_device_lengths_nan(gpu):
    import torch
    from modulation_mfcc_amd import modulation_lombscargle_ragged_batch
    n = 80
    x = gapped_rows(3, n, "empty")
    x[1, :20] = np.nan
    f = O.grid(n, count=5)
    lens = np.array([n, 20, 50])
    with pytest.raises(ValueError, match=r"equal non-zero length! \(row 1 has 0 samples\)"):
        modulation_lombscargle_ragged_batch(dev(x, gpu), lens, FS, f)
    got = run(x, f, gpu, lengths=torch.from_numpy(lens).to(gpu))
    assert np.isnan(got[1]).all() and np.isfinite(got[[0, 2]]).all()


# ---- against the Welch unit ---------------------------------------------------------------------------------------------------
def test_power_agrees_with_the_boxcar_periodogram_on_bin_centres(gpu):
    """A gap-free row at the bin centres k fs / n: the least-squares sinusoid at a DFT frequency has the amplitude
    A = 2 |X_k| / n, and scipy's 'power' is A^2 K / 4 (its docstring), so 'power' x 4 / K = the squared amplitude =
    2 x modulation_psd_batch(boxcar, one segment, scaling='spectrum', no detrending) -- against numpy's float64 rfft to
    the yardstick's floor, against the float32 Welch unit to float32 (1e-5 of the largest: 2^-24 a butterfly stage, eight
    stages, squared).  (K, not K^2: pgram = 2 (a YC + b YS) with a = 2 YC, b = 2 YS and YC = sum y cos / K is already
    4 |X_k|^2 / K^2 = A^2.)"""
    from modulation_mfcc_amd import modulation_psd_batch
    n = 256
    x = np.stack([O.f0_curve(n, ("welch", b)) for b in range(2)]) - 150.0          # (float32 on the Welch side: no large mean)
    k = np.arange(1, n // 2)                          # (not 0 and not the Nyquist bin: one-sided doubling)
    f = k * FS / n
    got = run(x, f, gpu) * 4.0 / n
    amp2 = (2.0 * np.abs(np.fft.rfft(x, axis=1)) / n) ** 2
    for b in range(2):
        c = O.measure(got[b], amp2[b, k])
        print(f"lomb against |rfft|^2, row {b}: c = {c:.3e}")
        assert c <= O.FLOOR
    fw, p = modulation_psd_batch(dev(x.astype(np.float32), gpu), FS, window="boxcar", nperseg=n, noverlap=0, nfft=n,
                                 detrend=False, scaling="spectrum")
    p = p.cpu().numpy().astype(np.float64)
    assert np.allclose(np.asarray(fw.cpu() if hasattr(fw, "cpu") else fw)[k], f)
    assert np.abs(2.0 * p[:, k] - got).max() <= 1e-5 * amp2[:, k].max()


# ---- the stream contract of mm_lombscargle_f64 -----------------------------------------------------------------------------------
# The cases are built with the registry's Case class but are NOT appended to stream_cases.CASES (the registry is pinned to
# the entries of include/modmfcc.h); the three checks are those of test_gpu_streams.py, called with these cases.
S_ROWS, S_N, S_F = 5, 2 * 512 + 90, np.linspace(0.5, 40.0, 21)        # three chunks: the workspace and the finish kernel
SK = dict(precenter=True, normalize="amplitude", floating_mean=True)


def _curves(name):
    a, b = S.curve_sets(name, S_ROWS, S_N)
    for k, x in enumerate((a, b)):
        x[:, 100 + 50 * k:160 + 70 * k] = np.nan
        x[2, 512:1024] = np.nan
    return a, b


def _wrapper_case(ragged):
    name = "lomb/" + ("ragged-wrapper" if ragged else "wrapper")

    def data():
        d = {"x": _curves(name)}
        if ragged:
            d["lengths"] = S.length_sets(S_ROWS, S_N, 37)
        return d

    def setup(env):
        from modulation_mfcc_amd import modulation_lombscargle_batch, modulation_lombscargle_ragged_batch
        if ragged:
            return lambda: torch_real(modulation_lombscargle_ragged_batch(env.buf["x"], env.buf["lengths"], FS, S_F, **SK))
        return lambda: torch_real(modulation_lombscargle_batch(env.buf["x"], FS, S_F, **SK))
    return S.Case(name, "mm_lombscargle_f64", "lomb", data, setup, ragged=ragged)


def torch_real(z):
    import torch
    return torch.view_as_real(z)


def _ctypes_case():
    """Every instance has its own buffers, outputs and workspace; the time axis and the grid are shared."""
    name = "lomb/ragged-ctypes"

    def setup(env):
        import torch
        from modulation_mfcc_amd import _lib
        lib = _lib.load()
        td = torch.from_numpy(O.time_axis(S_N)).to(env.gpu)
        od = torch.from_numpy(2.0 * np.pi * S_F).to(env.gpu)
        env.keep += [td, od]
        re, im = env.out((S_ROWS, len(S_F)), torch.float64), env.out((S_ROWS, len(S_F)), torch.float64)
        need = int(lib.mm_lombscargle_workspace_bytes(S_ROWS, S_N, len(S_F)))
        assert need > 0
        ws = env.work(need)
        flags = _lib.MM_LOMB_PRECENTER | _lib.MM_LOMB_FLOATING_MEAN | _lib.MM_LOMB_AMPLITUDE

        def call():
            _lib.check(lib.mm_lombscargle_f64(env.buf["x"].data_ptr(), S_ROWS, S_N, S_N, env.buf["lengths"].data_ptr(),
                                              td.data_ptr(), od.data_ptr(), len(S_F), flags, re.data_ptr(), len(S_F),
                                              im.data_ptr(), ws.data_ptr(), need, S.stream()), "mm_lombscargle_f64")
            return re, im
        return call
    return S.Case(name, "mm_lombscargle_f64", "lomb",
                  lambda: {"x": _curves(name), "lengths": S.length_sets(S_ROWS, S_N, 37)}, setup, ragged=True, threads=True)


STREAM_CASES = [_wrapper_case(False), _wrapper_case(True), _ctypes_case()]
_SESSION = []


@pytest.fixture(scope="module")
def stream_session(gpu):
    """test_gpu_streams.Session over STREAM_CASES instead of the registry: the entries, the calibrated gate, the side stream."""
    if not _SESSION:
        _SESSION.append(TS.Session(gpu, cases=STREAM_CASES))
    return _SESSION[0]


def test_the_stream_cases_are_not_in_the_registry():
    assert not {c.name for c in S.CASES} & {c.name for c in STREAM_CASES}
    assert all(c.entry == "mm_lombscargle_f64" for c in STREAM_CASES)


@pytest.mark.parametrize("case", STREAM_CASES, ids=lambda c: c.name)
def test_behind_a_gate_on_a_side_stream(case, stream_session):
    e = stream_session.get(case)
    assert e.reproducible, "two eager calls on the same data differ in a bit"
    TS.test_side_stream_order_and_asynchrony(case, stream_session)


@pytest.mark.parametrize("case", STREAM_CASES, ids=lambda c: c.name)
def test_captured_and_replayed_four_times(case, stream_session):
    TS.test_capture_and_replay(case, stream_session)


def test_two_threads(stream_session, gpu):
    TS.test_one_plan_two_threads(STREAM_CASES[2], stream_session, gpu)


def test_first_calls_of_a_process_on_two_threads():
    """A fresh process whose two threads make the FIRST calls of the process at the same moment: tests/_lomb_worker.py
    compares both threads' results with the serial call made afterwards and exits non-zero on a difference."""
    import os
    import subprocess
    import sys
    from conftest import ROOT
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_lomb_worker.py")], cwd=ROOT, capture_output=True,
                       text=True, timeout=240)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    assert "first calls ok" in r.stdout


# ---- refusals: before any launch, outputs untouched ------------------------------------------------------------------------------
def test_refusals_leave_the_outputs_untouched(gpu):
    import torch
    from modulation_mfcc_amd import _lib
    lib = _lib.load()
    rows, n, nf = 3, 2 * _chunk() + 5, 7
    x = dev(gapped_rows(rows, n, "refuse"), gpu)
    td, od = dev(O.time_axis(n), gpu), dev(2.0 * np.pi * O.grid(n, count=nf), gpu)
    need = int(lib.mm_lombscargle_workspace_bytes(rows, n, nf))
    ws = torch.empty(need + 256, dtype=torch.uint8, device=gpu)
    assert ws.data_ptr() % 256 == 0
    re = torch.full((rows, nf), -7.0, dtype=torch.float64, device=gpu)
    im = torch.full((rows, nf), -7.0, dtype=torch.float64, device=gpu)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(nf_=nf, flags=0, im_=None, ws_=ws.data_ptr(), wb=need):
        return lib.mm_lombscargle_f64(x.data_ptr(), rows, n, n, None, td.data_ptr(), od.data_ptr(), nf_, flags, re.data_ptr(),
                                      nf, im_, ws_, wb, st)
    assert call(wb=need - 1) == _lib.MM_ERR_WORKSPACE
    assert call(ws_=ws.data_ptr() + 8) == _lib.MM_ERR_WORKSPACE
    assert call(ws_=None) == _lib.MM_ERR_WORKSPACE
    assert call(nf_=0) == _lib.MM_ERR_INVALID_ARG
    assert call(flags=_lib.MM_LOMB_AMPLITUDE) == _lib.MM_ERR_INVALID_ARG
    assert call(flags=3 << 2) == _lib.MM_ERR_INVALID_ARG
    torch.cuda.synchronize()
    assert (re == -7.0).all() and (im == -7.0).all()
    assert call(flags=_lib.MM_LOMB_AMPLITUDE, im_=im.data_ptr()) == _lib.MM_OK
    torch.cuda.synchronize()
    assert torch.isfinite(re).all() and torch.isfinite(im).all()
