"""GPU: the Welch modulation power spectrum (modulation_psd_batch, modulation_psd_ragged_batch, MfccPlan.mfcc_modpsd;
mm_modpsd_f32) against the yardstick of tests/modpsd_oracle.py, the ragged identities bit for bit, values that need no
reference, and the stream contract of mm_modpsd_f32 with the steps of tests/test_gpu_streams.py.

The kernel gives segment i of a row to chunk i // 32 (a workgroup) and wave i % 4 of it: the segment counts below are 1, 1,
2, 7 (a remainder over the four waves), 33 (one more than a full chunk: the two-launch route) and 70 (two full chunks and a
remainder).
"""
import itertools

import numpy as np
import pytest

import modpsd_oracle as O
import stream_cases as S
import test_gpu_streams as TS

pytestmark = pytest.mark.gpu

FS = 200.0
SIZES = [(32, 32), (64, 64), (100, 128), (128, 128), (256, 256), (512, 512), (1000, 1024), (1024, 1024), (2048, 2048),
         (3000, 4096), (4096, 4096)]
COMBOS = list(itertools.product((False, "constant", "linear"), ("density", "spectrum"), ("hann", "boxcar", "array")))
SEGMENTS = (1, 1, 2, 7, 33, 70)


def window_of(name, nperseg):
    """'hann' and 'boxcar' go to the device by name, 'array' as a float64 Kaiser window of nperseg values."""
    return np.kaiser(nperseg, 7.4) if name == "array" else name


def lengths_of(nperseg, noverlap, counts=SEGMENTS):
    """Row lengths with 1, 1 (nperseg + step - 1: still one), 2, 7, 33, 70 segments, half a step beyond the last one."""
    step = nperseg - noverlap
    ns = [nperseg, nperseg + step - 1]
    ns += [nperseg + (k - 1) * step + (step - 1) // 2 for k in counts[2:]]
    ns[2] = nperseg + step          # exactly two
    return sorted(set(ns))


def overlaps_of(nperseg):
    return (0, nperseg // 2, nperseg - 1)


def device_psd(x, p, gpu):
    import torch
    from modulation_mfcc_amd import modulation_psd_batch
    f, P = modulation_psd_batch(torch.from_numpy(np.array(x)).to(gpu), p.fs, **p.kwargs())
    return f, P.cpu().numpy()


def check_one(p, T, gpu, rows=None):
    x = O.rows_for(p, T)
    if rows is not None:
        x = O.take(x, rows)
    f, got = device_psd(x, p, gpu)
    assert got.dtype == np.float32 and got.shape == (x.shape[0], p.bins)
    np.testing.assert_array_equal(f, O.welch64(x[:1], p)[0])
    c = O.check(got, x, p, "modulation_psd_batch")
    print(f"nperseg {p.nperseg} nfft {p.nfft} noverlap {p.noverlap} {p.detrend} {p.scaling} T {T}: c {c:.2f} "
          f"(tolerance {O.tolerance(p, T):.2f})")


# ---- against the yardstick ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i_nov", (0, 1, 2), ids=("no-overlap", "half", "hop1"))
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}in{s[1]}")
def test_every_transform_length_against_the_yardstick(size, i_nov, gpu):
    """Every nfft, with nperseg = nfft and with an nperseg that is no power of two; every length of lengths_of(); detrend,
    scaling and window cycle through their 18 combinations (test_all_combinations has the full product)."""
    nperseg, nfft = size
    noverlap = overlaps_of(nperseg)[i_nov]
    counts = SEGMENTS if nfft < 2048 else SEGMENTS[:5]          # (70 segments of 4096 points x 16 rows: host time only)
    for i_n, T in enumerate(lengths_of(nperseg, noverlap, counts)):
        detrend, scaling, win = COMBOS[(7 * SIZES.index(size) + 5 * i_nov + 11 * i_n) % len(COMBOS)]
        check_one(O.Params(FS, window_of(win, nperseg), nperseg, noverlap, nfft, detrend, scaling), T, gpu)


@pytest.mark.parametrize("i_nov", (0, 1, 2), ids=("no-overlap", "half", "hop1"))
@pytest.mark.parametrize("size", [(64, 64), (100, 128)], ids=lambda s: f"{s[0]}in{s[1]}")
def test_all_combinations(size, i_nov, gpu):
    nperseg, nfft = size
    noverlap = overlaps_of(nperseg)[i_nov]
    for detrend, scaling, win in COMBOS:
        for T in lengths_of(nperseg, noverlap):
            check_one(O.Params(FS, window_of(win, nperseg), nperseg, noverlap, nfft, detrend, scaling), T, gpu)


@pytest.mark.parametrize("rows", (1, 5, 37))
def test_row_counts(rows, gpu):
    for nperseg, nfft, T in ((100, 128, 100 + 50 * 6 + 9), (512, 512, 512 + 256 * 33)):
        check_one(O.Params(FS, "hann", nperseg, None, nfft), T, gpu, rows=rows)


def test_defaults_are_scipys_but_for_nfft(gpu):
    import torch
    from modulation_mfcc_amd import modulation_psd_batch
    p = O.Params(FS, "hann", 256, 128, 256, "constant", "density")
    x = O.rows_for(p, 1001)
    f, P = modulation_psd_batch(torch.from_numpy(np.array(x)).to(gpu), FS)
    O.check(P.cpu().numpy(), x, p, "defaults")
    q = O.Params(FS, "hann", 100, 50, 128, "constant", "density")            # nfft: 128, not scipy's 100
    f, P = modulation_psd_batch(torch.from_numpy(np.array(x)).to(gpu).reshape(2, 8, 1001), FS, nperseg=100)
    assert P.shape == (2, 8, 65) and f.shape == (65,)
    O.check(P.reshape(16, 65).cpu().numpy(), x, q, "nperseg 100")
    with pytest.raises(ValueError, match="greater than the input length"):
        modulation_psd_batch(torch.from_numpy(np.array(x)).to(gpu)[:, :255], FS)


def test_row_stride_and_offset_base(gpu):
    """Rows with a pitch > n whose first sample lies one float behind an aligned address, NaN around them."""
    import torch
    from modulation_mfcc_amd import modulation_psd_batch
    p = O.Params(FS, "hann", 100, 50, 128, "linear", "density")
    T = 100 + 50 * 33 + 3
    x = O.rows_for(p, T)
    big = torch.full((16, T + 9), float("nan"), device=gpu)
    view = big[:, 1:1 + T]
    view.copy_(torch.from_numpy(np.array(x)))
    assert view.stride(0) == T + 9 and view.data_ptr() % 8 == 4
    _, got = modulation_psd_batch(view, FS, **p.kwargs())
    _, want = modulation_psd_batch(view.contiguous(), FS, **p.kwargs())
    assert TS.bit_equal(got, want)
    O.check(got.cpu().numpy(), x, p, "strided rows")


@pytest.mark.parametrize("T", (100 + 50 * 6, 100 + 50 * 40), ids=("one-launch", "two-launches"))
def test_psd_stride_and_guard_band(T, gpu):
    """mm_modpsd_f32 with psd_stride = bins + 7: the seven floats behind every row keep their bits."""
    import torch
    from modulation_mfcc_amd import _lib, modpsd, modulation_psd_batch
    lib = _lib.load()
    p = O.Params(FS, "hann", 100, 50, 128)
    x = torch.from_numpy(np.array(O.rows_for(p, T))).to(gpu)
    spec = modpsd._Spec(FS, **p.kwargs())
    plan = modpsd._modpsd_plan(spec, gpu)
    need = int(lib.mm_modpsd_workspace_bytes(plan.h, 16, T))
    assert (need > 0) == (p.num_segments(T) > 32)
    ws = torch.empty(max(need, 8), dtype=torch.uint8, device=gpu)
    out = torch.full((16, p.bins + 7), -7.0, device=gpu)
    args = (plan.h, x.data_ptr(), 16, T, T, None, out.data_ptr(), p.bins + 7, ws.data_ptr(), need, S.stream())
    _lib.check(lib.mm_modpsd_f32(*args), "mm_modpsd_f32")
    torch.cuda.synchronize()
    assert (out[:, p.bins:] == -7.0).all()
    assert TS.bit_equal(out[:, :p.bins].contiguous(), modulation_psd_batch(x, FS, **p.kwargs())[1])
    # refusals: a pitch below the row, a short workspace, no lengths and no segment
    assert lib.mm_modpsd_f32(*args[:7], p.bins - 1, *args[8:]) == _lib.MM_ERR_INVALID_ARG
    assert lib.mm_modpsd_f32(*args[:4], T - 1, *args[5:]) == _lib.MM_ERR_INVALID_ARG
    if need:
        assert lib.mm_modpsd_f32(*args[:9], need - 1, args[10]) == _lib.MM_ERR_WORKSPACE
    assert lib.mm_modpsd_f32(plan.h, x.data_ptr(), 16, 99, T, None, out.data_ptr(), p.bins + 7, None, 0, S.stream()) == _lib.MM_ERR_INVALID_ARG


# ---- ragged ------------------------------------------------------------------------------------------------------------------
RP = dict(window="hann", nperseg=64, noverlap=32, nfft=64, detrend="constant", scaling="density")
R_NMAX = 64 + 32 * 40                      # 41 segments: two chunks
R_LENS = [R_NMAX, 64, 65, 95, 96, 200, 64 + 32 * 31, 64 + 32 * 32, 64 + 32 * 32 - 1, 1000, 777]


def _ragged_rows(gpu, rows=len(R_LENS), seed=0):
    import torch
    g = np.random.default_rng(seed)
    x = (3.0 + g.standard_normal((rows, R_NMAX))).astype(np.float32)
    lens = np.array([R_LENS[i % len(R_LENS)] for i in range(rows)], dtype=np.int64)
    return torch.from_numpy(np.array(x)).to(gpu), lens


def test_ragged_rows_equal_the_rows_alone(gpu):
    import torch
    from modulation_mfcc_amd import modulation_psd_batch, modulation_psd_ragged_batch
    x, lens = _ragged_rows(gpu)
    f, P = modulation_psd_ragged_batch(x, lens, FS, **RP)
    fd, Pd = modulation_psd_ragged_batch(x, torch.from_numpy(lens).to(gpu), FS, **RP)
    assert TS.bit_equal(P, Pd) and (f == fd).all()
    for b, n in enumerate(lens):
        f1, alone = modulation_psd_batch(x[b:b + 1, :n], FS, **RP)
        assert TS.bit_equal(P[b:b + 1], alone), (b, int(n))
        assert (f == f1).all()
    p = O.Params(FS, **RP)
    for b in (1, 5, 7):                     # and against the reference: one, five and 33 segments
        O.check(P[b].cpu().numpy(), x[b, :lens[b]].cpu().numpy(), p, f"ragged row {b}")


def test_short_rows_nan_on_the_device_and_refused_on_the_host(gpu):
    import torch
    from modulation_mfcc_amd import modulation_psd_ragged_batch
    x, lens = _ragged_rows(gpu)
    lens = lens.copy()
    lens[3], lens[6] = 63, 1
    with pytest.raises(ValueError, match=r"row 3 has 63 samples"):
        modulation_psd_ragged_batch(x, lens, FS, **RP)
    _, P = modulation_psd_ragged_batch(x, torch.from_numpy(lens).to(gpu), FS, **RP)
    _, full = modulation_psd_ragged_batch(x, _ragged_rows(gpu)[1], FS, **RP)
    bad = torch.zeros(len(lens), dtype=torch.bool, device=gpu)
    bad[3] = bad[6] = True
    assert torch.isnan(P[bad]).all() and TS.bit_equal(P[~bad], full[~bad])
    # lengths outside [1, n_max] are clamped on the device; one launch (n_max with at most 32 segments): NaN rows too
    wild = torch.tensor([10 ** 12, 0, -5, 64], device=gpu)
    _, Pw = modulation_psd_ragged_batch(x[:4], wild, FS, **RP)
    _, ref = modulation_psd_ragged_batch(x[:4], torch.tensor([R_NMAX, 1, 1, 64], device=gpu), FS, **RP)
    assert TS.bit_equal(Pw, ref) and torch.isnan(Pw[1:3]).all() and not torch.isnan(Pw[[0, 3]]).any()
    _, Ps = modulation_psd_ragged_batch(x[:4, :500], torch.tensor([500, 63, 64, 1], device=gpu), FS, **RP)
    assert torch.isnan(Ps[[1, 3]]).all() and not torch.isnan(Ps[[0, 2]]).any()
    with pytest.raises(ValueError, match="greater than the input length"):
        modulation_psd_ragged_batch(x[:4, :63], torch.tensor([63, 63, 64, 1], device=gpu), FS, **RP)
    with pytest.raises(ValueError, match=r"lengths must lie in \[1, "):
        modulation_psd_ragged_batch(x, np.where(lens == 1, 0, lens), FS, **RP)


def test_padding_never_matters_and_rows_permute(gpu):
    import torch
    from modulation_mfcc_amd import modulation_psd_ragged_batch
    x, lens = _ragged_rows(gpu)
    _, P = modulation_psd_ragged_batch(x, lens, FS, **RP)
    cols = torch.arange(R_NMAX, device=gpu)[None, :] >= torch.from_numpy(lens).to(gpu)[:, None]
    for fill in (float("nan"), float("inf"), None):
        y = x.clone()
        y[cols] = (1e6 * torch.randn(int(cols.sum()), device=gpu)) if fill is None else fill
        assert TS.bit_equal(modulation_psd_ragged_batch(y, lens, FS, **RP)[1], P), fill
    perm = np.random.default_rng(1).permutation(len(lens))
    _, Pp = modulation_psd_ragged_batch(x[torch.from_numpy(perm).to(gpu)], lens[perm], FS, **RP)
    assert TS.bit_equal(Pp, P[torch.from_numpy(perm).to(gpu)])


def test_a_row_of_37_equals_the_row_alone(gpu):
    from modulation_mfcc_amd import modulation_psd_batch, modulation_psd_ragged_batch
    x, lens = _ragged_rows(gpu, rows=37, seed=2)
    _, P = modulation_psd_ragged_batch(x, lens, FS, **RP)
    _, U = modulation_psd_batch(x, FS, **RP)
    for b in (0, 1, 6, 7, 20, 36):
        assert TS.bit_equal(P[b:b + 1], modulation_psd_ragged_batch(x[b:b + 1], lens[b:b + 1], FS, **RP)[1]), b
        assert TS.bit_equal(P[b:b + 1], modulation_psd_batch(x[b:b + 1, :lens[b]], FS, **RP)[1]), b
        assert TS.bit_equal(U[b:b + 1], modulation_psd_batch(x[b:b + 1], FS, **RP)[1]), b


# ---- values that need no reference ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", (64 + 32 * 6, R_NMAX), ids=("one-launch", "two-launches"))
def test_zero_row_and_nan_row(T, gpu):
    import torch
    from modulation_mfcc_amd import modulation_psd_batch
    x = torch.randn(5, T, device=gpu) + 2.0
    x[1] = 0.0
    x[3, T // 2] = float("nan")
    for detrend in (False, "constant", "linear"):
        _, P = modulation_psd_batch(x, FS, **dict(RP, detrend=detrend))
        assert (P[1].view(torch.int32) == 0).all(), "the zero row must be +0.0 in every bin"
        assert torch.isnan(P[3]).all()
        assert torch.isfinite(P[[0, 2, 4]]).all() and (P[[0, 2, 4]] >= 0).all()


def test_parseval_on_the_device(gpu):
    """Boxcar, no detrend, no overlap, 'density', nfft = nperseg = n: sum_k P_k df = mean x^2 over the used samples.  The
    yardstick bounds |G_k - A_k| <= t (A_k + L N), t = 4 * 2^-24 (its margin at C_ref = 1: never wider than its own),
    L = log2 n; with sum_k d_k A_k^2 = n N^2 and (Cauchy-Schwarz) sum_k d_k A_k <= n N that gives
    |sum P df - mean x^2| <= 2 t (1 + L) mean x^2 to first order in t (1 % is added for the second)."""
    import torch
    from modulation_mfcc_amd import modulation_psd_batch
    for n, K in ((64, 5), (64, 70), (1024, 3)):
        p = O.Params(FS, "boxcar", n, 0, n, False, "density")
        x = O.rows_for(p, n * K + 9)
        f, P = modulation_psd_batch(torch.from_numpy(np.array(x)).to(gpu), FS, **p.kwargs())
        total = P.double().sum(dim=1).cpu().numpy() * (f[1] - f[0])
        want = (x[:, :n * K].astype(np.float64) ** 2).mean(axis=1)
        bound = 2 * O.MARGIN * O.EPS * (1 + np.log2(n)) * 1.01 * want
        assert (np.abs(total - want) <= bound).all(), (n, K, np.abs(total - want) / np.maximum(bound, 1e-300))


def test_a_cosine_on_a_bin_has_half_its_squared_amplitude(gpu):
    """Boxcar, 'spectrum', no detrend: amp cos(2 pi k0 j / n) gives amp^2 / 2 at k0.  |X_k0| = amp n / 2 and
    N = amp sqrt(n / 2), so the yardstick's bound at C_ref = 1 is a relative 2 * 4 * 2^-24 (1 + log2(n) sqrt(2 / n)) on
    the power; rounding the samples to float32 adds at most 2 * 2^-24."""
    import torch
    from modulation_mfcc_amd import modulation_psd_batch
    for n, k0, amp in ((64, 5, 3.0), (512, 100, 0.25), (4096, 1000, 1e3)):
        j = np.arange(n * 3, dtype=np.int64)
        x = (amp * np.cos(2 * np.pi * ((k0 * j) % n) / n)).astype(np.float32)
        _, P = modulation_psd_batch(torch.from_numpy(np.array(x)).to(gpu), FS, window="boxcar", nperseg=n, noverlap=0, nfft=n,
                                    detrend=False, scaling="spectrum")
        got = float(P[k0])
        rel = 2 * O.EPS * (O.MARGIN * (1 + np.log2(n) * np.sqrt(2.0 / n)) + 1)
        assert abs(got - amp * amp / 2) <= rel * amp * amp / 2, (n, k0, got, amp * amp / 2, rel)
        others = P.clone()
        others[k0] = 0
        assert float(others.max()) <= 1e-9 * got


# ---- MfccPlan.mfcc_modpsd --------------------------------------------------------------------------------------------------------
WELCH = dict(nperseg=32, noverlap=24, detrend="linear")


def _clips(gpu):
    import torch
    import mfcc_oracle as MO
    a = torch.zeros(2, 16000, device=gpu)
    a[0] = torch.from_numpy(MO.synth_clip(0, 16000, 16000, "am").astype(np.float32)).to(gpu)
    a[1, :9600] = torch.from_numpy(MO.synth_clip(1, 9600, 16000, "am").astype(np.float32)).to(gpu)
    return a, np.array([16000, 9600], dtype=np.int64)


def test_mfcc_modpsd_is_modulation_psd_of_the_mfcc(gpu):
    import torch
    from modulation_mfcc_amd import MfccConfig, MfccPlan, mfcc_modpsd_batch, mfcc_modpsd_ragged_batch, modulation_psd_batch
    cfg = MfccConfig(**S.C1)
    plan = MfccPlan(cfg)
    audio, lens = _clips(gpu)
    fs = cfg.sr / cfg.hop_length
    mfcc, f, P = plan.mfcc_modpsd(audio, **WELCH)
    assert mfcc.shape == (2, 13, 101) and P.shape == (2, 13, 17) and TS.bit_equal(mfcc, plan.mfcc(audio))
    f2, P2 = modulation_psd_batch(mfcc, fs, **WELCH)
    assert TS.bit_equal(P, P2) and (f == f2).all() and (f == np.fft.rfftfreq(32, 1 / fs)).all()
    m3, f3, P3 = mfcc_modpsd_batch(audio, cfg, **WELCH)
    assert TS.bit_equal(P3, P) and TS.bit_equal(m3, mfcc)
    # ragged: each clip's spectrum is that of the clip alone, on the same grid
    for ln in (lens, torch.from_numpy(lens).to(gpu)):
        mr, fr, Pr = plan.mfcc_modpsd(audio, ln, **WELCH)
        assert (fr == f).all() and Pr.shape == (2, 13, 17)
        assert TS.bit_equal(mr, plan.mfcc_ragged(audio, ln)[0])
        for b, n in enumerate(lens):
            # the clip alone: through the ragged path too (mfcc() is another device path than mfcc_ragged(), equal to
            # mfcc_close and not to the bit: tests/test_gpu_ragged.py)
            m1, _, P1 = plan.mfcc_modpsd(audio[b:b + 1], ln[b:b + 1], **WELCH)
            assert TS.bit_equal(m1, mr[b:b + 1]) and TS.bit_equal(Pr[b:b + 1], P1), b
            T_b = (101, 61)[b]
            assert TS.bit_equal(Pr[b], modulation_psd_batch(mr[b, :, :T_b], fs, **WELCH)[1])
    assert TS.bit_equal(mfcc_modpsd_ragged_batch(audio, lens, cfg, **WELCH)[2], Pr)
    with pytest.raises(ValueError, match=r"clip 1 has 61 frames"):
        plan.mfcc_modpsd(audio, lens, nperseg=64)
    assert torch.isnan(plan.mfcc_modpsd(audio, torch.from_numpy(lens).to(gpu), nperseg=64)[2][1]).all()


# ---- the stream contract of mm_modpsd_f32 ------------------------------------------------------------------------------------------
# The cases are built with the registry's Case class but are NOT appended to stream_cases.CASES (the registry is pinned to
# the 47 entries of include/modmfcc.h); the three checks are those of test_gpu_streams.py, called with these cases.
SP = dict(window="hann", nperseg=64, noverlap=48, nfft=64, detrend="linear", scaling="density")
S_ROWS, S_N = 5, 64 + 16 * 50              # 51 segments: two launches, a workspace


def _wrapper_case(ragged):
    name = "modpsd/" + ("ragged-wrapper" if ragged else "wrapper")

    def data():
        d = {"x": S.audio_sets(name, S_ROWS, S_N)}
        if ragged:
            d["lengths"] = S.length_sets(S_ROWS, S_N, 64)
        return d

    def setup(env):
        from modulation_mfcc_amd import modulation_psd_batch, modulation_psd_ragged_batch
        if ragged:
            return lambda: modulation_psd_ragged_batch(env.buf["x"], env.buf["lengths"], FS, **SP)[1]
        return lambda: modulation_psd_batch(env.buf["x"], FS, **SP)[1]
    return S.Case(name, "mm_modpsd_f32", "modpsd", data, setup, ragged=ragged)


def _ctypes_case():
    """One handle for both thread instances; every instance has its own buffers, output and workspace."""
    name = "modpsd/ragged-ctypes"

    def setup(env):
        import torch
        from modulation_mfcc_amd import _lib, modpsd
        lib = _lib.load()
        spec = modpsd._Spec(FS, **SP)
        plan = env.plan(lambda: modpsd._ModpsdPlan(spec, env.gpu))
        out = env.out((S_ROWS, spec.bins), torch.float32)
        need = int(lib.mm_modpsd_workspace_bytes(plan.h, S_ROWS, S_N))
        assert need > 0
        ws = env.work(need)

        def call():
            _lib.check(lib.mm_modpsd_f32(plan.h, env.buf["x"].data_ptr(), S_ROWS, S_N, S_N, env.buf["lengths"].data_ptr(),
                                         out.data_ptr(), spec.bins, ws.data_ptr(), need, S.stream()), "mm_modpsd_f32")
            return out
        return call
    return S.Case(name, "mm_modpsd_f32", "modpsd",
                  lambda: {"x": S.audio_sets(name, S_ROWS, S_N), "lengths": S.length_sets(S_ROWS, S_N, 64)}, setup,
                  ragged=True, threads=True)


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
    assert all(c.entry == "mm_modpsd_f32" for c in STREAM_CASES)


@pytest.mark.parametrize("case", STREAM_CASES, ids=lambda c: c.name)
def test_behind_a_gate_on_a_side_stream(case, stream_session):
    e = stream_session.get(case)
    assert e.reproducible, "two eager calls on the same data differ in a bit"
    TS.test_side_stream_order_and_asynchrony(case, stream_session)


@pytest.mark.parametrize("case", STREAM_CASES, ids=lambda c: c.name)
def test_captured_and_replayed_four_times(case, stream_session):
    TS.test_capture_and_replay(case, stream_session)


def test_one_handle_two_threads(stream_session, gpu):
    TS.test_one_plan_two_threads(STREAM_CASES[2], stream_session, gpu)
