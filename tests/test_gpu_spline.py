"""GPU: interp_nan_spline_batch / interp_nan_spline_ragged_batch (mm_interp_spline_f64, csrc/mm_spline.hip) against the
yardstick of tests/spline_oracle.py -- scipy's interp1d 'quadratic' / 'cubic' within max(1e-12, 16 x scipy's own rounding) of
the row's maximum -- on every length, end, gap pattern and knot count at which the kernels take another path; bit-for-bit
independence of the batch, of the row pitch and of what lies behind a ragged row's count; scipy's errors; the stream contract
of the two entries (the cases and checks of tests/test_gpu_streams.py).

Every measured c is printed before it is asserted (pytest -s shows them; docs/experiments.md lists a run)."""
import numpy as np
import pytest

import spline_oracle as O
import stream_cases as S
import test_gpu_streams as TS

pytestmark = pytest.mark.gpu

SEG = O.S


def dev(x, gpu, dtype=None):
    import torch
    t = torch.from_numpy(np.array(x)).to(gpu)            # (a copy: the fixtures are read-only)
    return t if dtype is None else t.to(dtype)


def fill(x, method, gpu):
    from modulation_mfcc_amd import interp_nan_spline_batch
    return interp_nan_spline_batch(dev(x, gpu), method).cpu().numpy()


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def stack(names):
    return np.stack([O.fixture(k) for k in names])


# ---- values -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", O.METHODS)
@pytest.mark.parametrize("n", O.LENGTHS)
def test_lengths_and_ends(gpu, n, method):
    names = [f"f0-{n}-{l}-{t}" for l, t in O.ENDS]
    got = fill(stack(names), method, gpu)
    for k, name in enumerate(names):
        O.check(got[k], name, method)


PATTERNS = ["scatter30", "every-second", "sparse40", "alt-1-59", "alt-1-1-1-97", "swallow", "single-nan", "five-knot"]


@pytest.mark.parametrize("method", O.METHODS)
@pytest.mark.parametrize("name", PATTERNS)
def test_gap_patterns(gpu, name, method):
    x = O.fixture(name)
    got = fill(x, method, gpu)
    O.check(got, name, method)
    valid = ~np.isnan(x)
    assert same_bits(got[valid], x[valid]), "valid samples are copied through"


@pytest.mark.parametrize("method", O.METHODS)
def test_exactly_k_plus_one_and_k_plus_two_valid_samples(gpu, method):
    for name in O.few_names(method):
        assert (~np.isnan(O.fixture(name))).sum() in (O.DEGREE[method] + 1, O.DEGREE[method] + 2)
        O.check(fill(O.fixture(name), method, gpu), name, method)
    # k + 1 samples are ONE polynomial: the same through any other k + 1 of its points
    x = O.fixture(O.few_names(method)[0])
    idx = np.where(~np.isnan(x))[0]
    poly = np.polynomial.Polynomial.fit(idx, x[idx], O.DEGREE[method])
    got = fill(x, method, gpu)
    assert np.abs(got - poly(np.arange(len(x)))).max() <= 1e-9 * np.abs(got).max()


@pytest.mark.parametrize("method", O.METHODS)
def test_rows_without_gaps_come_back_as_they_are(gpu, method):
    import torch
    from modulation_mfcc_amd import interp_nan_spline_batch
    full = O.curve(1001, "full")
    full[17] = -0.0
    full[18] = np.inf                                   # not a NaN: a sample like any other in a row without a gap
    assert same_bits(fill(full, method, gpu), full)
    both = np.stack([full, O.fixture("scatter30"), O.curve(1001, "full2")])
    got = fill(both, method, gpu)
    assert same_bits(got[0], full) and same_bits(got[2], both[2])
    O.check(got[1], "scatter30", method)
    short = np.array([1.0, 2.0])                        # fewer samples than the spline needs, but none missing
    assert same_bits(fill(short, method, gpu), short)
    e = torch.empty((0, 7), dtype=torch.float64, device=gpu)
    assert interp_nan_spline_batch(e, method).shape == (0, 7)


@pytest.mark.parametrize("method", O.METHODS)
@pytest.mark.parametrize("K", O.KNOT_COUNTS)
def test_knot_counts_around_the_chunk_size(gpu, K, method):
    from modulation_mfcc_amd import interp
    assert interp.SPLINE_CHUNK == SEG
    name = f"knots-{K}"
    assert (~np.isnan(O.fixture(name))).sum() == K
    O.check(fill(O.fixture(name), method, gpu), name, method)


@pytest.mark.parametrize("method", O.METHODS)
def test_three_chunks_beside_four_knots(gpu, method):
    big = O.fixture("three-chunks")
    n = len(big)
    assert (~np.isnan(big)).sum() - 2 > 2 * SEG
    small = O.chosen(n, 4, key="beside")
    got = fill(np.stack([big, small, big[::-1].copy()]), method, gpu)
    O.check(got[0], "three-chunks", method)
    O.check_row(got[1], small, method, "four knots beside three chunks")
    O.check_row(got[2], big[::-1].copy(), method, "three chunks reversed")
    assert same_bits(got[0], fill(big, method, gpu)) and same_bits(got[1], fill(small, method, gpu))


# ---- independence of the batch -------------------------------------------------------------------------------------------------------
MIXED = ["five-knot", "scatter30", "every-second", "sparse40", "alt-1-59", "alt-1-1-1-97", "single-nan"]


@pytest.mark.parametrize("method", O.METHODS)
def test_a_mixed_batch_equals_each_row_alone(gpu, method):
    x = np.concatenate([stack(MIXED), O.curve(1001, "whole")[None, :], O.chosen(1001, O.DEGREE[method] + 1)[None, :]])
    got = fill(x, method, gpu)
    for k in range(len(x)):
        assert same_bits(got[k], fill(x[k], method, gpu)), k
    assert same_bits(fill(x[::-1].copy(), method, gpu), got[::-1])


@pytest.mark.parametrize("method", O.METHODS)
def test_dtypes_and_strides(gpu, method):
    import torch
    from modulation_mfcc_amd import interp_nan_spline_batch
    x = stack(MIXED)
    want = interp_nan_spline_batch(dev(x, gpu), method)
    # float32 in, float32 out: the float64 result of the widened input, rounded
    x32 = dev(x, gpu, torch.float32)
    got32 = interp_nan_spline_batch(x32, method)
    assert got32.dtype == torch.float32
    assert torch.equal(got32, interp_nan_spline_batch(x32.to(torch.float64), method).to(torch.float32))
    h = interp_nan_spline_batch(dev(x[1:], gpu, torch.float16)[:, :200], method)     # (five-knot has one sample there)
    assert h.dtype == torch.float16 and h.shape == (len(x) - 1, 200) and not torch.isnan(h).any()
    # a wider row pitch is taken as it is, any other layout is copied
    wide = torch.full((len(x), 1001 + 13), 7.0, dtype=torch.float64, device=gpu)
    wide[:, :1001] = dev(x, gpu)
    assert torch.equal(interp_nan_spline_batch(wide[:, :1001], method), want)
    assert torch.equal(interp_nan_spline_batch(dev(x, gpu).t().contiguous().t(), method), want)
    assert torch.equal(interp_nan_spline_batch(dev(np.repeat(x, 2, axis=1), gpu)[:, ::2], method), want)
    assert torch.equal(interp_nan_spline_batch(dev(x[1], gpu), method), want[1])
    with pytest.raises(ValueError, match=r"\[n\] or \[rows, n\]"):
        interp_nan_spline_batch(dev(x, gpu)[None], method)
    with pytest.raises(TypeError, match="floating"):
        interp_nan_spline_batch(torch.ones(4, 9, dtype=torch.int64, device=gpu), method)


@pytest.mark.parametrize("method", O.METHODS)
def test_three_hundred_short_rows(gpu, method):
    x = np.stack([O.f0_like(40, key=i, lead=i % 3, tail=(i // 3) % 4) for i in range(300)])
    got = fill(x, method, gpu)
    assert same_bits(fill(x[::-1].copy(), method, gpu), got[::-1])
    for k in (0, 1, 63, 64, 255, 256, 299):
        assert same_bits(got[k], fill(x[k], method, gpu)), k
        O.check_row(got[k], x[k], method, f"short row {k}")


# ---- ragged ---------------------------------------------------------------------------------------------------------------------------
def ragged_batch():
    """[7, n_max]: rows of every kind, the counts 1, n_max, one in each segment, one behind a three-chunk row's last knot."""
    big = O.fixture("three-chunks")
    n_max = len(big)
    x = np.stack([big, np.resize(O.fixture("scatter30"), n_max), np.resize(O.fixture("sparse40"), n_max),
                  O.f0_like(n_max, key=11, lead=7, tail=1), np.resize(O.fixture("every-second"), n_max),
                  O.curve(n_max, "ragged-whole"), O.f0_like(n_max, key=12)])
    counts = np.array([n_max, 1001, 977, 2 * SEG + 1, 1, SEG, SEG + 2], dtype=np.int64)
    return x, counts


@pytest.mark.parametrize("method", O.METHODS)
def test_ragged_rows_equal_the_single_call_bit_for_bit(gpu, method):
    import torch
    from modulation_mfcc_amd import interp_nan_spline_ragged_batch
    x, counts = ragged_batch()
    xd = dev(x, gpu)
    got = interp_nan_spline_ragged_batch(xd, counts, method)
    got_dev = interp_nan_spline_ragged_batch(xd, dev(counts, gpu), method)
    assert torch.equal(got, got_dev) and got.dtype == torch.float64 and got.shape == xd.shape
    g = got.cpu().numpy()
    for b, c in enumerate(counts):
        assert same_bits(g[b, :c], fill(x[b, :c], method, gpu)), b
        assert (g[b, c:] == 0).all() and not np.signbit(g[b, c:]).any(), b
    O.check(g[0], "three-chunks", method)
    O.check(g[1, :1001], "scatter30", method)
    # what lies behind a count never matters: NaN, infinities, another curve
    for junk in (np.nan, np.inf, None):
        y = x.copy()
        for b, c in enumerate(counts):
            y[b, c:] = O.curve(len(y[b]) - c, ("junk", b)) if junk is None else junk
        assert torch.equal(interp_nan_spline_ragged_batch(dev(y, gpu), counts, method), got), junk
    # device counts are clamped into [1, n_max]
    wild = counts.copy()
    wild[0], wild[4] = 10 * x.shape[1], -5
    assert torch.equal(interp_nan_spline_ragged_batch(xd, dev(wild, gpu), method), got)
    with pytest.raises(ValueError, match=r"counts must lie in \[1, "):
        interp_nan_spline_ragged_batch(xd, wild, method)
    got32 = interp_nan_spline_ragged_batch(xd.to(torch.float32), counts, method)
    assert got32.dtype == torch.float32 and not torch.isnan(got32).any()


# ---- errors ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", O.METHODS)
def test_too_few_valid_samples_raise_what_scipy_raises(gpu, method):
    from modulation_mfcc_amd import interp_nan_spline_batch, interp_nan_spline_ragged_batch
    k = O.DEGREE[method]
    good = O.fixture("scatter30")
    whole = O.curve(1001, "whole")
    for v in range(0, k + 1):
        bad = np.full(1001, np.nan)
        bad[np.arange(v) * 97 + 5] = 100.0 + np.arange(v)
        with pytest.raises(ValueError) as ref:
            O.recipe(bad, method)
        for x in (bad, np.stack([good, bad, whole])):
            with pytest.raises(ValueError) as e:
                interp_nan_spline_batch(dev(x, gpu), method)
            assert str(e.value) == str(ref.value), (v, str(e.value))
        # the ragged form counts the valid samples below the row's count: v of them here, ten more behind it
        r = np.stack([good, good, whole])
        r[1, :] = np.nan
        r[1, np.arange(v) * 3 + 1] = 50.0
        r[1, 40:50] = 60.0
        for counts in (np.array([1001, 30, 1001]), dev(np.array([1001, 30, 1001]), gpu)):
            with pytest.raises(ValueError) as e:
                interp_nan_spline_ragged_batch(dev(r, gpu), counts, method)
            assert str(e.value) == str(ref.value), (v, str(e.value))
        ok = interp_nan_spline_ragged_batch(dev(r, gpu), np.array([1001, 52, 1001]), method)       # v + 10 valid samples
        assert not np.isnan(ok.cpu().numpy()).any()
    # the row with the FEWEST valid samples decides; rows without a NaN (below their count) are exempt
    two, one = np.full(1001, np.nan), np.full(1001, np.nan)
    two[[4, 9]], one[[700]] = 1.0, 2.0
    with pytest.raises(ValueError) as ref:
        O.recipe(one, method)
    with pytest.raises(ValueError) as e:
        interp_nan_spline_batch(dev(np.stack([two, good, one]), gpu), method)
    assert str(e.value) == str(ref.value)
    r = np.stack([good, two, whole])                    # row 1 with a count of 1: its one sample is a NaN -> no valid sample
    with pytest.raises(ValueError) as ref:
        O.recipe(np.array([np.nan]), method)
    with pytest.raises(ValueError) as e:
        interp_nan_spline_ragged_batch(dev(r, gpu), np.array([1001, 1, 2]), method)
    assert str(e.value) == str(ref.value)
    r[1, 0] = 3.0                                       # ... and valid: a row without a NaN, however short
    got = interp_nan_spline_ragged_batch(dev(r, gpu), np.array([1001, 1, 2]), method).cpu().numpy()
    assert got[1, 0] == 3.0 and (got[1, 1:] == 0).all() and same_bits(got[2, :2], whole[:2]) and (got[2, 2:] == 0).all()
    O.check(got[0], "scatter30", method)


# ---- the stream contract of mm_interp_spline_f64 / mm_interp_spline_ragged_f64 --------------------------------------------------------------
# Built with the registry's Case class, NOT appended to stream_cases.CASES (pinned to include/modmfcc.h); the checks are those
# of test_gpu_streams.py.  2500 samples: three segments, two chunks of knots.
S_ROWS, S_N = 4, 2500
READ_BACK = ("interp_nan_spline_ragged_batch: 'taken from the smallest number of valid samples below a row's count, in one "
             "read-back'")


def _gap_sets(name):
    out = []
    for k in (0, 1):
        r = S._seed(name, k)
        x = np.cumsum(r.standard_normal((S_ROWS, S_N)), axis=1)
        x[r.random((S_ROWS, S_N)) < 0.3] = np.nan
        x[:, 0] = np.nan                     # a gap before the first and behind the last valid sample
        x[:, S_N - 3:] = np.nan
        x[:, 1:6] = 1.0 + k + np.arange(5)   # five valid samples below the smallest count
        out.append(x)
    return tuple(out)


def _data(name, ragged):
    d = {"x": _gap_sets(name)}
    if ragged:
        d["counts"] = S.length_sets(S_ROWS, S_N, 8)
    return d


def _wrapper_case(method, ragged):
    name = f"interp_spline/{'ragged-' if ragged else ''}wrapper-{method}"

    def setup(env):
        from modulation_mfcc_amd import interp_nan_spline_batch, interp_nan_spline_ragged_batch
        if ragged:
            return lambda: interp_nan_spline_ragged_batch(env.buf["x"], env.buf["counts"], method)
        return lambda: interp_nan_spline_batch(env.buf["x"], method)
    return S.Case(name, "mm_interp_spline" + ("_ragged" if ragged else "") + "_f64", "spline", lambda: _data(name, ragged), setup,
                  ragged=ragged, host_sync=READ_BACK)


def _ctypes_case(method, ragged):
    name = f"interp_spline/{'ragged-' if ragged else ''}ctypes-{method}"
    entry = "mm_interp_spline" + ("_ragged" if ragged else "") + "_f64"

    def setup(env):
        import torch
        from modulation_mfcc_amd import _lib, interp
        lib = _lib.load()
        kind = interp._SPLINE_KINDS[method]
        x = env.buf["x"]
        y = env.out((S_ROWS, S_N), torch.float64)
        need = int(lib.mm_interp_spline_workspace_bytes(kind, S_ROWS, S_N))
        ws = env.work(need)
        cnt = env.buf.get("counts")

        def call():
            if ragged:
                rc = lib.mm_interp_spline_ragged_f64(kind, x.data_ptr(), S_ROWS, S_N, S_N, cnt.data_ptr(), y.data_ptr(), S_N,
                                                     ws.data_ptr(), need, S.stream())
            else:
                rc = lib.mm_interp_spline_f64(kind, x.data_ptr(), S_ROWS, S_N, S_N, y.data_ptr(), S_N, ws.data_ptr(), need,
                                              S.stream())
            _lib.check(rc, entry)
            return y
        return call
    return S.Case(name, entry, "spline", lambda: _data(name, ragged), setup, ragged=ragged, threads=True)


STREAM_CASES = [_wrapper_case("cubic", False), _wrapper_case("quadratic", True), _ctypes_case("cubic", True),
                _ctypes_case("quadratic", False)]
GRAPH_CASES = [c for c in STREAM_CASES if c.host_sync is None]

_SESSION = []


@pytest.fixture(scope="module")
def stream_session(gpu):
    if not _SESSION:
        _SESSION.append(TS.Session(gpu, cases=STREAM_CASES))
    return _SESSION[0]


def test_the_stream_cases_are_not_in_the_registry():
    assert not {c.name for c in S.CASES} & {c.name for c in STREAM_CASES}
    assert {c.entry for c in STREAM_CASES} == {"mm_interp_spline_f64", "mm_interp_spline_ragged_f64"}
    from modulation_mfcc_amd import interp
    assert READ_BACK.split("'")[1] in " ".join(interp.interp_nan_spline_ragged_batch.__doc__.split())


@pytest.mark.parametrize("case", STREAM_CASES, ids=lambda c: c.name)
def test_behind_a_gate_on_a_side_stream(case, stream_session):
    e = stream_session.get(case)
    assert e.reproducible, "two eager calls on the same data differ in a bit"
    TS.test_side_stream_order_and_asynchrony(case, stream_session)


@pytest.mark.parametrize("case", GRAPH_CASES, ids=lambda c: c.name)
def test_captured_and_replayed_four_times(case, stream_session):
    TS.test_capture_and_replay(case, stream_session)


@pytest.mark.parametrize("case", GRAPH_CASES, ids=lambda c: c.name)
def test_two_threads(case, stream_session, gpu):
    TS.test_one_plan_two_threads(case, stream_session, gpu)


def test_the_stream_cases_compute_what_the_wrapper_computes(gpu, stream_session):
    import torch
    from modulation_mfcc_amd import interp_nan_spline_batch
    e = stream_session.get(STREAM_CASES[3])
    x = dev(_gap_sets(STREAM_CASES[3].name)[1], gpu)
    assert torch.equal(e.eager[1][0], interp_nan_spline_batch(x, "quadratic"))
