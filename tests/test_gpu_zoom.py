"""GPU: zoom_batch / zoom_ragged_batch / spline_filter_batch / spectrogram_image(_batch) (mm_zoom2d_*, csrc/mm_zoom.hip)
against the yardstick of tests/zoom_oracle.py -- scipy.ndimage.zoom within max(1e-12, 16 x scipy's own rounding) of the
image's maximum, cval bit for bit where scipy returns it -- on every order, mode, zoom factor, degenerate axis and segment
edge at which the kernels take another path; bit-for-bit independence of the batch, of the strides and of what lies behind
a ragged image's width; the non-finite guarantee; the stream contract of the four entries (the cases and checks of
tests/test_gpu_streams.py).

Every measured c is printed before it is asserted (pytest -s shows them; docs/experiments.md lists a run)."""
import numpy as np
import pytest
import scipy.ndimage

import stream_cases as S
import test_gpu_streams as TS
import zoom_oracle as O

pytestmark = pytest.mark.gpu


def seg():
    from modulation_mfcc_amd import zoom
    return zoom.ZOOM_SEGMENT            # the horizontal segment length, read from the module


def dev(x, gpu):
    import torch
    return torch.from_numpy(np.array(x)).to(gpu)            # (a copy: the fixtures are read-only)


def run(x, zoom, gpu, **kw):
    from modulation_mfcc_amd import zoom_batch
    return zoom_batch(dev(x, gpu), zoom, **kw).cpu().numpy()


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


# ---- values -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", O.MODES)
@pytest.mark.parametrize("order", O.ORDERS)
@pytest.mark.parametrize("shape", [(7, 59), (5, 129)], ids=str)
def test_orders_and_modes(gpu, shape, order, mode):
    x = O.image(*shape)
    for cval in (0.0, -7.5):
        got = run(x, 6, gpu, order=order, mode=mode, cval=cval)
        O.check(got, x, 6, order, mode, cval)
        last = got[:, -1]
        if mode == "constant" and shape[1] == 59:
            assert (last == cval).all(), "59 x 6: the last column is cval"
        else:
            assert (last != -7.5).all()
    x32 = O.image(*shape, dtype=np.float32)
    O.check(run(x32, 6, gpu, order=order, mode=mode, cval=-7.5), x32, 6, order, mode, -7.5)


FACTORS = [((5, 8), (1.5, 2.5)), ((9, 11), 1.3), ((12, 10), 0.5), ((33, 70), (0.5, 0.3)), ((4, 5), 1.0), ((6, 63), 2.5),
           ((6, 64), 2.5), ((40, 3), (7.3, 1.0)), ((300, 4), (0.05, 2))]


@pytest.mark.parametrize("case", FACTORS, ids=str)
def test_zoom_factors(gpu, case):
    shape, z = case
    x = O.image(*shape)
    if case == FACTORS[0]:
        assert run(x, z, gpu).shape == (8, 20)                              # 5 x 1.5 = 7.5 rounds to 8: ties to even
    for order in O.ORDERS:
        for mode in O.MODES:
            O.check(run(x, z, gpu, order=order, mode=mode, cval=2.25), x, z, order, mode, 2.25)


@pytest.mark.parametrize("shape", [(1, 7), (2, 7), (3, 7), (7, 1), (7, 2), (7, 3), (1, 1), (2, 2), (1, 2), (3, 1)], ids=str)
def test_degenerate_axes(gpu, shape):
    x = O.image(*shape)
    for z in (3, (2.5, 1.6)):
        for order in O.ORDERS:
            for mode in O.MODES:
                O.check(run(x, z, gpu, order=order, mode=mode, cval=-1.5), x, z, order, mode, -1.5)


def edge_widths():
    s = seg()
    return [s - 1, s, s + 1, 2 * s + 3, 2, 5, 40, 65]


EDGE_HEIGHTS = (1, 2, 129)


@pytest.mark.parametrize("k", range(8))
def test_segment_edges(gpu, k):
    from modulation_mfcc_amd import zoom
    w = edge_widths()[k]
    assert zoom.ZOOM_MAX_TAPS == 80 and sorted(edge_widths())[:4] == [2, 5, 40, 65]       # below the halo: several reflections
    for h in EDGE_HEIGHTS:
        x = O.image(h, w, key="edge")
        for order in (2, 3, 4, 5):
            O.check(run(x, (1.5, 2), gpu, order=order, cval=0.5), x, (1.5, 2), order, "constant", 0.5)
        O.check(run(x, (1.5, 2), gpu, order=5, mode="mirror"), x, (1.5, 2), 5, "mirror")


@pytest.mark.parametrize("order", [2, 3, 4, 5])
def test_the_prefilter_alone(gpu, order):
    import torch
    from modulation_mfcc_amd import spline_filter_batch
    for w in edge_widths() + [1]:
        for h in EDGE_HEIGHTS + (9, 90):
            x = O.image(h, w, key="filter")
            O.check_filter(spline_filter_batch(dev(x, gpu), order).cpu().numpy(), x, order)
    x32 = O.image(129, 65, key="filter", dtype=np.float32)
    got = spline_filter_batch(dev(x32, gpu), order)
    assert got.dtype == torch.float32
    O.check_filter(got.cpu().numpy(), x32, order)
    batch = np.stack([O.image(9, 40, key=i) for i in range(3)])
    got = spline_filter_batch(dev(batch, gpu), order).cpu().numpy()
    for i in range(3):
        assert same_bits(got[i], spline_filter_batch(dev(batch[i], gpu), order).cpu().numpy())


@pytest.mark.parametrize("mode", O.MODES)
@pytest.mark.parametrize("order", O.ORDERS)
def test_the_evaluation_alone(gpu, order, mode):
    for shape in ((7, 59), (5, 129)):
        x = O.image(*shape)
        O.check(run(x, 6, gpu, order=order, mode=mode, cval=-7.5, prefilter=False), x, 6, order, mode, -7.5, prefilter=False)


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_the_references_call(gpu, dtype):
    """script/praat_py_ui/spectrogram.py:70-71 on 10 * numpy.log10(values) of a strictly positive 129 x 300 power image."""
    from modulation_mfcc_amd import spectrogram_image, spectrogram_image_batch
    power = O.power(129, 300).astype(dtype)
    power64 = power.astype(np.float64)
    db64 = 10 * np.log10(power64)
    assert power.min() > 0 and db64.max() - db64.min() > 60
    want64 = scipy.ndimage.zoom(db64, 6, order=4)
    _, outside, b64, sp = O.reference(db64, 6, 4)
    assert want64.shape == (774, 1800) and not outside.any()
    # the dB image made by the caller, in the caller's type
    db = (10 * np.log10(power)).astype(dtype)
    O.check(spectrogram_image(dev(db, gpu)).cpu().numpy(), db, 6, 4, what=f"spectrogram_image {np.dtype(dtype).name}")
    assert spectrogram_image(dev(db, gpu), zoom_blur=False).shape == (129, 300)
    # the dB step on load, in float64, from the power image
    got = spectrogram_image_batch(dev(power, gpu), db=True).cpu().numpy()
    assert got.dtype == dtype and got.shape == want64.shape
    bound = O.bound_of(sp, dtype, float(np.abs(want64).max()))
    c = O.measure(got, want64.astype(dtype))
    print(f"spectrogram_image_batch {np.dtype(dtype).name}: c = {c:.3e}, bound = {bound:.3e}, spread = {sp:.3e}")
    assert c <= bound
    both = spectrogram_image_batch(dev(np.stack([power, power[::-1]]), gpu)).cpu().numpy()
    assert same_bits(both[0], got)


# ---- independence ---------------------------------------------------------------------------------------------------------------
def test_three_hundred_small_images(gpu):
    r = np.random.default_rng(300)
    x = r.standard_normal((300, 6, 9)) * 10.0 ** r.integers(-3, 4, size=(300, 1, 1))
    x[7] = 0.0
    x[8] = np.arange(54).reshape(6, 9)
    for order, mode in ((3, "constant"), (4, "mirror"), (1, "constant")):
        got = run(x, (2, 3.5), gpu, order=order, mode=mode, cval=1.0)
        assert got.shape == (300, 12, 32)
        assert same_bits(run(x[::-1].copy(), (2, 3.5), gpu, order=order, mode=mode, cval=1.0), got[::-1])
        for k in range(300):
            assert same_bits(got[k], run(x[k], (2, 3.5), gpu, order=order, mode=mode, cval=1.0)), k
        for k in (0, 1, 7, 8, 63, 64, 255, 256, 299):
            O.check(got[k], x[k], (2, 3.5), order, mode, 1.0)


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_strides_offsets_and_guard_bands(gpu, dtype):
    import torch
    from modulation_mfcc_amd import _lib, zoom_batch
    x = np.stack([O.image(9, 70, key=i, dtype=dtype) for i in range(3)])
    want = zoom_batch(dev(x, gpu), (2, 3), order=4, cval=-2.0)
    assert want.dtype == dev(x, gpu).dtype and want.shape == (3, 18, 210)
    # inputs: a window of a larger tensor (row pitch, image pitch, offset), a transposed layout, every second column
    big = torch.full((3, 9 + 5, 70 + 11), float("nan"), dtype=want.dtype, device=gpu)
    big[:, 2:11, 3:73] = dev(x, gpu)
    assert torch.equal(zoom_batch(big[:, 2:11, 3:73], (2, 3), order=4, cval=-2.0), want)
    assert torch.equal(zoom_batch(dev(x, gpu).transpose(1, 2).contiguous().transpose(1, 2), (2, 3), order=4, cval=-2.0), want)
    assert torch.equal(zoom_batch(dev(np.repeat(x, 2, axis=2), gpu)[:, :, ::2], (2, 3), order=4, cval=-2.0), want)
    assert torch.equal(zoom_batch(dev(x, gpu)[1], (2, 3), order=4, cval=-2.0), want[1])
    assert torch.equal(zoom_batch(dev(x[:1], gpu).expand(3, 9, 70), (2, 3), order=4, cval=-2.0)[2], want[0])
    # output: a window of a larger buffer through the C entry; the guard bands around it stay as they were
    lib = _lib.load()
    out = torch.full((3, 18 + 4, 210 + 6), 777.0, dtype=want.dtype, device=gpu)
    win = out[:, 1:19, 5:215]
    xd = dev(x, gpu)
    need = int(lib.mm_zoom2d_workspace_bytes(4, 3, 9, 70, 18, 210))
    ws = torch.empty(need, dtype=torch.uint8, device=gpu)
    fn = lib.mm_zoom2d_f32 if dtype == np.float32 else lib.mm_zoom2d_f64
    _lib.check(fn(4, 0, -2.0, 1, xd.data_ptr(), 3, 9, 70, 9 * 70, 70, 18, 210, win.data_ptr(), out.stride(0), out.stride(1),
                  ws.data_ptr(), need, S.stream()), "mm_zoom2d")
    torch.cuda.synchronize()
    assert torch.equal(win, want)
    guard = out.clone()
    guard[:, 1:19, 5:215] = 777.0
    assert (guard == 777.0).all()
    with pytest.raises(TypeError, match="float32 or float64"):
        zoom_batch(torch.ones(4, 9, dtype=torch.float16, device=gpu), 2)
    with pytest.raises(ValueError, match=r"\[H, W\]"):
        zoom_batch(dev(x, gpu)[None], 2)
    assert zoom_batch(dev(x, gpu), 0.01).shape == (3,) + scipy.ndimage.zoom(x[0], 0.01).shape == (3, 0, 1)


# ---- ragged ---------------------------------------------------------------------------------------------------------------------
def ragged_batch(dtype=np.float64):
    s = seg()
    widths = np.array([1, 2, 59, 64, s + 1, 5, 40, 2 * s + 3], dtype=np.int64)
    x = np.stack([O.image(5, int(widths.max()), key=("ragged", i), dtype=dtype) for i in range(8)])
    return x, widths


@pytest.mark.parametrize("order,mode,dtype", [(0, "constant", np.float64), (1, "constant", np.float64), (3, "constant", np.float64),
                                              (4, "constant", np.float64), (4, "mirror", np.float64), (5, "constant", np.float32)])
def test_ragged_images_equal_the_single_call_bit_for_bit(gpu, order, mode, dtype):
    import torch
    from modulation_mfcc_amd import zoom_ragged_batch
    x, widths = ragged_batch(dtype)
    z = (1.5, 6)
    xd = dev(x, gpu)
    got, wo = zoom_ragged_batch(xd, widths, z, order=order, mode=mode, cval=-7.5)
    got_dev, wo_dev = zoom_ragged_batch(xd, dev(widths, gpu), z, order=order, mode=mode, cval=-7.5)
    assert isinstance(wo, np.ndarray) and wo.dtype == np.int64 and wo.tolist() == [int(round(int(w) * 6)) for w in widths]
    assert wo_dev.dtype == torch.int64 and wo_dev.is_cuda and wo_dev.cpu().numpy().tolist() == wo.tolist()
    assert got.shape == (8, 8, int(wo.max())) and torch.equal(got, got_dev) and got.dtype == xd.dtype
    g = got.cpu().numpy()
    for b, w in enumerate(widths):
        alone = run(x[b, :, :w], z, gpu, order=order, mode=mode, cval=-7.5)
        assert same_bits(g[b, :, :wo[b]], alone), b
        assert (g[b, :, wo[b]:] == 0).all() and not np.signbit(g[b, :, wo[b]:]).any(), b
    O.check(g[2, :, :wo[2]], x[2, :, :59], z, order, mode, -7.5)            # (59 x 6: with the cval column in constant mode)
    O.check(g[7], x[7], z, order, mode, -7.5)
    # what lies behind a width never matters: NaN, infinities, another image
    for junk in (np.nan, np.inf, None):
        y = x.copy()
        for b, w in enumerate(widths):
            y[b, :, w:] = O.image(5, y.shape[2] - int(w), key=("junk", b)) if junk is None else junk
        assert torch.equal(zoom_ragged_batch(dev(y, gpu), widths, z, order=order, mode=mode, cval=-7.5)[0], got), junk
    # device widths are clamped into [1, W_max]
    wild = widths.copy()
    wild[7], wild[0] = 10 * x.shape[2], -5
    assert torch.equal(zoom_ragged_batch(xd, dev(wild, gpu), z, order=order, mode=mode, cval=-7.5)[0], got)
    with pytest.raises(ValueError, match=r"widths must lie in \[1, "):
        zoom_ragged_batch(xd, wild, z, order=order, mode=mode)


# ---- non-finite samples -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", O.ORDERS)
def test_every_output_whose_taps_touch_a_non_finite_sample_is_non_finite(gpu, order):
    h, w, iy, ix = 40, 300, 20, 150
    for bad, db in ((np.inf, False), (np.nan, False), (0.0, True)):         # (10 log10(0) = -inf)
        x = np.array(O.power(h, w, key="inf"))
        x[iy, ix] = bad
        for z in (2, (1.3, 0.7)):
            got = run(x, z, gpu, order=order, db=db)
            zy, zx = (z, z) if np.isscalar(z) else z
            oy, ty, _ = O.axis_plan(h, O.out_size(h, zy), order, "constant", np.float64)
            ox, tx, _ = O.axis_plan(w, O.out_size(w, zx), order, "constant", np.float64)
            touch = ((ty == iy).any(axis=1) & ~oy)[:, None] & ((tx == ix).any(axis=1) & ~ox)[None, :]
            assert touch.sum() >= 1 and not np.isfinite(got[touch]).any(), (bad, z, int(touch.sum()))


# ---- the stream contract of mm_zoom2d_f32 / _f64 / _ragged_f32 / _ragged_f64 -----------------------------------------------------
# Built with the registry's Case class, NOT appended to stream_cases.CASES (pinned to include/modmfcc.h); the checks are those
# of test_gpu_streams.py.  4 images of 9 x 140: two horizontal segments, two evaluation tiles across.
S_B, S_H, S_W, S_Z = 4, 9, 140, (2, 3)
S_HO, S_WO = 18, 420


def _data(name, ragged, dtype):
    d = {"x": tuple(S._seed(name, k).standard_normal((S_B, S_H, S_W)).astype(dtype) for k in (0, 1))}
    if ragged:
        d["widths"] = S.length_sets(S_B, S_W, 2)
    return d


def _wrapper_case(ragged, dtype, order, mode):
    name = f"zoom/{'ragged-' if ragged else ''}wrapper-{np.dtype(dtype).name}-order{order}-{mode}"
    entry = "mm_zoom2d_" + ("ragged_" if ragged else "") + ("f32" if dtype == np.float32 else "f64")

    def setup(env):
        from modulation_mfcc_amd import zoom_batch, zoom_ragged_batch
        if ragged:
            return lambda: zoom_ragged_batch(env.buf["x"], env.buf["widths"], S_Z, order=order, mode=mode, cval=-1.0)
        return lambda: zoom_batch(env.buf["x"], S_Z, order=order, mode=mode, cval=-1.0)
    return S.Case(name, entry, "zoom", lambda: _data(name, ragged, dtype), setup, ragged=ragged)


def _ctypes_case(ragged, dtype, order, mode):
    name = f"zoom/{'ragged-' if ragged else ''}ctypes-{np.dtype(dtype).name}-order{order}-{mode}"
    entry = "mm_zoom2d_" + ("ragged_" if ragged else "") + ("f32" if dtype == np.float32 else "f64")

    def setup(env):
        import torch
        from modulation_mfcc_amd import _lib, zoom
        lib = _lib.load()
        x = env.buf["x"]
        y = env.out((S_B, S_HO, S_WO), x.dtype)
        need = int(lib.mm_zoom2d_workspace_bytes(order, S_B, S_H, S_W, S_HO, S_WO))
        ws = env.work(need)
        wd = env.buf.get("widths")
        fn = getattr(lib, entry)
        head = (order, zoom._MODE_CODES[mode], -1.0, 1, x.data_ptr(), S_B, S_H, S_W, S_H * S_W, S_W)

        def call():
            tail = (S_HO, S_WO, y.data_ptr(), S_HO * S_WO, S_WO, ws.data_ptr(), need, S.stream())
            rc = fn(*head, wd.data_ptr(), float(S_Z[1]), *tail) if ragged else fn(*head, *tail)
            _lib.check(rc, entry)
            return y
        return call
    return S.Case(name, entry, "zoom", lambda: _data(name, ragged, dtype), setup, ragged=ragged, threads=True)


STREAM_CASES = [_wrapper_case(False, np.float64, 4, "constant"), _wrapper_case(True, np.float32, 3, "mirror"),
                _ctypes_case(False, np.float32, 5, "mirror"), _ctypes_case(True, np.float64, 4, "constant")]
GRAPH_CASES = [c for c in STREAM_CASES if c.host_sync is None]

_SESSION = []


@pytest.fixture(scope="module")
def stream_session(gpu):
    if not _SESSION:
        _SESSION.append(TS.Session(gpu, cases=STREAM_CASES))
    return _SESSION[0]


def test_the_stream_cases_are_not_in_the_registry():
    assert not {c.name for c in S.CASES} & {c.name for c in STREAM_CASES}
    assert {c.entry for c in STREAM_CASES} == {"mm_zoom2d_f32", "mm_zoom2d_f64", "mm_zoom2d_ragged_f32", "mm_zoom2d_ragged_f64"}
    assert len(GRAPH_CASES) == 4 and (O.out_size(S_H, S_Z[0]), O.out_size(S_W, S_Z[1])) == (S_HO, S_WO)


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
    from modulation_mfcc_amd import zoom_batch, zoom_ragged_batch
    for k, case in ((2, STREAM_CASES[2]), (3, STREAM_CASES[3])):
        e = stream_session.get(case)
        d = _data(case.name, case.ragged, np.float32 if k == 2 else np.float64)
        x = dev(d["x"][1], gpu)
        if case.ragged:
            want, wo = zoom_ragged_batch(x, dev(d["widths"][1], gpu), S_Z, order=4, mode="constant", cval=-1.0)
            assert want.shape == e.eager[1][0].shape
        else:
            want = zoom_batch(x, S_Z, order=5, mode="mirror", cval=-1.0)
        assert torch.equal(e.eager[1][0], want)
    x = O.image(S_H, S_W)
    O.check(run(x, S_Z, gpu, order=4, cval=-1.0), x, S_Z, 4, "constant", -1.0)
