"""GPU (-m gpu): the Hilbert envelope sample by sample, and the forward transform of csrc/mm_hilbert.hip.inc bin by bin, on
every pass plan.

The envelope checks are hilbert_oracle.check: the error of every sample against |hilbert(x)| in the next higher precision,
normalised by the row's own propagated-error scale (the pair's, where two clips share a transform), at most MARGIN x
max(C_ref, 1) PER CASE ROW -- C_ref from scipy's same-precision transform and the host restatements of the chirp identity
and of the pairing, computed on the host.  The forward transform is checked with modspec_oracle.check.  The length lists
come from hilbert_oracle: test_hilbert_host.py asserts that, with these row counts, they reach every kernel instantiation
that any 2-3-5-7-smooth length up to 200 000 and any chirp transform of 2^5 .. 2^19 points reaches.  Each test prints
"hilbert-c ..." lines (shown with -s): docs/experiments.md holds the table."""
import ctypes as C

import numpy as np
import pytest

import hilbert_oracle as H
import modspec_oracle as M

pytestmark = pytest.mark.gpu

DTYPES = ("float32", "float64")
BIG = 20000             # beyond: three layouts at 5 rows only (a row pitch enters the index arithmetic, not the pass plan)


def _dev(x, gpu):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).to(gpu)


def _layouts(x, gpu):
    """(name, device view of x): contiguous; odd row pitch; even pitch starting one element into the buffer.  What lies between
    the rows is NaN: a sample taken from there shows in the whole row."""
    import torch
    R, L = x.shape
    xd = _dev(x, gpu)
    yield "contiguous", xd
    odd = torch.full((R, (L + 2) | 1), float("nan"), dtype=xd.dtype, device=gpu)
    odd[:, :L] = xd
    assert odd.stride(0) % 2 == 1
    yield "odd-pitch", odd[:, :L]
    off = torch.full((R, (L + 3) & ~1), float("nan"), dtype=xd.dtype, device=gpu)
    off[:, 1:1 + L] = xd
    view = off[:, 1:1 + L]
    assert view.stride(0) % 2 == 0 and view.data_ptr() % (2 * xd.element_size()) == xd.element_size()
    yield "offset", view


def _plan_name(n, ragged=False):
    p = H.passes(n, ragged)
    return ("chirp-%d:" % p["M"] if p["bluestein"] else "direct:") + ("-".join(str(r) for r in p["radix"]) or "none")


class _Worst:
    """The (c, C_ref, bound) closest to its bound per form; prints the hilbert-c lines."""

    def __init__(self):
        self.by_form = {}

    def add(self, form, triple):
        old = self.by_form.get(form)
        if old is None or triple[0] / triple[2] > old[0] / old[2]:
            self.by_form[form] = triple

    def note(self, n, dtype, plan=None):
        for form, (c, cr, tol) in sorted(self.by_form.items()):
            print(f"hilbert-c form={form} n={n} passes={plan or _plan_name(n)} dtype={np.dtype(dtype).name} c={c:.2f} "
                  f"C_ref={cr:.2f} bound={tol:.2f}")


def _envelope(x, gpu):
    import torch
    from modulation_mfcc_amd import calc
    got = calc.hilbert_envelope_batch(x if torch.is_tensor(x) else _dev(x, gpu))
    assert tuple(got.shape) == tuple(x.shape)
    return got.cpu().numpy()


def _form(n, rows):
    return "paired" if rows > 1 and n > 1 else "single"


# ---- the forward transform, bin by bin ----

@pytest.mark.parametrize("n", H.FORWARD_LENGTHS)
def test_forward_transform(n, gpu):
    """calc.rfft_rows_long (mm_hilbert_rfft_f32: the forward passes alone, every HALF store path) at every zero-padding edge,
    1 / 5 / 37 rows, three row layouts: radices 3, 5, 7, 9, 25, 49 and 625 as first and later passes."""
    from modulation_mfcc_amd import calc
    worst = 0.0
    for T in M.edge_lengths(n):
        if T < 1 or T > n:
            continue
        rows_all = M.cases(n, T)
        for R in (1, 5, 37):
            x = M.take(rows_all, R)
            for layout, view in _layouts(x, gpu):
                if n > BIG and R != 5 and layout != "contiguous":
                    continue
                got = calc.rfft_rows_long(view, n)
                assert tuple(got.shape) == (R, n // 2 + 1)
                worst = max(worst, M.check(got.cpu().numpy(), x, n, f"rfft_rows_long n {n} T {T} rows {R} {layout}"))
    print(f"hilbert-c form=forward n={n} passes={_plan_name(n)} dtype=float32 c={worst:.2f} C_ref={M.c_ref(n):.2f} "
          f"bound={M.tolerance(n):.2f}")


# ---- the envelope, sample by sample ----

@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", H.ENVELOPE_LENGTHS + H.BLUESTEIN_LENGTHS)
def test_envelope(n, dtype, gpu):
    """calc.hilbert_envelope_batch on the case rows: 1 row (the unpaired branches; hb_mid_kernel as loader and envelope store at
    one pass), 2, 5 (the last clip has no partner) and 37 rows, three row layouts."""
    ref = H.reference(n, dtype)
    worst = _Worst()
    for R in H.ENVELOPE_ROWS:
        x, idx = H.take(ref.rows, R)
        for layout, view in _layouts(x, gpu):
            if n > BIG and R != 5 and layout != "contiguous":
                continue
            form = _form(n, R)
            worst.add(form, H.check(_envelope(view, gpu), x, idx, n, dtype, form == "paired", f"rows {R} {layout}"))
    worst.note(n, dtype)


@pytest.mark.parametrize("n", H.LONG_CASES)
def test_envelope_long(n, gpu):
    """441 000 samples (passes 8, 9, 25, 5, 49: ten seconds at 44.1 kHz) and a length that goes through chirp transforms of 2^19
    points, five float32 rows each."""
    ref = H.reference(n, np.float32)
    x, idx = H.take(ref.rows, 5)
    worst = _Worst()
    worst.add("paired", H.check(_envelope(x, gpu), x, idx, n, np.float32, True, "5 rows"))
    worst.note(n, np.float32)


PAIR_LENGTHS = (8, 35, 256, 625, 4096, 9600, 46875, 511, 8193)      # one per pass family: mid alone, mid2 alone, behind passes, chirps


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", PAIR_LENGTHS)
def test_pairing(n, dtype, gpu):
    """The 1e-6 row between the 1e3 row and the mean-1e4 row, each held to its own scale; then a row with a NaN, with +inf and
    with -inf as row 0 (its partner is the quiet row) and as the last row of an odd count: NaN throughout, every other row
    within its bound."""
    ref = H.reference(n, dtype)
    x, idx = H.take(ref.rows, 5)
    assert idx[:3].tolist() == [H.ROW_LOUD, H.ROW_QUIET, H.ROW_MEAN1E4]
    worst = _Worst()
    got = _envelope(x, gpu)
    worst.add("paired", H.check(got, x, idx, n, dtype, True, "loud, quiet, mean-1e4"))
    quiet = H.errors(got[1:2], ref.want[idx[1:2]], H.sigma(x, True)[1:2], n, dtype,
                     H.stored(x, ref.want[idx], True)[1:2]).max()
    assert quiet <= H.bound(ref.c_ref("paired")[H.ROW_QUIET]), quiet
    for value in (np.nan, np.inf, -np.inf):
        for pos in (0, 4):
            bad, bad_idx = x.copy(), idx.copy()
            bad[pos, n // 3], bad_idx[pos] = value, -1
            worst.add("paired, non-finite neighbour", H.check(_envelope(bad, gpu), bad, bad_idx, n, dtype, True,
                                                              f"{value} in row {pos}"))
    worst.note(n, dtype)


@pytest.mark.parametrize("n,rows", [(256, 1000), (625, 1001), (35, 1000)])
def test_many_rows(n, rows, gpu):
    """The XCD-ordered block lists of the fused pairs with a block count that is no multiple of eight (256: 500 blocks, 625:
    501), and a plain pass plan beside them: every row within its bound, three rows spread through the batch again as
    single-row calls."""
    for dtype in DTYPES:
        ref = H.reference(n, dtype)
        x, idx = H.take(ref.rows, rows)
        got = _envelope(x, gpu)
        worst = _Worst()
        worst.add("paired", H.check(got, x, idx, n, dtype, True, f"{rows} rows"))
        for r in (1, rows // 2 + 1, rows - 1):
            one = _envelope(x[r:r + 1], gpu)
            worst.add("single", H.check(one, x[r:r + 1], idx[r:r + 1], n, dtype, False, f"row {r} alone"))
            if not x[r].any():
                assert (got[r] == 0).all() and (one == 0).all()
        worst.note(n, dtype)


@pytest.mark.parametrize("n", [625, 9600, 511])
def test_chunked_calls(n, gpu):
    """Nine rows under a workspace bound that takes two pairs: library calls of 4, 4 and 1 rows -- the last one a single
    unpaired row; the partner of a row is its neighbour in its own call."""
    from modulation_mfcc_amd import _lib, calc
    for dtype in DTYPES:
        ref = H.reference(n, dtype)
        x, idx = H.take(ref.rows, 9)
        hp = calc._hilbert_plan(n, 0 if dtype == "float32" else 1, gpu)
        per_pair = int(_lib.load().mm_hilbert_workspace_bytes(hp.h, 2))
        old = calc.HILBERT_WS_BYTES
        try:
            calc.HILBERT_WS_BYTES = 2 * per_pair
            got = _envelope(x, gpu)
        finally:
            calc.HILBERT_WS_BYTES = old
        worst = _Worst()
        for r0, r1 in ((0, 4), (4, 8), (8, 9)):
            form = _form(n, r1 - r0)
            worst.add(form, H.check(got[r0:r1], x[r0:r1], idx[r0:r1], n, dtype, form == "paired", f"rows {r0}:{r1}"))
        worst.note(n, dtype)


@pytest.mark.parametrize("n", [9600, 511])
def test_library_call_with_pitches(n, gpu):
    """mm_hilbert_envelope itself with x_stride = n + 3 and env_stride = n + 5 (the Python layer always passes env_stride = n):
    columns below n within the bound, columns at and beyond n untouched bit for bit."""
    import torch
    from modulation_mfcc_amd import _lib, calc
    lib = _lib.load()
    for dtype in DTYPES:
        ref = H.reference(n, dtype)
        x, idx = H.take(ref.rows, 5)
        tdt = torch.float32 if dtype == "float32" else torch.float64
        xd = torch.full((5, n + 3), float("nan"), dtype=tdt, device=gpu)
        xd[:, :n] = _dev(x, gpu)
        sentinel = -12345.6789
        env = torch.full((5, n + 5), sentinel, dtype=tdt, device=gpu)
        hp = calc._hilbert_plan(n, 0 if dtype == "float32" else 1, gpu)
        ws = torch.empty(int(lib.mm_hilbert_workspace_bytes(hp.h, 5)), dtype=torch.uint8, device=gpu)
        stream = C.c_void_p(torch.cuda.current_stream(gpu).cuda_stream)
        with torch.cuda.device(gpu):
            _lib.check(lib.mm_hilbert_envelope(hp.h, xd.data_ptr(), 5, n + 3, env.data_ptr(), n + 5, ws.data_ptr(), ws.numel(),
                                               stream), "mm_hilbert_envelope")
        out = env.cpu().numpy()
        assert (out[:, n:] == np.asarray(sentinel, dtype=dtype)).all()
        worst = _Worst()
        worst.add("paired, pitches", H.check(np.ascontiguousarray(out[:, :n]), x, idx, n, dtype, True, "pitched call"))
        worst.note(n, dtype)


# ---- the ragged call ----

def _ragged_lengths(n_max):
    want = {1, 2, 3, 5, 7, 8, 11, 13, 16, 31, 97, 100, 127, 625, 1000, 1021, 4093, 4096, 4097, 30240, 32749, 40000, 65521,
            n_max // 2 - 1, n_max // 2, n_max // 2 + 1, n_max - 3, n_max - 1, n_max}
    out = sorted(v for v in want if 1 <= v <= n_max)
    keep = [v for v in out if v < 16][:6] + [v for v in out if v >= 16][-8:]      # the shortest, and the class's own range
    return sorted(set(keep) | {n_max})


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("M_fft", H.RAGGED_M)
def test_ragged(M_fft, dtype, gpu):
    """calc.hilbert_envelope_ragged_batch with device lengths (one call at the transform length of n_max = M / 2): lengths from
    1 to n_max, smooth and prime, NaN behind every clip; every clip against the reference of its own valid samples, +0.0
    behind it."""
    import torch
    from modulation_mfcc_amd import calc
    n_max = M_fft // 2
    assert calc.hilbert_ragged_fft_size(n_max) == M_fft == H.passes(n_max, ragged=True)["M"]
    lengths = _ragged_lengths(n_max)
    x = np.full((len(lengths), n_max), np.nan, dtype=dtype)
    clips = []
    for b, L in enumerate(lengths):
        clips.append(H.rows_for(L, dtype)[(H.ROW_LOUD + 3 * b) % M.N_CASES])
        x[b, :L] = clips[-1]
    lens = torch.tensor(lengths, dtype=torch.int64, device=gpu)
    got = calc.hilbert_envelope_ragged_batch(_dev(x, gpu), lens).cpu().numpy()
    assert got.shape == x.shape
    worst = _Worst()
    for b, L in enumerate(lengths):
        assert (got[b, L:] == 0).all() and not np.signbit(got[b, L:]).any()
        worst.add("ragged", H.check_clip(got[b, :L], clips[b], M_fft, f"clip {b} of {L} samples"))
    worst.note(f"1..{n_max}", dtype, plan=_plan_name(n_max, ragged=True))
