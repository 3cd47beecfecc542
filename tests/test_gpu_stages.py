"""GPU (-m gpu): the STFT power and log-mel stages (rows A1-A5) bin by bin and filter by filter on every kernel path and
instantiation the dispatcher can select.

Every check is stage_oracle's: |sqrt(P) - |X|| and |lm - L| against the float64 reference of the same clips, normalised by
the FRAME's own floor, at most MARGIN x max(C_ref, 1) -- C_ref from the float32 host pipeline over the case set of the
configuration, computed on the host.  The 14 case clips go in one batch (clip boundaries fall inside tiles):

  * contiguous, at the lengths of stage_oracle.lengths (one frame, a partial tile, 63 / 64 / 65 / 66 frames);
  * at the longest of them in three row layouts (contiguous, odd pitch, one float into an even-pitch buffer) with NaN between
    the rows and one all-NaN clip in the middle of the batch, whose neighbours must stay finite and inside the bound;
  * at stage_oracle.aligned_lengths (the same lengths rounded up to multiples of 4) in a fourth layout the kernels with an
    alignment gate accept -- rows at 16 bytes, pitch n + 4, NaN in the gap, the all-NaN clip in the batch.

plan.kernel_path answers for a regular call; the call itself is dispatched again on its length, row pitch and pointer
(choose_kernel).  takes() restates those gates, and every figure is booked to the pinned kernel only for the calls it took;
the calls it handed over are held to the same bound and printed apart ("->handed-over").  Each pinned kernel must have taken
a partial tile, the 64- and 65-frame lengths and a longer batch with the NaN clip.  m12, h32, the pruned wave-per-frame
kernels and the embedded n_fft 64 / 128 / 256 plans have no power mode (mm_stft_power_f32 runs another kernel for them):
their log-mel rows are what pins them.  Each test prints the largest c per path ("stage-c ..." lines, shown with -s):
docs/experiments.md holds the table."""
import numpy as np
import pytest

import stage_oracle as S
from conftest import load_golden
from test_gpu_modspec import _layouts
from test_gpu_parity import _ANY_NFFT, _HALFBAND_CFGS, VARIANTS, _plan, _variant

pytestmark = pytest.mark.gpu

NAN_CLIP = 7        # where the all-NaN clip goes: behind the last tone, in front of the impulse at n - 1


def _golden(name):
    kw = load_golden(name)[0]
    return {k: kw[k] for k in ("sr", "n_fft", "win_length", "hop_length", "n_mels", "n_mfcc", "fmin", "fmax")}


def takes(path, n, view):
    """Whether a call of this length and layout runs on the kernel the plan names (choose_kernel, call = true): h32 wants
    n >= 4, n % 4 == 0, a pitch that is a multiple of 4 and rows at 16 bytes; m12 and w16s want n >= 4; the direct-load
    kernels w16 and w8 an even pitch, rows at 8 bytes and n >= 2; wave-per-frame n >= 2.  Whatever a kernel does not take
    goes to the next one that does (w16s, wave-per-frame, generic)."""
    pitch, ptr = view.stride(0), view.data_ptr()
    if path == "radix16-h32":
        return n >= 4 and n % 4 == 0 and pitch % 4 == 0 and ptr % 16 == 0
    if path in ("radix16-m12", "radix16-w16s"):
        return n >= 4
    if path in ("radix16-w16", "radix16-w8"):
        return n >= 2 and pitch % 2 == 0 and ptr % 8 == 0
    if path == "radix16-wpf":
        return n >= 2
    return True


def _with_nan_clip(x):
    return np.insert(x, NAN_CLIP, np.nan, axis=0), np.delete(np.arange(S.N_CASES + 1), NAN_CLIP)


def _batches(cfg, n, gpu, kind):
    """(layout, device view [B, n], the rows of it that are the case clips, whether the all-NaN clip is in the batch)."""
    import torch
    x = S.cases(n, cfg)
    if kind == "plain":
        yield "contiguous", torch.from_numpy(np.array(x)).to(gpu), np.arange(S.N_CASES), False
    elif kind == "layouts":
        xn, keep = _with_nan_clip(x)
        for name, view in _layouts(xn, gpu):
            yield name, view, keep, True
    else:
        assert kind == "aligned" and n % 4 == 0
        xn, keep = _with_nan_clip(x)
        buf = torch.full((xn.shape[0], n + 4), float("nan"), dtype=torch.float32, device=gpu)
        buf[:, :n] = torch.from_numpy(xn).to(gpu)
        view = buf[:, :n]
        assert view.stride(0) % 4 == 0 and view.data_ptr() % 16 == 0
        yield "aligned", view, keep, True


def _worst_of(c, bound, what, names):
    """Asserts c <= bound per clip, naming the worst element; returns c.max()."""
    per_clip = c.reshape(c.shape[0], -1).max(-1)
    bad = np.flatnonzero(~(per_clip <= bound))
    if bad.size:
        b, t, k = np.unravel_index(np.nanargmax(np.where(np.isnan(c), np.inf, c)), c.shape)
        raise AssertionError(f"{what}: clips {bad.tolist()} beyond c = {bound:.2f}; worst c = {c[b, t, k]:.4g} at clip {b} "
                             f"frame {t} {names} {k}; per clip {np.round(per_clip, 2).tolist()}")
    return float(per_clip.max())


def check(plan, cfg, n, view, keep, power, what):
    """One batch: plan.stft_power (where the path has a power mode) held to c_A on every clip, frame and bin, plan.logmel to
    c_L on every filter and frame, and the returned per-clip maximum equal to the maximum of the clip's returned rows bit for
    bit (every kernel takes it from the values it stores).  -> (c_A or None, c_L, frames per clip)."""
    ref = S.reference(cfg, n)
    bA, bL = S.bounds(cfg)
    T = ref.A.shape[1]
    assert plan.cfg.num_frames(n) == T and len(keep) == S.N_CASES and view.shape[0] in (S.N_CASES, S.N_CASES + 1) and view.shape[1] == n
    cA = None
    if power:
        P = plan.stft_power(view).cpu().numpy()
        assert P.shape == (view.shape[0], T, cfg["n_fft"] // 2 + 1)
        cA = _worst_of(S.power_error(P[keep], ref), bA, f"{what}: power", "bin")
    lm, mx = plan.logmel(view)
    lm, mx = lm.cpu().numpy(), mx.cpu().numpy()
    assert lm.shape == (view.shape[0], cfg["n_mels"], T)
    lm, mx = lm[keep], mx[keep]
    assert np.isfinite(lm).all() and np.isfinite(mx).all(), f"{what}: log-mel rows not finite"
    cL = _worst_of(S.logmel_error(lm, ref), bL, f"{what}: log-mel", "filter")
    rows_max = lm.reshape(lm.shape[0], -1).max(-1)
    assert np.array_equal(mx, rows_max), f"{what}: clip maximum {mx.tolist()} != maximum of the rows {rows_max.tolist()}"
    return cA, cL, T


class Worst:
    """The largest c_A / c_L over some calls, and which (length, layout) pairs they were."""

    def __init__(self):
        self.cA, self.cL, self.calls = None, 0.0, []

    def add(self, cA, cL, n, layout):
        self.cL = max(self.cL, cL)
        if cA is not None:
            self.cA = max(self.cA or 0.0, cA)
        self.calls.append((n, layout))


def run_path(plan, path, cfg, gpu, power, what):
    """Every length of the configuration in its layouts -> (Worst of the calls `path` took, Worst of those it handed over).
    Asserts that the kernel itself took a partial tile, the 64- and the 65-frame length and a longer batch with the NaN clip."""
    lens, hop = S.lengths(cfg), cfg["hop_length"]
    own, other = Worst(), Worst()
    took = []                                            # (n, frames, NaN clip in the batch) of the calls `path` took
    plan_of = [(n, "layouts" if n == lens[-1] else "plain") for n in lens] + [(n, "aligned") for n in S.aligned_lengths(cfg)]
    for n, kind in plan_of:
        for layout, view, keep, nan_clip in _batches(cfg, n, gpu, kind):
            mine = takes(path, n, view)
            cA, cL, T = check(plan, cfg, n, view, keep, power, f"{what} n {n} {layout}")
            (own if mine else other).add(cA, cL, n, layout)
            if mine:
                took.append((n, T, nan_clip))
    if cfg["n_fft"] <= 2048:
        t64, t65 = plan.cfg.num_frames(63 * hop), plan.cfg.num_frames(64 * hop)     # (an odd n_fft: 63 and 64 frames)
        frames = {T for _, T, _ in took}
        assert t64 in frames and t65 in frames, (what, took)
        assert any(T > t65 and nan for _, T, nan in took), (what, took)
        assert any(3 <= n <= cfg["n_fft"] // 2 + 4 and T < t64 for n, T, _ in took), (what, took)
    else:
        assert any(nan for _, _, nan in took), (what, took)
    return own, other


def note(path, cfg, what, w):
    rA, rL = S.c_ref(cfg)
    bA, bL = S.bounds(cfg)
    a = "-" if w.cA is None else f"{w.cA:.2f}"
    print(f"stage-c path={path} n_fft={cfg['n_fft']} c_A={a} c_L={w.cL:.2f} C_ref={rA:.2f}/{rL:.2f} bound={bA:.2f}/{bL:.2f} "
          f"calls={len(w.calls)} ({what})")


def note_both(path, cfg, what, own, other):
    note(path, cfg, what, own)
    if other.calls:
        note(path + "->handed-over", cfg, what + ": " + " ".join(f"{n}/{layout}" for n, layout in other.calls), other)


# the kernels mm_stft_power_f32 cannot select (choose_kernel, mode 0): their plans' power stage runs on another kernel
NO_POWER_MODE = ("radix16-m12", "radix16-h32")


def run_variants(cfg, gpu, what, expected, power_on=None):
    """Every variant of VARIANTS pinned in turn, duplicates dropped by plan.kernel_path; asserts the paths reached.
    power_on: the paths whose power stage is measured (default: all that have one)."""
    plan = _plan(cfg)
    seen = []
    for variant in VARIANTS:
        with _variant(plan, variant):
            path = plan.kernel_path
            if path in seen:
                continue
            seen.append(path)
            power = path not in NO_POWER_MODE and (power_on is None or path in power_on)
            own, other = run_path(plan, path, cfg, gpu, power, f"{what} {path}")
        note_both(path, cfg, what, own, other)
    assert sorted(seen) == sorted(expected), (what, seen)


REF_DEFAULT = dict(sr=10000, n_fft=512, win_length=250, hop_length=50, n_mels=128, n_mfcc=13, fmin=100.0, fmax=10000.0)
C1, C4, ODD22K = _golden("c1_am"), _golden("c4_am"), _golden("odd_22k")
_ALL7 = ("radix16-m12", "radix16-w16s", "radix16-h32", "radix16-w16", "radix16-w8", "radix16-wpf", "generic")
# pre-emphasis or an odd hop: the direct-load kernels (w16, w8, h32) hand over to the wave-per-frame kernel
_STAGED = ("radix16-m12", "radix16-w16s", "radix16-wpf", "generic")

_TILE512 = {
    "refdefault": (REF_DEFAULT, _ALL7),                                     # half window, staged NR 1, 26 empty filters
    "refdefault+preemph": (dict(REF_DEFAULT, preemph=0.97), _STAGED),       # NR >= 3
    "c1": (C1, _ALL7),                                                      # NR 3
    "hop100": (dict(C1, hop_length=100), _ALL7),                            # NR 2
    # NR 4; a tile's samples fit neither beside m12's power tiles nor in h32's three staging groups
    "hop250": (dict(C1, hop_length=250), ("radix16-w16s", "radix16-w16", "radix16-w8", "radix16-wpf", "generic")),
    "hop161": (dict(C1, hop_length=161), _STAGED),                          # odd hop
    # w8 by default: the 16-way run table does not fit, so no w16 / w16s / m12 / h32 plan; nor a wave-per-frame one
    "mel256": (dict(C1, n_mels=256, fmin=0.0), ("radix16-w8", "generic")),
    "hop300": (dict(C1, hop_length=300), ("radix16-w16", "radix16-w8", "radix16-wpf", "generic")),   # direct loads
    "hop301": (dict(C1, hop_length=301), ("radix16-wpf", "generic")),       # wave per frame at R = 1
}
_TILE512_DEFAULT = {"refdefault": "radix16-w16s", "refdefault+preemph": "radix16-w16s", "c1": "radix16-w16s",
                    "hop100": "radix16-w16s", "hop250": "radix16-w16s", "hop161": "radix16-w16s", "mel256": "radix16-w8",
                    "hop300": "radix16-w16", "hop301": "radix16-wpf"}


@pytest.mark.parametrize("name", sorted(_TILE512))
def test_nfft512_kernels(name, gpu):
    """The n_fft 512 kernels -- m12, w16s (NR 1 .. 4, half window, odd hop, pre-emphasis), h32, w16, w8, wave per frame,
    generic -- in log-mel mode and, where they have one, in power mode."""
    cfg, expected = _TILE512[name]
    plan = _plan(cfg)
    assert plan.kernel_path == _TILE512_DEFAULT[name]
    if name == "mel256":      # no h32 plan without the w16 tables it shares (it read a lane table that was never uploaded)
        with _variant(plan, "h32"):
            assert plan.kernel_path == "radix16-w8"
    run_variants(cfg, gpu, name, expected)


_EMB_ALL = ("radix16-m12", "radix16-w16s", "radix16-h32", "radix16-w16", "radix16-w8", "generic")
_EMB_STAGED = ("radix16-m12", "radix16-w16s", "generic")       # an odd hop: no direct-load kernel
# test_small_nfft_on_the_512_kernels' six: (n_fft, win, hop, sr) -> the paths the variants reach (wave-per-frame has no
# embedded form: that variant stays on w16s)
_EMBEDDED = [((256, 200, 80, 8000), _EMB_ALL), ((256, 256, 64, 8000), _EMB_ALL), ((128, 100, 25, 8000), _EMB_STAGED),
             ((64, 64, 16, 8000), _EMB_ALL), ((256, 250, 50, 10000), _EMB_ALL), ((256, 201, 77, 16000), _EMB_STAGED)]


@pytest.mark.parametrize("shape,expected", _EMBEDDED, ids=[f"nfft{c[0][0]}-hop{c[0][2]}" for c in _EMBEDDED])
def test_embedded_small_nfft(shape, expected, gpu):
    """n_fft 64 / 128 / 256 embedded in the 512-point tile kernels: log-mel on the tile kernel (every variant the plan has),
    power on the generic kernel whatever variant is pinned (the only one with n_fft / 2 + 1 bins per row): measured there."""
    n_fft, win, hop, sr = shape
    cfg = dict(sr=sr, n_fft=n_fft, win_length=win, hop_length=hop, n_mels=min(40, n_fft // 4), n_mfcc=13 if n_fft > 64 else 8,
               fmin=50.0, fmax=sr / 2)
    assert _plan(cfg).kernel_path == "radix16-w16s"
    run_variants(cfg, gpu, f"embedded win {win} hop {hop}", expected, power_on=("generic",))


_WPF = [(kw, what) for kw, what in _HALFBAND_CFGS] + [
    (C4, "c4"), (ODD22K, "odd_22k"), (dict(C4, preemph=0.97), "c4 + pre-emphasis"), (dict(ODD22K, preemph=0.97), "odd_22k + pre-emphasis"),
    (dict(C4, hop_length=481), "c4, hop 481"), (dict(ODD22K, hop_length=221), "odd_22k, hop 221")]


@pytest.mark.parametrize("cfg,what", _WPF, ids=[f"wpf{i}" for i in range(len(_WPF))])
def test_wave_per_frame_kernels(cfg, what, gpu):
    """n_fft 1024 / 2048: the full, input-pruned (z) and output-pruned (half, 4 .. 7 pairs) instantiations in log-mel mode,
    the full kernel in power mode, with pre-emphasis and odd hops."""
    plan = _plan(cfg)
    assert plan.kernel_path == "radix16-wpf"
    note_both("radix16-wpf", cfg, what, *run_path(plan, "radix16-wpf", cfg, gpu, True, what))


@pytest.mark.parametrize("cfg,what", _ANY_NFFT, ids=[f"nfft{c[0]['n_fft']}_{i}" for i, c in enumerate(_ANY_NFFT)])
def test_any_length_kernels(cfg, what, gpu):
    """Every n_fft that is not a power of two in [32, 4096]: mixed radix, two register stages, Bluestein, one wave or one
    workgroup per frame."""
    plan = _plan(cfg)
    assert plan.kernel_path == "any-length"
    note_both("any-length", cfg, what, *run_path(plan, "any-length", cfg, gpu, True, what))


_FORMS = [(kw, what) for kw, what in _ANY_NFFT if kw["n_fft"] in (400, 800)]


@pytest.mark.parametrize("cfg,what", _FORMS, ids=[f"nfft{c[0]['n_fft']}_{i}" for i, c in enumerate(_FORMS)])
def test_any_length_forms(cfg, what, gpu):
    """n_fft 400 / 800: the forms set_variant selects on an any-length plan (launch_any).  The default of all five plans is
    the two-register-stage kernel (n_fft / 2 = 200 = 8 x 25 and 400 = 16 x 25 complex points); form 1 is the one-frame-per-
    wave kernel.  Forms 2 .. 4 are stft_anyb_kernel with that many frames per batch only where the plan has a batched form
    (setup_any: n_fft / 2 <= 256 complex points with the tables in LDS, so the n_fft 400 plans); on the n_fft 800 plans they
    select what form 1 selects.  Nothing the C ABI returns tells the forms apart, so this test cannot see which one ran: it
    holds whatever each setting runs to the bound."""
    assert len(_FORMS) == 5
    plan = _plan(cfg)
    assert plan.kernel_path == "any-length"
    for form in (1, 2, 3, 4):
        old = plan.set_variant(form)
        try:
            own, other = run_path(plan, "any-length", cfg, gpu, True, f"{what} form {form}")
        finally:
            plan.set_variant(old)
        note_both(f"any-length/form{form}", cfg, what, own, other)


_GENERIC = {
    "nfft32": (dict(sr=8000, n_fft=32, win_length=32, hop_length=8, n_mels=8, n_mfcc=4, fmin=0.0, fmax=4000.0), False),
    "nfft4096": (dict(sr=16000, n_fft=4096, win_length=2000, hop_length=500, n_mels=64, n_mfcc=13, fmin=0.0, fmax=8000.0), False),
    "c1": (C1, True), "odd_22k": (ODD22K, True), "c4": (C4, True),
}


@pytest.mark.parametrize("name", sorted(_GENERIC))
def test_generic_power_of_two_kernel(name, gpu):
    """stft_generic_kernel: the lengths no other kernel takes (32, 4096) and, forced, n_fft 512 / 1024 / 2048."""
    cfg, force = _GENERIC[name]
    plan = _plan(cfg)
    with _variant(plan, "generic" if force else "auto"):
        assert plan.kernel_path == "generic"
        own, other = run_path(plan, "generic", cfg, gpu, True, f"generic {name}")
    note_both("generic", cfg, name, own, other)
