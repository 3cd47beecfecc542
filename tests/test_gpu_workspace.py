"""The workspace contract of the C ABI (DESIGN.md "Workspace contract") for every compute entry that takes a
``(void* ws, size_t bytes)`` pair: exactly ``*_workspace_bytes`` bytes suffice, what the workspace held before the call
never reaches a result, and nothing outside it is written.  The instrument is tests/ws_arena.py: the entry gets exactly the
bytes its sizer named, between two 256 KiB guards, every byte of the arena set to 0x00, 0xFF or 0x7F before the call.

A. every case of tests/stream_cases.py and of the STREAM_CASES lists of the zoom, Lomb-Scargle, Welch and spline test
   files, eager, on both data sets: under each pattern the guards must be intact and every output bit for bit what the
   same call gives with nothing redirected (the eager results of the stream sessions).
B. the MFCC workspace on every kernel instantiation of tests/test_gpu_stages.py (its configuration lists, the forced
   variants included): plan.mfcc, plan.logmel and plan.mfcc_modspec of a three-clip batch of two tiles.
C. the harness is seen to work: stand-in "entries" in pure torch on our own arena that write a byte behind and in front
   of their workspace, return the sum of a workspace they never wrote, or allocate their scratch past the redirect.

Every test prints the entry, the number of arenas handed out and their sizes (-s); docs/experiments.md holds one run.
Nothing here is captured into a graph, and nothing probes a misaligned or undersized workspace: the refusals are tested
elsewhere, and every stray write this harness can show lands inside memory the test owns."""
import contextlib

import numpy as np
import pytest

import stream_cases as S
import test_gpu_lomb
import test_gpu_modcsd
import test_gpu_modpsd
import test_gpu_spline
import test_gpu_stages as ST
import test_gpu_streams as TS
import test_gpu_zoom
import test_workspace_host as WH
import ws_arena as W
from test_gpu_parity import _plan, _variant

pytestmark = pytest.mark.gpu

_OWN_SESSION = (test_gpu_zoom, test_gpu_lomb, test_gpu_modpsd, test_gpu_modcsd, test_gpu_spline)
ALL_CASES = list(S.CASES) + [c for mod in _OWN_SESSION for c in mod.STREAM_CASES]
assert [c.name for c in ALL_CASES] == [c.name for c in WH.all_cases()]


def eager_entry(case, gpu):
    """The case's entry of the stream session it belongs to (made here if that session's own tests have not run): its
    eager results on both data sets with nothing redirected."""
    mod = next((m for m in _OWN_SESSION if case in m.STREAM_CASES), None)
    if mod is None:
        if not TS._SESSION:
            TS._SESSION.append(TS.Session(gpu))
        return TS._SESSION[0].get(case)
    if not mod._SESSION:
        mod._SESSION.append(TS.Session(gpu, cases=mod.STREAM_CASES))
    return mod._SESSION[0].get(case)


def run_redirected(case, gpu, fill, monkeypatch):
    """The case prepared under redirect() with arenas of ``fill``; on each data set: fill(k), outputs poisoned as in the
    eager run, every arena poisoned again, the call, clones, the guards checked -> ({k: clones}, arena sizes, sizer log)."""
    import torch
    arenas = W.Arenas(gpu, fill)
    got = {}
    with monkeypatch.context() as m:
        W.redirect(m, arenas)
        p = case.prepare(gpu)
        for k in (1, 0):
            p.fill(k)
            p.poison()
            arenas.refill()
            got[k] = TS._clones(p.call())
            torch.cuda.synchronize()
            arenas.check(f"{case.name}, pattern 0x{fill:02X}, data set {k}")
    arenas.check_handed_out(f"{case.name}, pattern 0x{fill:02X}")
    sizes, sized = arenas.sizes, list(arenas.sized)
    arenas.close()
    return got, sizes, sized


_HANDED = {}      # case name -> arena sizes (the same under every pattern)


def hold(case, gpu, monkeypatch):
    e = eager_entry(case, gpu)
    host = case.data()
    monkeypatch.setattr(case, "data", lambda: host)            # (made once, staged once per pattern)
    seen = []
    for fill in W.PATTERNS:
        got, sizes, sized = run_redirected(case, gpu, fill, monkeypatch)
        for k in (1, 0):
            TS.assert_same(case, got[k], e.eager[k], f"workspace of 0x{fill:02X}, data set {k}", e.exact())
        seen.append(sizes)
    assert seen[0] == seen[1] == seen[2], (case.name, seen)
    _HANDED[case.name] = seen[0]
    print(f"\nworkspace {case.name}: entry {case.entry}, {len(seen[0])} arenas, bytes {seen[0]}")
    return seen[0]


# ---- A. every registry case -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ALL_CASES, ids=lambda c: c.name)
def test_poisoned_guarded_workspace(case, gpu, monkeypatch):
    assert case.tol is None
    hold(case, gpu, monkeypatch)


def test_every_workspace_entry_was_handed_an_arena(gpu, monkeypatch):
    """Every entry whose prototype has a workspace size parameter has a case in A in which an arena of more than 0 bytes
    was handed out (the one legitimate zero, a Welch call without a second launch, is covered by another case of its
    entry).  Cases A has not run in this process are run here."""
    entries = WH.workspace_entries()
    assert len(entries) == 30
    for case in ALL_CASES:
        if case.entry in entries and case.name not in _HANDED:
            hold(case, gpu, monkeypatch)
    for entry in entries:
        best = max((max(_HANDED[c.name], default=0), c.name) for c in ALL_CASES if c.entry == entry)
        assert best[0] > 0, f"{entry}: no case handed it a workspace of more than 0 bytes"
        print(f"workspace entry {entry}: up to {best[0]} bytes ({best[1]})")


# ---- B. the MFCC workspace on every kernel instantiation ------------------------------------------------------------------------
def _short(path):
    return path[len("radix16-"):] if path.startswith("radix16-") else path


def _instantiations():
    """(id, configuration, pin, the kernel_path it must reach) for every instantiation of tests/test_gpu_stages.py.  pin:
    ("variant", name) as run_variants pins it, ("form", k) as test_any_length_forms does, or None."""
    out = []
    for name in sorted(ST._TILE512):
        cfg, paths = ST._TILE512[name]
        out += [(f"tile512-{name}-{_short(p)}", cfg, ("variant", _short(p)), p) for p in paths]
    for (n_fft, win, hop, sr), paths in ST._EMBEDDED:           # the configuration test_embedded_small_nfft builds
        cfg = dict(sr=sr, n_fft=n_fft, win_length=win, hop_length=hop, n_mels=min(40, n_fft // 4), n_mfcc=13 if n_fft > 64 else 8,
                   fmin=50.0, fmax=sr / 2)
        out += [(f"embedded-nfft{n_fft}-hop{hop}-{_short(p)}", cfg, ("variant", _short(p)), p) for p in paths]
    out += [(f"wpf{i}", cfg, None, "radix16-wpf") for i, (cfg, _) in enumerate(ST._WPF)]
    out += [(f"any-nfft{cfg['n_fft']}_{i}", cfg, None, "any-length") for i, (cfg, _) in enumerate(ST._ANY_NFFT)]
    out += [(f"any-nfft{cfg['n_fft']}_{i}-form{k}", cfg, ("form", k), "any-length") for i, (cfg, _) in enumerate(ST._FORMS)
            for k in (1, 2, 3, 4)]
    out += [(f"generic-{name}", ST._GENERIC[name][0], ("variant", "generic" if ST._GENERIC[name][1] else "auto"), "generic")
            for name in sorted(ST._GENERIC)]
    return out


INSTANTIATIONS = _instantiations()
assert len({i[0] for i in INSTANTIATIONS}) == len(INSTANTIATIONS)


@contextlib.contextmanager
def _pinned(plan, pin):
    if pin is None:
        yield
    elif pin[0] == "variant":
        with _variant(plan, pin[1]):
            yield
    else:
        old = plan.set_variant(pin[1])
        try:
            yield
        finally:
            plan.set_variant(old)


def three_clips(cfg, n):
    """[3, n] float32: a full-scale clip (a tone inside the mel bank plus noise, its peak at 1.0); the same clip 60 dB down
    with digital silence in its second half; digital silence."""
    rng = np.random.default_rng(n)
    t = np.arange(n) / cfg["sr"]
    x = 0.5 * np.sin(2 * np.pi * (cfg["fmin"] + 0.3 * (cfg["fmax"] - cfg["fmin"])) * t) + 0.5 * rng.uniform(-1, 1, n)
    x /= np.abs(x).max()
    quiet = 1e-3 * x
    quiet[n // 2:] = 0.0
    return np.stack([x, quiet, np.zeros(n)]).astype(np.float32)


def _front(plan, x):
    lm, mx = plan.logmel(x)
    mfcc2, mod = plan.mfcc_modspec(x)
    return [plan.mfcc(x), lm, mx, mfcc2, mod]


@pytest.mark.parametrize("what,cfg,pin,path", INSTANTIATIONS, ids=[i[0] for i in INSTANTIATIONS])
def test_mfcc_workspace_on_every_instantiation(what, cfg, pin, path, gpu, monkeypatch):
    """plan.mfcc, plan.logmel and plan.mfcc_modspec (one launch where the plan fuses it, mfcc and modspec otherwise) of
    three clips of the shortest length that gives two tiles on the path -- 65 frames, 33 on the 32-frame kernel --, with the
    workspace in a poisoned arena, against the same calls on the plan's own workspace.  The quiet clip's own key decides
    its result: its maximum lies 60 dB under its neighbour's, so a stale or unset key (0x00 is the key of 0 dB, 0x7F of
    3.39e38) moves its clamp and the silent clip's and not the loud one's.  Whether its own clamp is active in the right
    result is printed: with amin 1e-10 the silence lies at -100 dB, and an 80 dB clamp then needs a maximum above -20 dB."""
    import torch
    plan = _plan(cfg)
    tile = 32 if path == "radix16-h32" else 64
    n = tile * cfg["hop_length"]
    while plan.cfg.num_frames(n) < tile + 1:
        n += 1
    assert plan.cfg.num_frames(n) == tile + 1
    x = torch.from_numpy(three_clips(cfg, n)).to(gpu)
    with _pinned(plan, pin):
        assert plan.kernel_path == path, (what, plan.kernel_path)
        assert ST.takes(path, n, x), (what, n)
        want = TS._clones(_front(plan, x))
        torch.cuda.synchronize()
        lm, mx = want[1], want[2]
        # (a bank that sees none of the power -- n_fft 2: one filter whose weights vanish on both bins -- is at the floor thrice)
        assert bool(torch.isfinite(want[0]).all()) and float(mx[2]) <= float(mx[1]) <= float(mx[0])
        assert float(mx[1]) < float(mx[0]) - 55.0 or float(mx[0]) < float(mx[2]) + 65.0, mx.tolist()
        clamps = float(lm[1].min()) < float(mx[1]) - float(cfg.get("top_db", 80.0))
        sizes = None
        for fill in W.PATTERNS:
            arenas = W.Arenas(gpu, fill)
            with monkeypatch.context() as m:
                W.redirect(m, arenas)
                got = TS._clones(_front(plan, x))
                torch.cuda.synchronize()
            arenas.check(f"{what}, pattern 0x{fill:02X}")
            arenas.check_handed_out(f"{what}, pattern 0x{fill:02X}")
            for name, g, w in zip(("mfcc", "logmel", "clip maximum", "mfcc of mfcc_modspec", "modspec"), got, want):
                if not TS.bit_equal(g, w):
                    bad = (TS._bits(g) != TS._bits(w)).reshape(g.shape[0], -1).sum(1).tolist()
                    raise AssertionError(f"{what} ({path}): {name} with a workspace of 0x{fill:02X} differs from the call on the "
                                         f"plan's own workspace; differing bytes per clip {bad}")
            assert sizes in (None, arenas.sizes)
            sizes = arenas.sizes
            arenas.close()
        assert len(sizes) == 2 and sizes[0] == sizes[1] > 0, sizes         # mm_mfcc_f32 and mm_mfcc_modspec_f32
    print(f"\nworkspace {what}: path {path}, n {n}, entries mm_mfcc_f32 + mm_mfcc_modspec_f32, {len(sizes)} arenas, bytes {sizes}, "
          f"quiet clip clamps: {clamps}")


# ---- C. the harness must be seen to work ----------------------------------------------------------------------------------------
def _stand_in(name, setup):
    def data():
        r = np.random.default_rng(5)
        return {"x": (r.standard_normal(4096).astype(np.float32), r.standard_normal(4096).astype(np.float32))}
    return S.Case(name, "stand-in", "self-check", data, setup)


def _stray_writer(offset_from_start):
    """An "entry" that doubles its input and writes one byte at ws[offset] THROUGH THE BASE TENSOR of its arena."""
    import torch

    def setup(env):
        out = env.out((4096,), torch.float32)
        ws = env.work(1000)

        def call():
            out.copy_(env.buf["x"] * 2)
            base = ws._base
            assert base is not None and base.numel() == 2 * W.GUARD + 1024 and ws.storage_offset() == W.GUARD
            base[W.GUARD + offset_from_start] = 0x55
            return out
        return call
    return setup


@pytest.mark.parametrize("fill", W.PATTERNS)
def test_harness_sees_a_byte_written_at_ws_nbytes(fill, gpu, monkeypatch):
    with pytest.raises(AssertionError, match=r"1000-byte workspace.*offset \+0 from its end"):
        run_redirected(_stand_in(f"self-check/overrun-{fill}", _stray_writer(1000)), gpu, fill, monkeypatch)


@pytest.mark.parametrize("fill", W.PATTERNS)
def test_harness_sees_a_byte_written_at_ws_minus_1(fill, gpu, monkeypatch):
    with pytest.raises(AssertionError, match=r"1000-byte workspace.*offset -1 from its start"):
        run_redirected(_stand_in(f"self-check/underrun-{fill}", _stray_writer(-1)), gpu, fill, monkeypatch)


def test_harness_passes_an_entry_that_keeps_to_its_workspace(gpu, monkeypatch):
    got, sizes, _ = run_redirected(_stand_in("self-check/in-bounds", _stray_writer(999)), gpu, 0x7F, monkeypatch)
    assert sizes == [1000] and len(got[0]) == 1


def test_harness_sees_a_result_made_of_unwritten_workspace(gpu, monkeypatch):
    """An "entry" that adds the sum of a workspace it never wrote to its output: every pair of patterns must differ."""
    import torch

    def setup(env):
        out = env.out((4096,), torch.float32)
        ws = env.work(4096)

        def call():
            out.copy_(env.buf["x"] + ws.view(torch.int32).sum().to(torch.float32))
            return out
        return call
    case = _stand_in("self-check/reads-unwritten", setup)
    got = {fill: run_redirected(case, gpu, fill, monkeypatch)[0] for fill in W.PATTERNS}
    for a, b in ((0x00, 0xFF), (0x00, 0x7F), (0xFF, 0x7F)):
        with pytest.raises(AssertionError, match="differs from the eager call"):
            TS.assert_same(case, got[a][1], got[b][1], f"0x{a:02X} against 0x{b:02X}")
    TS.assert_same(case, got[0x7F][1], run_redirected(case, gpu, 0x7F, monkeypatch)[0][1], "the same pattern twice")


def test_harness_sees_a_wrapper_that_allocates_past_the_redirect(gpu, monkeypatch):
    """A "wrapper" that asks a sizer of the library and then allocates the scratch itself: no arena was handed out although
    the sizer was positive."""
    import torch

    def setup(env):
        from modulation_mfcc_amd import _lib
        out = env.out((4096,), torch.float32)

        def call():
            need = _lib.load().mm_sosfiltfilt_workspace_bytes(4, 1100)
            assert need > 0
            own = torch.empty(need, dtype=torch.uint8, device=env.gpu)
            out.copy_(env.buf["x"] * 2 + own.numel())
            return out
        return call
    with pytest.raises(AssertionError, match=r"mm_sosfiltfilt_workspace_bytes.*no workspace was taken from the arenas"):
        run_redirected(_stand_in("self-check/own-scratch", setup), gpu, 0x00, monkeypatch)
