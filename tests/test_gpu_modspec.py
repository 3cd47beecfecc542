"""GPU (-m gpu): the modulation spectrum (row A8) bin by bin on every transform path.

Every check is modspec_oracle.check: the per-bin error against np.fft.rfft in float64 OF THE ROWS THE DEVICE TRANSFORMED (for
the end-to-end calls the MFCC tensor the same call returned, so the transform's error is apart from the MFCC's), normalised
by the row's own norm, at most MARGIN x max(C_ref(n), 1) -- C_ref from scipy's float32 transform of the case rows, computed on
the host.  The paths: rfft16_kernel<1|2, FAST|masked>, rfft_wpf_kernel<4, FAST|masked>, rfft_generic_kernel, the transforms
inside the clip-mode launch (s16_fin_modspec<1|2>, s16_fin_modspec_2k), the long transform in global memory and the ragged
call.  Each test prints the largest c it saw per path and length ("modspec-c ..." lines, shown with -s): docs/experiments.md
holds the table."""
import numpy as np
import pytest

import mfcc_oracle as O
import modspec_oracle as M
from conftest import load_golden

pytestmark = pytest.mark.gpu

REF_DEFAULT = dict(sr=10000, n_fft=512, win_length=250, hop_length=50, n_mels=128, n_mfcc=13, fmin=100.0, fmax=10000.0)
KINDS = ("am", "quiet_tail", "noise", "silence", "impulse")


def _c1():
    return load_golden("c1_am")[0]


def _plan(kw, **extra):
    from modulation_mfcc_amd import MfccConfig, get_plan
    return get_plan(MfccConfig(**{**kw, **extra}))


def _dev(x, gpu):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).to(gpu)


def _note(path, n, c):
    print(f"modspec-c path={path} n={n} c={c:.2f} C_ref={M.c_ref(n):.2f} bound={M.tolerance(n):.2f}")


def _layouts(x, gpu):
    """(name, device view of x): contiguous; odd row pitch; even pitch starting one float into the buffer.  What lies between
    the rows is NaN: a sample taken from there shows in every bin."""
    import torch
    R, L = x.shape
    xd = _dev(x, gpu)
    yield "contiguous", xd
    odd = torch.full((R, (L + 2) | 1), float("nan"), dtype=torch.float32, device=gpu)
    odd[:, :L] = xd
    assert odd.stride(0) % 2 == 1
    yield "odd-pitch", odd[:, :L]
    off = torch.full((R, (L + 3) & ~1), float("nan"), dtype=torch.float32, device=gpu)
    off[:, 1:1 + L] = xd
    view = off[:, 1:1 + L]
    assert view.stride(0) % 2 == 0 and view.data_ptr() % 8 == 4
    yield "offset", view


def _rfft_path(n, L, layout, generic):
    if generic or n not in (512, 1024, 2048):
        return "generic"
    return ("rfft16" if n < 2048 else "wpf") + (" FAST" if L == n and layout == "contiguous" else " masked")


@pytest.mark.parametrize("n,generic", [(n, False) for n in (32, 64, 128, 256, 512, 1024, 2048, 4096, 8192)] +
                         [(n, True) for n in (512, 1024, 2048)],
                         ids=lambda v: ("generic" if v else "auto") if isinstance(v, bool) else str(v))
def test_rfft_stage(n, generic, gpu):
    """plan.rfft at every zero-padding edge, 1 / 5 / 37 rows (partial row groups, partial waves), three row layouts; the
    1e-6-scaled row between the 1e3-scaled one and the mean-1e4 one is held to its own norm."""
    plan = _plan(_c1())
    worst = {}
    plan.force_generic(generic)
    try:
        for L in M.edge_lengths(n):
            rows_all = M.cases(n, L)
            for R in (1, 5, 37):
                x = M.take(rows_all, R)
                for layout, view in _layouts(x, gpu):
                    got = plan.rfft(view, n)
                    assert tuple(got.shape) == (R, n // 2 + 1)
                    c = M.check(got.cpu().numpy(), x, n, f"rfft n {n} L {L} rows {R} {layout}")
                    path = _rfft_path(n, L, layout, generic)
                    worst[path] = max(worst.get(path, 0.0), c)
    finally:
        plan.force_generic(False)
    for path, c in sorted(worst.items()):
        _note(path, n, c)


def _trajectories(n, T, B, n_mfcc):
    return M.take(M.cases(n, T), B * n_mfcc).reshape(B, n_mfcc, T)


_MODSPEC_PLANS = {2: dict(n_mfcc=2), 13: dict(), 16: dict(n_mfcc=16), 20: dict(n_mfcc=20, n_mels=64)}


@pytest.mark.parametrize("T", [1, 31, 32, 33, 257, 511, 512, 513, 1023, 1024, 1025, 2047, 2048, 2049, 4096, 4097, 8191, 8192])
def test_modspec_at_both_edges_of_every_length(T, gpu):
    """plan.modspec of [3, n_mfcc, T] trajectories built from the case rows, n_mfcc 2 / 13 / 16 / 20 (row counts that fill
    neither the row groups nor the waves)."""
    for n_mfcc, extra in _MODSPEC_PLANS.items():
        plan = _plan(_c1(), **extra)
        assert plan.cfg.n_mfcc == n_mfcc
        n = plan.cfg.mod_fft_len(T)
        assert n == max(32, 1 << (T - 1).bit_length())
        x = _trajectories(n, T, 3, n_mfcc)
        got = plan.modspec(_dev(x, gpu))
        assert tuple(got.shape) == (3, n_mfcc, n // 2 + 1)
        c = M.check(got.cpu().numpy(), x, n, f"modspec T {T} n_mfcc {n_mfcc}")
        _note(f"modspec({_rfft_path(n, T, 'contiguous', False)}) T={T} n_mfcc={n_mfcc}", n, c)


def _clips(n, sr, count, gpu, first_seed=700):
    """[count, n] on the device: ten synthetic clips (two of every kind) repeated, every clip b with b % 7 in (2, 5) scaled by
    1e-3 -- neighbouring clips' trajectories differ in scale and kind."""
    import torch
    base = _dev(np.stack([O.synth_clip(first_seed + i, n, sr, KINDS[i % 5]) for i in range(10)]), gpu)
    b = torch.arange(count, device=gpu)
    scale = torch.where((b % 7 == 2) | (b % 7 == 5), 1e-3, 1.0).to(torch.float32)
    return base[b % 10] * scale[:, None]


@pytest.mark.parametrize("n_mod,T", [(32, 5), (32, 32), (1024, 301), (2048, 301), (8192, 100), (16384, 1001)])
def test_user_set_n_mod_fft(n_mod, T, gpu):
    """MfccConfig.n_mod_fft: T << n_mod through every transform, from modspec() on the case rows and from mfcc_modspec() on
    audio of the matching length."""
    import torch
    kw = _c1()
    plan = _plan(kw, n_mod_fft=n_mod)
    assert plan.cfg.mod_fft_len(T) == n_mod
    x = _trajectories(n_mod, T, 3, 13)
    got = plan.modspec(_dev(x, gpu))
    assert tuple(got.shape) == (3, 13, n_mod // 2 + 1)
    c = M.check(got.cpu().numpy(), x, n_mod, f"modspec n_mod_fft {n_mod} T {T}")
    _note(f"modspec n_mod_fft T={T}", n_mod, c)
    n = (T - 1) * kw["hop_length"]
    assert plan.cfg.num_frames(n) == T
    audio = _clips(n, kw["sr"], 5, gpu)
    m, s = plan.mfcc_modspec(audio)
    assert tuple(m.shape) == (5, 13, T) and tuple(s.shape) == (5, 13, n_mod // 2 + 1)
    assert torch.equal(m, plan.mfcc(audio))
    c = M.check(s.cpu().numpy(), m.cpu().numpy(), n_mod, f"mfcc_modspec n_mod_fft {n_mod} T {T}")
    _note(f"mfcc_modspec n_mod_fft T={T}", n_mod, c)


def test_n_mod_fft_shorter_than_the_trajectory_is_refused(gpu):
    import torch
    kw = _c1()
    plan = _plan(kw, n_mod_fft=32)
    with pytest.raises(ValueError):
        plan.cfg.mod_fft_len(33)
    canary = torch.full((1, 13, 17), 7.0, dtype=torch.complex64, device=gpu)
    with pytest.raises(ValueError):
        plan.modspec(torch.zeros((1, 13, 33), device=gpu), out=canary)
    audio = torch.zeros((1, 32 * kw["hop_length"]), device=gpu)
    assert plan.cfg.num_frames(audio.shape[1]) == 33
    with pytest.raises(ValueError):
        plan.mfcc_modspec(audio, out_mod=canary)
    assert bool((canary == 7.0).all())                   # refused before any launch
    assert plan.modspec(torch.zeros((1, 13, 32), device=gpu)).shape == (1, 13, 17)


def _clip_mode(plan, T, hop, sr, n_mod, wide, gpu):
    import torch
    B, n = 256, (T - 1) * hop
    assert plan.cfg.num_frames(n) == T and plan.cfg.mod_fft_len(T) == n_mod
    audio = _clips(n, sr, B, gpu)
    prev = plan.set_fuse_tail(False)
    try:
        assert not plan.fused_tail(B, n)
        m0, s0 = plan.mfcc_modspec(audio)
        plan.set_fuse_tail(2 if wide else True)
        assert plan.kernel_path == "radix16-w16s" and plan.fused_dct and plan.fused_tail(B, n)
        m1, s1 = plan.mfcc_modspec(audio)
    finally:
        plan.set_fuse_tail(prev)
    assert tuple(m1.shape) == (B, plan.cfg.n_mfcc, T) and tuple(s1.shape) == (B, plan.cfg.n_mfcc, n_mod // 2 + 1)
    assert torch.equal(m1, m0), float((m1 - m0).abs().max())
    # the clamp fix-up ran (quiet_tail clips) and neighbouring clips differ in scale
    lm, mx = plan.logmel(audio[1:2])
    assert float(lm.min()) < float(mx[0]) - 80.0
    mh = m1.cpu().numpy()                                # every clip and row, moved once
    assert np.isfinite(mh).all()
    c1 = M.check(s1.cpu().numpy(), mh, n_mod, f"clip mode T {T}")
    c0 = M.check(s0.cpu().numpy(), mh, n_mod, f"separate launches T {T}")
    return c1, c0


@pytest.mark.parametrize("T", [257, 511, 512, 513, 1023, 1024])
def test_clip_mode(T, gpu):
    """mm_mfcc_modspec_f32 as ONE launch on the c1 configuration: 256 clips (one per workgroup) of the shortest length that
    gives T frames; every row of every clip against the float64 transform of the MFCC the same call returned."""
    kw = _c1()
    n_mod = 512 if T <= 512 else 1024
    c1, c0 = _clip_mode(_plan(kw), T, kw["hop_length"], kw["sr"], n_mod, False, gpu)
    _note(f"fused {n_mod} T={T}", n_mod, c1)
    _note(f"rfft16 masked (MFCC rows) T={T}", n_mod, c0)


@pytest.mark.parametrize("T", [1025, 2047, 2048])
def test_clip_mode_2048(T, gpu):
    """The reference's default call (10 kHz, hop 50, 128 mel) under set_fuse_tail(2): s16_fin_modspec_2k."""
    c1, c0 = _clip_mode(_plan(REF_DEFAULT), T, 50, 10000, 2048, True, gpu)
    _note(f"fused 2048 T={T}", 2048, c1)
    _note(f"wpf {'FAST' if T == 2048 else 'masked'} (MFCC rows) T={T}", 2048, c0)


def test_clip_mode_with_a_user_set_length(gpu):
    """n_mod_fft = 1024 on 301 frames in clip mode: the in-kernel transform loads far past every row and masks by e < T."""
    kw = _c1()
    c1, c0 = _clip_mode(_plan(kw, n_mod_fft=1024), 301, kw["hop_length"], kw["sr"], 1024, False, gpu)
    _note("fused 1024 n_mod_fft T=301", 1024, c1)
    _note("rfft16 masked (MFCC rows) n_mod_fft T=301", 1024, c0)


@pytest.mark.parametrize("n,lengths", [(16384, (8193, 12000, 16383, 16384)), (32768, (20001,)), (65536, (40001,))],
                         ids=["16384", "32768", "65536"])
def test_long_path(n, lengths, gpu):
    """calc.rfft_rows_long (the transform in global memory; 8193 = 16384 / 2 + 1) on the case rows, the batch cut into chunks of seven rows, and
    modspec() of trajectories with more than 8192 frames, which hands over to it."""
    from modulation_mfcc_amd import _lib, calc
    plan = _plan(_c1())
    hp = calc._hilbert_plan(n, 0, gpu)
    per_row = int(_lib.load().mm_hilbert_rfft_workspace_bytes(hp.h, 1))
    old = calc.HILBERT_WS_BYTES
    try:
        calc.HILBERT_WS_BYTES = 7 * per_row
        for T in lengths:
            x = M.take(M.cases(n, T), 37)
            got = calc.rfft_rows_long(_dev(x, gpu), n)
            assert tuple(got.shape) == (37, n // 2 + 1)
            _note(f"long rfft_rows_long T={T}", n, M.check(got.cpu().numpy(), x, n, f"rfft_rows_long n {n} T {T}"))
            assert plan.cfg.mod_fft_len(T) == n
            x = _trajectories(n, T, 2, 13)
            got = plan.modspec(_dev(x, gpu))
            assert tuple(got.shape) == (2, 13, n // 2 + 1)
            _note(f"long modspec T={T}", n, M.check(got.cpu().numpy(), x, n, f"modspec n {n} T {T}"))
    finally:
        calc.HILBERT_WS_BYTES = old


def test_ragged(gpu):
    """mfcc_modspec_ragged: lengths from one frame to T_max = 601 (n_mod 1024), per-clip scales, NaN behind every clip; every
    clip's rows against the float64 transform of its own valid frames."""
    import torch
    kw = _c1()
    plan = _plan(kw)
    hop = kw["hop_length"]
    n_max = 600 * hop
    lengths = (1, hop - 1, hop, 5000, 256 * hop, 300 * hop + 7, 512 * hop, n_max)
    audio = _clips(n_max, kw["sr"], len(lengths), gpu, first_seed=720).clone()
    for b, L in enumerate(lengths):
        audio[b, L:] = float("nan")
    out, mod, frames = plan.mfcc_modspec_ragged(audio, list(lengths))
    n_mod = plan.cfg.mod_fft_len(plan.cfg.num_frames(n_max))
    assert n_mod == 1024 and tuple(mod.shape) == (len(lengths), 13, 513)
    fr = frames.cpu().numpy().tolist()
    assert fr == [plan.cfg.num_frames(L) for L in lengths] and fr[0] == 1 and fr[-1] == 601
    oh, mh = out.cpu().numpy(), mod.cpu().numpy()
    worst = 0.0
    for b, T_b in enumerate(fr):
        assert np.isfinite(oh[b]).all() and (oh[b, :, T_b:] == 0).all()
        worst = max(worst, M.check(mh[b], np.ascontiguousarray(oh[b, :, :T_b]), n_mod, f"ragged clip {b} ({T_b} frames)"))
    _note("ragged", n_mod, worst)
