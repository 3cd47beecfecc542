"""GPU (-m gpu): the top_db clamp + DCT-II stage (row A6) coefficient by coefficient on every kernel form the library has.

Every check is dct_oracle's: |MFCC - M| against the float64 reference of the same clips, normalised by the frame's and the
coefficient's own floor, at most MARGIN x max(C_ref[k], 1) per coefficient index k -- C_ref[k] from the float32 host pipelines
over the case set at the lengths of dct_oracle.frame_lengths (1, 2, 15, 16, 17, 63, 64, 65, 255, 256, 257 frames: the 16-, 64-
and 256-frame tiles of the kernels, one fewer and one more), computed on the host.  The 14 case clips go in one batch (clip
boundaries fall inside tiles), clips that clamp beside clips that do not; at the longest length in three row layouts with NaN
between the rows and one all-NaN clip in the middle of the batch, whose neighbours must stay finite and inside the bound;
for the kernel with an alignment gate (h32) in the aligned layout at every length.  top_db is 80, 40 and -1 (no clamp)
throughout.

The forms (dct_form restates the selection rules of mm_mfcc_f32 / setup_wpf / mm_mfcc_ragged_f32):

  1    dct_clamp_kernel: lane <-> frame, 256 frames per block, sixteen coefficients per accumulator block
  2    the DCT inside the log-mel launch of w16s / m12 (n_mfcc <= 16) + dct_fixup_kernel (mm_clamp_corr)
  3    the same with dct_fixup_kernel's empty-filter add branch (plans with empty mel filters, w16s: every clip takes it)
  4    clip mode: whole clips per workgroup, s16_fix_clip and the empty filters' add inside the launch
  5    dct_clamp_fm_wave_kernel<10, 5, false>      6    <10, 8, true>      7    <8, 8, true>
  8/KB dct_clamp_fm_kernel<KB>, KB in 4, 8, 10, 12, 16 (VALU, 64-frame tiles)
  9    ragged_clamp_dct_kernel

What the C ABI reports is asserted: kernel_path (which log-mel kernel feeds the stage), fused_dct (forms 2 - 4 against 1) and
fused_tail (form 4).  What it does not report and this file therefore cannot observe: which of the forms 5 / 6 / 7 / 8 a
wave-per-frame plan launches (dct_form computes it from n_mels, n_mfcc and the 64 KB limit as setup_wpf does; a plan whose
table upload failed would run form 8 and still be held to the same bound), whether a clip took the fix-up or the add branch
inside form 3 / 4, and whether mfcc() after set_fuse_tail(2) ran in clip mode (fused_tail answers for mfcc_modspec()).  A
call the pinned log-mel kernel does not take (test_gpu_stages.takes) is held to the same bound and booked as handed over,
to no form.  Every parametrised case names the forms it is meant to reach; test_every_form_is_named asserts that the cases
of this file name all nine rows and every KB of row 8.  Each test prints the largest c_M per form ("stage-c ... c_M="
lines, shown with -s): docs/experiments.md holds the table."""
import numpy as np
import pytest

import dct_oracle as D
import stage_oracle as S
from test_gpu_parity import _ANY_NFFT, VARIANTS, _plan, _variant
from test_gpu_stages import C1, REF_DEFAULT, _batches, takes

pytestmark = pytest.mark.gpu

TOP_DBS = (80.0, 40.0, -1.0)
ALL_FORMS = {"1", "2", "3", "4", "5", "6", "7", "8/4", "8/8", "8/10", "8/12", "8/16", "9"}


def has_empty_filters(cfg):
    W = S.mel_weights(cfg)
    empty = ~(W != 0).any(-1)
    return bool(empty.any() and not empty.all())


def wave_form(cfg):
    """The matrix-pipe form of a wave-per-frame plan (setup_wpf, mm_mfcc_f32) or None where it has none: batches of 10 or 8
    steps, whichever pads nk = ceil(n_mels / 4) less; the A operands [ceil(n_mfcc / 16)][nk padded][64] and four
    16-frame tiles of odd pitch must fit 64 KB; at most 128 filters."""
    n_mels, n_mfcc = int(cfg["n_mels"]), int(cfg["n_mfcc"])
    nk, kbn = (n_mels + 3) // 4, (n_mfcc + 15) // 16
    ch = 10 if (nk + 9) // 10 * 10 <= (nk + 7) // 8 * 8 else 8
    nkp = (nk + ch - 1) // ch * ch
    if n_mels > 128 or (kbn * nkp * 64 + 4 * 16 * ((4 * nkp) | 1)) * 4 > 65536:
        return None
    if ch != 10:
        return "7"
    return "5" if n_mels % 4 == 0 and n_mels <= 80 else "6"


def dct_form(cfg, fuse_dct, path, fused_dct=False, clip=False, ragged=False):
    """The form a call runs: cfg, the set_fuse_dct switch, the log-mel kernel that takes the call (a KERNEL_PATHS name) and
    what plan.fused_dct reports under that pin (the staged-sample kernel's fused tables must fit its LDS layout: only the
    plan knows)."""
    if ragged:
        return "9"
    if path == "radix16-wpf":
        w = wave_form(cfg) if fuse_dct else None
        if w is not None:
            return w
        kb = (int(cfg["n_mfcc"]) + 3) // 4
        return "8/%d" % next(k for k in (4, 8, 10, 12, 16) if kb <= k or k == 16)
    may_fuse = fuse_dct and (path == "radix16-w16s" or (path == "radix16-m12" and cfg["n_mfcc"] <= 16))
    assert bool(fused_dct) == bool(may_fuse and fused_dct), (path, fuse_dct, fused_dct)
    if not fused_dct:
        return "1"
    if clip:
        return "4"
    return "3" if path == "radix16-w16s" and has_empty_filters(cfg) else "2"


class Worst:
    """The largest c_M per coefficient index over some calls."""

    def __init__(self, cfg):
        self.cfg, self.c, self.calls = cfg, np.zeros(cfg["n_mfcc"]), 0

    def add(self, c):
        self.c = np.maximum(self.c, c)
        self.calls += 1

    def note(self, form, path, what):
        if not self.calls:
            return
        cfg, r, c = self.cfg, D.c_ref(self.cfg), self.c
        tail = f" c_M[2:]={c[2:].max():.2f} C_ref[2:]={r[2:].max():.2f}" if c.size > 2 else ""
        print(f"stage-c form={form} path={path} n_fft={cfg['n_fft']} mel={cfg['n_mels']} mfcc={cfg['n_mfcc']} "
              f"top_db={cfg['top_db']:g} c_M/bound={float((c / D.bounds(cfg)).max()):.2f} c_M[0]={c[0]:.2f} C_ref[0]={r[0]:.2f}"
              f" c_M[1]={c[min(1, c.size - 1)]:.2f} C_ref[1]={r[min(1, c.size - 1)]:.2f}{tail} calls={self.calls} ({what})")


def held(got, cfg, ref, what):
    """got [14, n_mfcc, T] of the case clips held to the bound per coefficient; names the worst (clip, frame, k); -> c_M[k]."""
    assert got.shape == (S.N_CASES, cfg["n_mfcc"], ref.M.shape[1]), (what, got.shape)
    assert np.isfinite(got).all(), f"{what}: MFCC of the case clips not finite"
    c = D.mfcc_error(got, ref)
    ratio = c / D.bounds(cfg)
    if not (ratio <= 1.0).all():
        b, t, k = np.unravel_index(np.argmax(ratio), ratio.shape)
        raise AssertionError(f"{what}: worst c_M = {c[b, t, k]:.4g} at clip {b} frame {t} k {k} (bound {D.bounds(cfg)[k]:.2f}, "
                             f"C_ref[k] {D.c_ref(cfg)[k]:.2f}): got {got[b, k, t]!r}, reference {ref.M[b, t, k]!r}; "
                             f"per k {np.round(c.max(axis=(0, 1)), 2).tolist()}")
    return c.max(axis=(0, 1))


def check(plan, cfg, n, view, keep, what):
    ref = D.reference(cfg, n)
    T = ref.M.shape[1]
    assert plan.cfg.num_frames(n) == T and view.shape[1] == n
    got = plan.mfcc(view)
    assert tuple(got.shape) == (view.shape[0], cfg["n_mfcc"], T), (what, tuple(got.shape))
    return held(got.cpu().numpy()[keep], cfg, ref, what)


def run_path(plan, cfg, path, fuse, gpu, what):
    """Every length of frame_lengths in its layouts on the pinned kernel -> {form: Worst} (the calls the kernel handed over
    under 'handed-over')."""
    lens = D.frame_lengths(cfg)
    fused = plan.fused_dct
    form = dct_form(cfg, fuse, path, fused)
    out = {form: Worst(cfg), "handed-over": Worst(cfg)}
    frames = set()
    for n in lens:
        if path == "radix16-h32":
            n, kind = D.aligned_length(cfg, n), "aligned"
        else:
            kind = "layouts" if n == lens[-1] else "plain"
        for layout, view, keep, nan_clip in _batches(cfg, n, gpu, kind):
            mine = takes(path, n, view)
            out[form if mine else "handed-over"].add(check(plan, cfg, n, view, keep, f"{what} n {n} {layout}"))
            if mine:
                frames.add((plan.cfg.num_frames(n), nan_clip))
    assert {T for T, _ in frames} == set(D.FRAME_EDGES) and (D.FRAME_EDGES[-1], True) in frames, (what, sorted(frames))
    return out


def run_cfg(base, fuse, gpu, what, variants, expect):
    """One configuration at every top_db: every variant pinned in turn (duplicates dropped by plan.kernel_path), the fused
    DCT allowed or forbidden.  expect: {path: form} -- the paths the variants must reach and the form each is meant to run."""
    D.check_case_set(base)
    for top_db in TOP_DBS:
        cfg = dict(base, top_db=top_db)
        plan = _plan(cfg)
        prev = plan.set_fuse_dct(fuse)
        try:
            seen = {}
            for variant in variants:
                with _variant(plan, variant):
                    path = plan.kernel_path
                    if path in seen:
                        continue
                    res = run_path(plan, cfg, path, fuse, gpu, f"{what} top_db {top_db:g} {path}")
                    seen[path] = next(f for f in res if f != "handed-over")
                for form, w in res.items():
                    w.note(form, path, what)
        finally:
            plan.set_fuse_dct(prev)
        assert sorted(seen) == sorted(expect), (what, seen)
        for path, form in expect.items():
            assert seen[path] == form, (what, path, seen[path], form)


# ---- n_fft 512 plans ---------------------------------------------------------------------------------------------------------

def _tile512(n_mfcc_fused_m12, wave, valu, w16s="2"):
    on = {"radix16-m12": ("2" if n_mfcc_fused_m12 else "1"), "radix16-w16s": w16s, "radix16-h32": "1", "radix16-w16": "1",
          "radix16-w8": "1", "radix16-wpf": wave, "generic": "1"}
    off = dict({p: "1" for p in on}, **{"radix16-wpf": valu})
    return on, off


# name: (cfg, forms with the fused DCT allowed, forms with it forbidden)
_TILE512 = {
    "c1": (C1,) + _tile512(True, "5", "8/4"),
    "c1-mfcc16": (dict(C1, n_mfcc=16),) + _tile512(True, "5", "8/4"),            # the last size m12 fuses
    "c1-mfcc17": (dict(C1, n_mfcc=17),) + _tile512(False, "5", "8/8"),           # a second accumulator block
    "c1-mfcc33": (dict(C1, n_mfcc=33),) + _tile512(False, "5", "8/10"),          # a third
    "c1-mfcc40": (dict(C1, n_mfcc=40),) + _tile512(False, "5", "8/10"),          # n_mfcc == n_mels
    "refdefault": (REF_DEFAULT,) + _tile512(True, "7", "8/4", w16s="3"),         # 26 empty filters: the add branch
}


@pytest.mark.parametrize("fuse", [True, False], ids=["fused", "separate"])
@pytest.mark.parametrize("name", sorted(_TILE512))
def test_nfft512_plans(name, fuse, gpu):
    """Every variant of VARIANTS on the n_fft 512 plans: forms 2 / 3 where the DCT is fused into the log-mel launch (clips
    that clamp and clips that do not in the same batch), form 1 behind every other tile kernel and behind all of them after
    set_fuse_dct(False), forms 5 / 7 and 8 behind the wave-per-frame kernel."""
    cfg, on, off = _TILE512[name]
    assert has_empty_filters(cfg) == (name == "refdefault")
    run_cfg(cfg, fuse, gpu, f"{name} {'fused' if fuse else 'separate'}", VARIANTS, on if fuse else off)


# ---- wave-per-frame plans: the log-mel kernel unchanged, n_mels / n_mfcc varied --------------------------------------------------

_WPF1024 = dict(sr=16000, n_fft=1024, win_length=400, hop_length=160, fmin=0.0, fmax=8000.0)
_WPF2048 = dict(sr=16000, n_fft=2048, win_length=640, hop_length=160, fmin=0.0, fmax=8000.0)
# (base, n_mels, n_mfcc, fused DCT allowed, form)
_WPF = [
    (_WPF1024, 40, 13, True, "5"), (_WPF1024, 40, 17, True, "5"), (_WPF1024, 40, 33, True, "5"),
    (_WPF1024, 80, 16, True, "5"), (_WPF1024, 80, 32, True, "5"), (_WPF1024, 80, 48, True, "5"),
    (_WPF1024, 37, 13, True, "6"), (_WPF1024, 37, 17, True, "6"),           # the split loader; 37 -> 40 filters of pitch 41
    (_WPF1024, 78, 33, True, "6"), (_WPF1024, 100, 16, True, "6"), (_WPF1024, 100, 48, True, "6"),     # 25 steps padded to 30
    (_WPF1024, 30, 13, True, "7"), (_WPF1024, 48, 17, True, "7"), (_WPF1024, 64, 32, True, "7"), (_WPF1024, 128, 48, True, "7"),
    (_WPF1024, 128, 128, True, "8/16"),                                     # the A operands exceed 64 KB: VALU without a switch
    (_WPF2048, 160, 20, True, "8/8"),                                       # more than 128 filters: VALU
    (_WPF1024, 80, 13, False, "8/4"), (_WPF1024, 37, 20, False, "8/8"), (_WPF1024, 80, 40, False, "8/10"),
    (_WPF1024, 78, 48, False, "8/12"), (_WPF1024, 80, 64, False, "8/16"),
]


@pytest.mark.parametrize("base,n_mels,n_mfcc,fuse,form", _WPF,
                         ids=[f"nfft{c[0]['n_fft']}-mel{c[1]}-mfcc{c[2]}-{'fused' if c[3] else 'separate'}-form{c[4]}" for c in _WPF])
def test_wave_per_frame_plans(base, n_mels, n_mfcc, fuse, form, gpu):
    """n_fft 1024 / 2048: the three matrix-pipe instantiations (pad to ten or eight steps, the split loader for n_mels % 4 != 0,
    one to three coefficient blocks) and the VALU kernel at each of its five KB."""
    cfg = dict(base, n_mels=n_mels, n_mfcc=n_mfcc)
    assert not has_empty_filters(cfg) and (S.mel_weights(cfg) != 0).any(-1).all()
    assert _plan(cfg).kernel_path == "radix16-wpf"
    run_cfg(cfg, fuse, gpu, f"wpf mel {n_mels} mfcc {n_mfcc}", ["auto"], {"radix16-wpf": form})


# ---- row 1 behind the generic and the any-length kernel ----------------------------------------------------------------------------

_ROW1 = {
    "generic-nfft4096": (dict(sr=16000, n_fft=4096, win_length=2000, hop_length=250, n_mels=64, n_mfcc=17, fmin=0.0, fmax=8000.0), "generic"),
    "any-nfft400": (dict(_ANY_NFFT[0][0], n_mfcc=17), "any-length"),
}


@pytest.mark.parametrize("name", sorted(_ROW1))
def test_generic_and_any_length_plans(name, gpu):
    cfg, path = _ROW1[name]
    assert cfg["n_fft"] in (400, 4096) and _plan(cfg).kernel_path == path
    run_cfg(cfg, True, gpu, name, ["auto"], {path: "1"})


# ---- row 9: ragged ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["c1-mfcc17", "refdefault"])
def test_ragged_plans(name, gpu):
    """mfcc_ragged on one padded batch of 14 x 11 clips: every case clip at every length of frame_lengths, neighbours differing
    in both (the loud noise clip lies beside the AM clip, whose own clamp is active at top_db 40), NaN behind every clip's
    end.  Each clip is held to the bound of the clip ALONE -- the reference of its own length: its own maximum, its own
    centre padding -- and the columns behind its frame count are exactly 0.0."""
    import torch
    base = _TILE512[name][0]
    lens = D.frame_lengths(base)
    rows = [(i % S.N_CASES, (i // S.N_CASES + i) % len(lens)) for i in range(S.N_CASES * len(lens))]
    assert len(set(rows)) == len(rows)
    host = np.full((len(rows), lens[-1]), np.nan, dtype=np.float32)
    for i, (r, j) in enumerate(rows):
        host[i, :lens[j]] = S.cases(lens[j], base)[r]
    audio = torch.from_numpy(host).to(gpu)
    n_of = np.array([lens[j] for _, j in rows])
    for top_db in TOP_DBS:
        cfg = dict(base, top_db=top_db)
        plan = _plan(cfg)
        assert dct_form(cfg, True, plan.kernel_path, plan.fused_dct, ragged=True) == "9"
        got, frames = plan.mfcc_ragged(audio, n_of)
        assert tuple(got.shape) == (len(rows), cfg["n_mfcc"], D.FRAME_EDGES[-1])
        got, frames = got.cpu().numpy(), frames.cpu().numpy()
        assert frames.tolist() == [D.FRAME_EDGES[j] for _, j in rows]
        w = Worst(cfg)
        for j, n in enumerate(lens):
            idx = np.array([i for i, (_, jj) in enumerate(rows) if jj == j])
            idx = idx[np.argsort([rows[i][0] for i in idx])]
            T = D.FRAME_EDGES[j]
            tail = got[idx][:, :, T:]
            assert (tail == 0.0).all() and not np.signbit(tail).any(), f"{name} top_db {top_db:g} n {n}: columns behind T_b not 0.0"
            w.add(held(got[idx][:, :, :T], cfg, D.reference(cfg, n), f"ragged {name} top_db {top_db:g} n {n}"))
        w.note("9", plan.kernel_path, f"ragged {name}")


# ---- row 4: clip mode ------------------------------------------------------------------------------------------------------------

def _all_clips_held(m, rows, cfg, ref, what):
    w = Worst(cfg)
    for s in range(0, len(rows), S.N_CASES):
        blk = rows[s:s + S.N_CASES]
        if len(blk) == S.N_CASES:      # a rotation of the case set: put it back in order (the last few clips: bit-equality only)
            w.add(held(m[s:s + S.N_CASES][np.argsort(blk)], cfg, ref, f"{what} clips {s}.."))
    return w


@pytest.mark.parametrize("name", ["c1", "refdefault"])
def test_clip_mode(name, gpu):
    """Whole clips per workgroup: as many clips as the device has compute units (fused_tail wants an even spread), 257 frames
    each (a 512-point trajectory), the case clips repeated with a rotation so that neighbouring workgroups hold different
    ones.  MFCC bit for bit equal to the same call after set_fuse_tail(False) (include/modmfcc.h promises it), and every
    clip held to the bound.  On the reference-default plan (empty filters) mfcc() itself runs in clip mode after
    set_fuse_tail(2), the empty filters' add inside the launch: the same two assertions."""
    import torch
    base = _TILE512[name][0]
    n = D.frame_lengths(base)[-1]
    B = torch.cuda.get_device_properties(gpu).multi_processor_count          # one clip per workgroup
    rows = [(i + i // S.N_CASES) % S.N_CASES for i in range(B)]
    audio = torch.from_numpy(np.ascontiguousarray(S.cases(n, base)[rows])).to(gpu)
    for top_db in TOP_DBS:
        cfg = dict(base, top_db=top_db)
        plan = _plan(cfg)
        ref = D.reference(cfg, n)
        assert plan.kernel_path == "radix16-w16s" and plan.fused_dct and plan.fused_tail(B, n)
        assert dct_form(cfg, True, plan.kernel_path, plan.fused_dct, clip=plan.fused_tail(B, n)) == "4"
        m1, _ = plan.mfcc_modspec(audio)
        prev = plan.set_fuse_tail(False)
        try:
            assert not plan.fused_tail(B, n)
            m0, _ = plan.mfcc_modspec(audio)
            ms = plan.mfcc(audio)
        finally:
            plan.set_fuse_tail(prev)
        assert tuple(m1.shape) == (B, cfg["n_mfcc"], D.FRAME_EDGES[-1])
        assert torch.equal(m0, ms) and torch.equal(m1, m0), float((m1 - m0).abs().max())
        _all_clips_held(m1.cpu().numpy(), rows, cfg, ref, f"clip mode {name} top_db {top_db:g}").note("4", plan.kernel_path, f"clip mode {name}")
        if name == "refdefault":
            prev = plan.set_fuse_tail(2)
            try:
                assert plan.fused_tail(B, n)
                m2 = plan.mfcc(audio)
            finally:
                plan.set_fuse_tail(prev)
            assert torch.equal(m2, m0), float((m2 - m0).abs().max())
            _all_clips_held(m2.cpu().numpy(), rows, cfg, ref, f"clip mode mfcc() {name} top_db {top_db:g}").note(
                "4", plan.kernel_path, f"clip mode mfcc() {name}")


def test_every_form_is_named():
    """The forms the cases of this file are meant to reach -- each case asserts that it does -- are all nine rows, row 8 at
    each of its five KB."""
    named = {"9", "4"}                                               # test_ragged_plans, test_clip_mode
    for _, on, off in _TILE512.values():
        named |= set(on.values()) | set(off.values())
    named |= {form for *_, form in _WPF} | {"1"}                      # test_generic_and_any_length_plans
    assert named == ALL_FORMS, sorted(named)
    for base, n_mels, n_mfcc, fuse, form in _WPF:
        assert dct_form(dict(base, n_mels=n_mels, n_mfcc=n_mfcc), fuse, "radix16-wpf") == form, (n_mels, n_mfcc, fuse, form)
    for name, (cfg, on, off) in _TILE512.items():
        assert dct_form(cfg, True, "radix16-wpf") == on["radix16-wpf"] and dct_form(cfg, False, "radix16-wpf") == off["radix16-wpf"], name
