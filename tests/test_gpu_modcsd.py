"""GPU: the Welch cross spectrum and coherence (modulation_cross_spectra_batch and its kin, MfccPlan.mfcc_modcsd;
mm_modcsd_f32) against the yardstick of tests/modcsd_oracle.py on the parameter sets of its list, the properties of the
coherence that need no reference, the identities bit for bit (alone / in a batch / shared y / padding / strides / lengths /
NULL outputs) and the stream contract of mm_modcsd_f32 with the steps of tests/test_gpu_streams.py.

The kernel gives segment i of a pair to chunk i // 32 (a workgroup) and wave i % 4 of it: the list has pairs of 1, 4, 5 (a
remainder over the four waves), 32 (a full chunk), 33 (two chunks: the finish kernel) and 65 (three) segments.  No call has
more than 48 rows.
"""
import itertools

import numpy as np
import pytest

import modcsd_oracle as O
import modpsd_oracle as P
import stream_cases as S
import test_gpu_streams as TS

pytestmark = pytest.mark.gpu

FS = O.FS
NORMAL = float(np.finfo(np.float32).tiny)


def dev(a, gpu):
    import torch
    return torch.from_numpy(np.array(a)).to(gpu)


def device_spectra(x, y, p, gpu):
    """modulation_cross_spectra_batch in calls of at most 32 pairs -> f, [Pxx, Pyy, Pxy, Cxy] as numpy."""
    import torch
    from modulation_mfcc_amd import modulation_cross_spectra_batch
    parts = []
    for a in range(0, x.shape[0], 32):
        f, *o = modulation_cross_spectra_batch(dev(x[a:a + 32], gpu), dev(y[a:a + 32], gpu), p.fs, **p.kwargs())
        assert [t.dtype for t in o] == [torch.float32, torch.float32, torch.complex64, torch.float32]
        parts.append([t.cpu().numpy() for t in o])
    return f, [np.concatenate(c) for c in zip(*parts)]


def check_coherence_properties(pxx, pyy, pxy, coh, one_segment, what):
    """What holds without a reference: NaN exactly where Pxx Pyy == 0, never above 1, exactly 1 for one segment, and within
    6 * 2^-24 of |Pxy|^2 / (Pxx Pyy) of the returned float32 spectra where Pxx and Pyy are normal numbers (four rounded
    factors, its own rounding, one to spare).

    The coherence comes from the float64 sums, so a power below float32's range (under 2^-149: the bin a quarter of the way
    up for the cosine on the last bin, exact zeros but for 1e-25 of rounding) is returned as 0 beside a coherence that is a
    number.  Such a bin must show that it is one: the power its own Pxy and coherence imply, |Pxy|^2 / (C P_other), is
    below 2^-149.  Everywhere else NaN and Pxx Pyy == 0 coincide."""
    nan = np.isnan(coh)
    none = pxx.astype(np.float64) * pyy.astype(np.float64) == 0
    assert not (nan & ~none).any(), (what, np.argwhere(nan & ~none)[:6].tolist())
    tiny = 2.0 ** -149
    for r, k in np.argwhere(none & ~nan):
        other = max(float(pxx[r, k]), float(pyy[r, k]))
        g2 = abs(complex(pxy[r, k])) ** 2
        implied = g2 / (float(coh[r, k]) * other) if other > 0 and coh[r, k] > 0 else (0.0 if g2 <= tiny * tiny else np.inf)
        assert implied <= tiny * (1 + 1e-5), (what, int(r), int(k), float(pxx[r, k]), float(pyy[r, k]), complex(pxy[r, k]),
                                             float(coh[r, k]), implied)
    assert (coh[~nan] <= np.float32(1.0)).all() and (coh[~nan] >= 0).all(), (what, float(coh[~nan].max()))
    if one_segment:
        assert (coh[~nan] == np.float32(1.0)).all(), what
    ok = ~nan & (pxx >= NORMAL) & (pyy >= NORMAL)
    want = np.abs(pxy.astype(np.complex128)[ok]) ** 2 / (pxx.astype(np.float64)[ok] * pyy.astype(np.float64)[ok])
    rel = np.abs(coh.astype(np.float64)[ok] - want)
    assert (rel <= 6 * O.EPS * want).all(), (what, float((rel / np.maximum(want, 1e-300)).max() / O.EPS))
    return int(ok.sum())


# ---- against the yardstick ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(O.N_GPU_SETS), ids=O.GPU_SET_IDS)
def test_every_output_against_the_yardstick(i, gpu):
    p, T = O.gpu_set(i)
    x, y = O.pairs_for(p, T)
    f, (pxx, pyy, pxy, coh) = device_spectra(x, y, p, gpu)
    assert pxx.shape == pyy.shape == pxy.shape == coh.shape == (64, p.bins)
    np.testing.assert_array_equal(f, P.welch64(x[:1], p)[0])
    cx = P.check(pxx, x, p, "Pxx")
    cy = P.check(pyy, y, p, "Pyy")
    c1, c2 = (float(c.max()) for c in O.cross_errors(pxy, x, y, p))
    print(f"{O.GPU_SET_IDS[i]} T {T}: Pxx c {cx:.2f} Pyy c {cy:.2f} (tolerance {P.tolerance(p, T):.2f}); Pxy c {c1:.2f} "
          f"(tolerance {O.tolerance(p, T):.2f}) c2 {c2:.2f} (tolerance {O.tolerance(p, T, True):.2f})")
    O.check_pxy(pxy, x, y, p, "modulation_cross_spectra_batch", measures=(True,))     # (the first-order measure: next test)
    # a side that puts nothing but zeros into the transform comes back as exact zeros, the cross spectrum with it
    zx, zy = (O.row_norm(x, p) == 0)[:, 0], (O.row_norm(y, p) == 0)[:, 0]
    assert zy[48:].all() and zx[15::16].all()
    assert (pxx[zx].view(np.int32) == 0).all() and (pyy[zy].view(np.int32) == 0).all()
    assert (pxy[zx | zy] == 0).all() and np.isnan(coh[zx | zy]).all()
    n = check_coherence_properties(pxx, pyy, pxy, coh, p.num_segments(T) == 1, O.GPU_SET_IDS[i])
    assert n > 24 * p.bins                                    # (the relative check saw the bins of the live pairs)
    if i in O.COH_SETS:                                       # (a detrend under a boxcar window leaves bin 0 without power)
        live = [0, 1, 2, 4, 5, 6]                             # the trajectory and noise rows: power in every bin
        assert not np.isnan(coh[live]).any() and not np.isnan(coh[[32 + r for r in live]]).any()


@pytest.mark.parametrize("i", range(O.N_GPU_SETS), ids=O.GPU_SET_IDS)
def test_pxy_within_the_first_order_measure(i, gpu):
    """The Pxy measure as the issue states it, without the second-order term, with its own C_ref (the oracle's module text:
    why every other test checks both measures, and why this one binds nothing where C_ref is 2.5e7 or inf).  Where it does
    bind it is the hardest check of the file: at pair 7 -- the impulse at sample 0 against itself, under the zero of the Hann
    taper, so that only what the detrend subtracted is transformed -- neither side has a true amplitude and |G - A| is the
    product of the two transforms' rounding noise.  With float32 butterflies the kernel reached c = 6.05 of 4.15 (64 points)
    and 60.3 of 4.99 (1024 points) there; with the butterflies evaluated in float64 (mcsd_cfft_lds) 1.44 and 1.25."""
    p, T = O.gpu_set(i)
    x, y = O.pairs_for(p, T)
    _, (_, _, pxy, _) = device_spectra(x, y, p, gpu)
    O.check_pxy(pxy, x, y, p, "modulation_cross_spectra_batch", measures=(False,))


@pytest.mark.parametrize("i", O.COH_SETS, ids=[O.GPU_SET_IDS[i] for i in O.COH_SETS])
def test_coherence_against_scipy(i, gpu):
    """White noise plus a shared component: every bin carries power, no bin is excluded; the bound is MARGIN x the largest
    error of the oracle's float32 pipeline on the same pairs."""
    from modulation_mfcc_amd import modulation_coherence_batch
    p, T = O.gpu_set(i)
    x, y = O.coherence_pairs(T)
    kw = {k: v for k, v in p.kwargs().items() if k != "scaling"}
    f, coh = modulation_coherence_batch(dev(x, gpu), dev(y, gpu), p.fs, **kw)
    got = coh.cpu().numpy()
    err, ref = float(O.coherence_error(got, x, y, p).max()), O.coherence_ref_error(x, y, p)
    print(f"{O.GPU_SET_IDS[i]}: coherence error {err:.3e}, float32 pipeline {ref:.3e}, bound {O.MARGIN * ref:.3e}")
    assert np.isfinite(got).all() and err <= O.MARGIN * ref, (err, ref)


def test_defaults_shapes_and_single_outputs(gpu):
    import torch
    from modulation_mfcc_amd import (modulation_coherence_batch, modulation_cross_spectra_batch, modulation_csd_batch,
                                     modulation_psd_batch)
    p = O.Params(FS, "hann", 256, 128, 256, "constant", "density")
    r = O.rows_for(p, 1001)
    x, y = dev(P.take(r, 26, 0), gpu).reshape(2, 13, 1001), dev(r[[0, 5]], gpu)
    f, pxx, pyy, pxy, coh = modulation_cross_spectra_batch(x, y, FS)
    assert f.shape == (129,) and pxx.shape == pyy.shape == pxy.shape == coh.shape == (2, 13, 129)
    xs, ys = P.take(r, 26, 0), np.repeat(r[[0, 5]], 13, axis=0)
    P.check(pxx.reshape(26, 129).cpu().numpy(), xs, p, "defaults Pxx")
    P.check(pyy.reshape(26, 129).cpu().numpy(), ys, p, "defaults Pyy")
    O.check_pxy(pxy.reshape(26, 129).cpu().numpy(), xs, ys, p, "defaults Pxy")
    assert TS.bit_equal(modulation_csd_batch(x, y, FS)[1], pxy) and TS.bit_equal(modulation_coherence_batch(x, y, FS)[1], coh)
    # the auto spectra are within the yardstick of modulation_psd_batch, and (documented) not its bits
    P.check(modulation_psd_batch(x, FS)[1].reshape(26, 129).cpu().numpy(), xs, p, "psd")
    # one row, one dimension; nperseg 100 -> nfft 128
    f1, c1 = modulation_csd_batch(x[0, 0], y[0], FS, nperseg=100)
    assert c1.shape == (65,) and f1.shape == (65,) and c1.dtype == torch.complex64
    with pytest.raises(ValueError, match="greater than the input length"):
        modulation_csd_batch(x[..., :255], y[..., :255], FS)
    with pytest.raises(ValueError, match="divisor"):
        modulation_csd_batch(x, dev(r[:4], gpu), FS)
    with pytest.raises(ValueError, match="samples per row"):
        modulation_csd_batch(x, y[:, :1000], FS)
    with pytest.raises(NotImplementedError, match=r"\[32, 2048\]"):
        modulation_csd_batch(x, y, FS, nfft=4096)


# ---- bit identities -------------------------------------------------------------------------------------------------------------
RP = dict(window="hann", nperseg=64, noverlap=32, nfft=64, detrend="linear", scaling="density")
R_NMAX = 64 + 32 * 40                      # 41 segments: two chunks
R_LENS = [R_NMAX, 64, 65, 95, 96, 200, 64 + 32 * 31, 64 + 32 * 32, 64 + 32 * 32 - 1, 1000, 777, 64 + 32 * 4, 500]


def _rows(gpu, rows=26, seed=0):
    g = np.random.default_rng(seed)
    x = (3.0 + g.standard_normal((rows, R_NMAX))).astype(np.float32)
    y = (x[::13] * 0.5 + g.standard_normal((rows // 13, R_NMAX))).astype(np.float32)
    lens = np.array([R_LENS[i % len(R_LENS)] for i in range(rows)], dtype=np.int64)
    return dev(x, gpu), dev(y, gpu), lens


def _same(a, b):
    return all(TS.bit_equal(s, t) for s, t in zip(a, b))


def test_a_pair_alone_in_the_batch_and_with_y_shared_or_materialised(gpu):
    import torch
    from modulation_mfcc_amd import modulation_cross_spectra_batch as single, modulation_cross_spectra_ragged_batch as ragged
    x, y, lens = _rows(gpu)
    f, *full = ragged(x, y, lens, FS, **RP)                                     # y_group 13
    assert all(t.shape == (26, 33) for t in full)
    ymat = y.repeat_interleave(13, dim=0)
    assert _same(ragged(x, ymat, lens, FS, **RP)[1:], full), "y_group 1 on a materialised copy of y"
    assert _same(ragged(x, y, dev(lens, gpu), FS, **RP)[1:], full), "device lengths"
    for b, n in enumerate(lens):
        alone = single(x[b, :n], y[b // 13, :n], FS, **RP)[1:]
        assert _same([t[b] for t in full], alone), (b, int(n))
    assert _same(ragged(x[5:6], y[0:1], lens[5:6], FS, **RP)[1:], [t[5:6] for t in full])
    # every pair at n_max: the non-ragged call, and its rows alone (one chunk less in no row, the workspace route in all)
    _, *u = single(x, y, FS, **RP)
    assert _same(single(x[14:15], y[1:2], FS, **RP)[1:], [t[14:15] for t in u])
    assert _same([t[0] for t in u], [t[0] for t in full])                       # lens[0] == n_max
    # against the reference: one, five and 33 segments
    p = O.Params(FS, **RP)
    for b in (1, 11, 7):
        xs, ys = x[b, :lens[b]].cpu().numpy(), y[b // 13, :lens[b]].cpu().numpy()
        P.check(full[0][b].cpu().numpy(), xs, p, f"ragged pair {b} Pxx")
        P.check(full[1][b].cpu().numpy(), ys, p, f"ragged pair {b} Pyy")
        O.check_pxy(full[2][b].cpu().numpy(), xs, ys, p, f"ragged pair {b}")
    assert torch.isfinite(torch.view_as_real(full[2])).all()


def test_padding_and_strides_never_matter(gpu):
    import torch
    from modulation_mfcc_amd import modulation_cross_spectra_ragged_batch as ragged
    x, y, lens = _rows(gpu)
    _, *full = ragged(x, y, lens, FS, **RP)
    cols = torch.arange(R_NMAX, device=gpu)[None, :]
    behind_x = cols >= dev(lens, gpu)[:, None]
    behind_y = cols >= dev(lens.reshape(2, 13).max(axis=1), gpu)[:, None]       # behind the longest pair that shares the row
    for fill in (float("nan"), float("inf"), None):
        xp, yp = x.clone(), y.clone()
        xp[behind_x] = 1e6 * torch.randn(int(behind_x.sum()), device=gpu) if fill is None else fill
        yp[behind_y] = 1e6 * torch.randn(int(behind_y.sum()), device=gpu) if fill is None else fill
        assert _same(ragged(xp, yp, lens, FS, **RP)[1:], full), fill
    # y materialised: its padding begins at each pair's own length
    ymat = y.repeat_interleave(13, dim=0)
    ymat[behind_x] = float("nan")
    assert _same(ragged(x, ymat, lens, FS, **RP)[1:], full)
    # strided row views, one float behind an aligned address, NaN (another row's end) around them
    bx, by = torch.full((26, R_NMAX + 9), float("nan"), device=gpu), torch.full((2, R_NMAX + 5), float("nan"), device=gpu)
    vx, vy = bx[:, 1:1 + R_NMAX], by[:, 3:3 + R_NMAX]
    vx.copy_(x)
    vy.copy_(y)
    assert vx.stride(0) == R_NMAX + 9 and vy.stride(0) == R_NMAX + 5 and vx.data_ptr() % 8 == 4
    assert _same(ragged(vx, vy, lens, FS, **RP)[1:], full)
    perm = np.random.default_rng(1).permutation(26)
    _, *pp = ragged(x[dev(perm, gpu)], ymat[dev(perm, gpu)], lens[perm], FS, **RP)
    assert _same(pp, [t[dev(perm, gpu)] for t in full])


def test_ragged_lengths_at_the_edges(gpu):
    import torch
    from modulation_mfcc_amd import (modulation_coherence_ragged_batch, modulation_cross_spectra_ragged_batch as ragged,
                                     modulation_csd_ragged_batch)
    x, y, lens = _rows(gpu)
    lens = lens.copy()
    lens[3], lens[4], lens[5], lens[20] = 63, 64, R_NMAX, 1
    with pytest.raises(ValueError, match=r"row 3 has 63 samples"):
        ragged(x, y, lens, FS, **RP)
    _, *got = ragged(x, y, dev(lens, gpu), FS, **RP)
    ok = lens.copy()
    ok[3] = ok[20] = 64
    _, *want = ragged(x, y, ok, FS, **RP)
    bad = torch.zeros(26, dtype=torch.bool, device=gpu)
    bad[3] = bad[20] = True
    for g, w in zip(got, want):
        g, w = (torch.view_as_real(t) if t.is_complex() else t for t in (g, w))
        assert torch.isnan(g[bad]).all() and TS.bit_equal(g[~bad], w[~bad]) and not torch.isnan(w[:, 1:]).any()
    # lengths outside [1, n_max] are clamped on the device; n_max with at most 32 segments: one launch, NaN pairs too
    wild = torch.tensor([10 ** 12, 0, -5, 64], device=gpu)
    kw = {k: v for k, v in RP.items() if k != "scaling"}
    _, cw = modulation_coherence_ragged_batch(x[:4, :500], y[:1, :500], wild, FS, **kw)
    _, cr = modulation_coherence_ragged_batch(x[:4, :500], y[:1, :500], torch.tensor([500, 1, 1, 64], device=gpu), FS, **kw)
    assert TS.bit_equal(cw, cr) and torch.isnan(cw[1:3]).all() and not torch.isnan(cw[[0, 3], 1:]).any()
    _, pw = modulation_csd_ragged_batch(x[:4, :500], y[:1, :500], wild, FS, **RP)
    assert torch.isnan(torch.view_as_real(pw[1:3])).all() and torch.isfinite(torch.view_as_real(pw[[0, 3]])).all()
    with pytest.raises(ValueError, match="greater than the input length"):
        ragged(x[:4, :63], y[:1, :63], torch.tensor([63, 63, 64, 1], device=gpu), FS, **RP)
    with pytest.raises(ValueError, match=r"lengths must lie in \[1, "):
        ragged(x, y, np.where(lens == 1, 0, lens), FS, **RP)


# ---- NULL outputs, the guard band and the refusals of the entry ------------------------------------------------------------------
@pytest.mark.parametrize("T", (64 + 32 * 6, R_NMAX), ids=("one-launch", "two-launches"))
def test_every_subset_of_outputs_and_the_guard_band(T, gpu):
    import torch
    from modulation_mfcc_amd import _lib, modcsd, modpsd
    lib = _lib.load()
    spec = modcsd._spec(FS, **RP)
    plan = modpsd._modpsd_plan(spec, gpu)
    x, y, _ = _rows(gpu)
    x, y = x[:, :T].contiguous(), y[:, :T].contiguous()
    lens = dev(np.array([T, 64, 63, T - 1] * 6 + [T, 100]), gpu)
    need = int(lib.mm_modcsd_workspace_bytes(plan.h, 26, T))
    assert (need > 0) == (T == R_NMAX) and need == (0 if T != R_NMAX else 26 * 2 * 4 * 33 * 8)
    ws = torch.empty(max(need, 8), dtype=torch.uint8, device=gpu)
    stride = spec.bins + 5

    def call(mask, x_ptr=None, **kw):
        outs = [torch.full((26, stride, 2) if j == 2 else (26, stride), -7.0, device=gpu) for j in range(4)]
        a = dict(rows=26, n_max=T, x_stride=T, y_stride=T, group=13, out_stride=stride, ws=ws.data_ptr(), need=need)
        a.update(kw)
        rc = lib.mm_modcsd_f32(plan.h, x.data_ptr(), a["rows"], a["n_max"], a["x_stride"], y.data_ptr(), a["y_stride"],
                               a["group"], lens.data_ptr(), *[o.data_ptr() if m else None for o, m in zip(outs, mask)],
                               a["out_stride"], a["ws"], a["need"], S.stream())
        torch.cuda.synchronize()
        return rc, outs

    rc, full = call((1, 1, 1, 1))
    assert rc == 0
    for o in full:
        assert (o[:, spec.bins:] == -7.0).all() and not (o[:, :spec.bins] == -7.0).any()
    _, *want = modcsd.modulation_cross_spectra_ragged_batch(x, y, lens, FS, **RP)
    want[2] = torch.view_as_real(want[2])
    assert all(TS.bit_equal(o[:, :spec.bins].contiguous(), w) for o, w in zip(full, want))
    assert torch.isnan(full[3][2, :spec.bins]).all() and torch.isnan(full[2][2, :spec.bins]).all()          # the pair of 63 samples
    for mask in itertools.product((0, 1), repeat=4):
        rc, outs = call(mask)
        if not any(mask):
            assert rc == _lib.MM_ERR_INVALID_ARG
            continue
        assert rc == 0, mask
        for o, w, m in zip(outs, full, mask):
            assert TS.bit_equal(o, w) if m else (o == -7.0).all(), mask
    # refusals: a pitch below the row on either side, an output pitch below the bins, no group, a short workspace
    for kw in (dict(x_stride=T - 1), dict(y_stride=T - 1), dict(out_stride=spec.bins - 1), dict(group=0), dict(rows=0)):
        assert call((1, 1, 1, 1), **kw)[0] == _lib.MM_ERR_INVALID_ARG, kw
    if need:
        assert call((1, 1, 1, 1), need=need - 1)[0] == _lib.MM_ERR_WORKSPACE
        assert call((1, 1, 1, 1), ws=None)[0] == _lib.MM_ERR_INVALID_ARG
    # a handle of the second header at nfft 4096 is not one of this entry
    big = modpsd._modpsd_plan(modpsd._Spec(FS, "hann", 64, 32, 4096, "linear", "density"), gpu)
    o = torch.empty(26, 2049, device=gpu)
    assert lib.mm_modcsd_workspace_bytes(big.h, 26, R_NMAX) == 0
    assert lib.mm_modcsd_f32(big.h, x.data_ptr(), 26, T, T, y.data_ptr(), T, 13, None, o.data_ptr(), None, None, None, 2049,
                             None, 0, S.stream()) == _lib.MM_ERR_UNSUPPORTED


# ---- MfccPlan.mfcc_modcsd ----------------------------------------------------------------------------------------------------------
WELCH = dict(nperseg=32, noverlap=24, detrend="linear")


def test_mfcc_modcsd_against_the_oracle_on_the_plans_own_mfcc(gpu):
    import torch
    import mfcc_oracle as MO
    from modulation_mfcc_amd import (MfccConfig, MfccPlan, mfcc_modcsd_batch, mfcc_modcsd_ragged_batch,
                                     modulation_cross_spectra_batch, rms_batch)
    cfg = MfccConfig(**S.C1)
    plan = MfccPlan(cfg)
    lens = np.array([16000, 9600, 12345], dtype=np.int64)
    audio = torch.zeros(3, 16000, device=gpu)
    for b, n in enumerate(lens):
        audio[b, :n] = dev(MO.synth_clip(b, int(n), 16000, "am").astype(np.float32), gpu)
    ref = rms_batch(audio, cfg.n_fft, cfg.hop_length)
    fs = cfg.sr / cfg.hop_length
    frames = (101, 61, 78)
    assert ref.shape == (3, 101) and ref.dtype == torch.float32
    p = O.Params(fs, "hann", 32, 24, 32, "linear", "density")
    mfcc, f, *sp = plan.mfcc_modcsd(audio, ref, **WELCH)
    assert mfcc.shape == (3, 13, 101) and all(t.shape == (3, 13, 17) for t in sp) and TS.bit_equal(mfcc, plan.mfcc(audio))
    assert (f == np.fft.rfftfreq(32, 1 / fs)).all()
    assert _same(modulation_cross_spectra_batch(mfcc, ref, fs, **WELCH)[1:], sp)
    assert _same(mfcc_modcsd_batch(audio, ref, cfg, **WELCH)[2:], sp)

    def against_the_oracle(m, spectra, T_of, what):
        for b in range(3):
            xs, ys = m[b, :, :T_of[b]].cpu().numpy(), np.repeat(ref[b:b + 1, :T_of[b]].cpu().numpy(), 13, axis=0)
            P.check(spectra[0][b].cpu().numpy(), xs, p, f"{what} clip {b} Pxx")
            P.check(spectra[1][b].cpu().numpy(), ys, p, f"{what} clip {b} Pyy")
            O.check_pxy(spectra[2][b].cpu().numpy(), xs, ys, p, f"{what} clip {b}")
            check_coherence_properties(*[t[b].cpu().numpy() for t in spectra], False, f"{what} clip {b}")
    against_the_oracle(mfcc, sp, (101, 101, 101), "single")
    for ln in (lens, dev(lens, gpu)):
        mr, fr, *sr = plan.mfcc_modcsd(audio, ref, ln, **WELCH)
        assert (fr == f).all() and TS.bit_equal(mr, plan.mfcc_ragged(audio, ln)[0])
        for b in range(3):
            alone = modulation_cross_spectra_batch(mr[b, :, :frames[b]], ref[b:b + 1, :frames[b]], fs, **WELCH)[1:]
            assert _same([t[b] for t in sr], alone), b
    against_the_oracle(mr, sr, frames, "ragged")
    assert _same(mfcc_modcsd_ragged_batch(audio, ref, lens, cfg, **WELCH)[2:], sr)
    with pytest.raises(ValueError, match=r"clip 1 has 61 frames"):
        plan.mfcc_modcsd(audio, ref, lens, nperseg=64)
    nan = plan.mfcc_modcsd(audio, ref, dev(lens, gpu), nperseg=64)
    assert all(torch.isnan(torch.view_as_real(t) if t.is_complex() else t)[1].all() for t in nan[2:])
    assert not torch.isnan(nan[2][[0, 2]]).any()
    with pytest.raises(ValueError, match="one curve per clip"):
        plan.mfcc_modcsd(audio, ref[:, :100], **WELCH)


# ---- the stream contract of mm_modcsd_f32 ------------------------------------------------------------------------------------------
# Built with the registry's Case class but NOT appended to stream_cases.CASES (the registry is pinned to the entries of
# include/modmfcc.h); the checks are those of test_gpu_streams.py, called with these cases.
SP = dict(window="hann", nperseg=64, noverlap=48, nfft=64, detrend="linear", scaling="density")
S_ROWS, S_N = 6, 64 + 16 * 50              # 51 segments: two launches, a workspace; y [2, n]: y_group 3


def _data(name, ragged):
    def data():
        d = {"x": S.audio_sets(name, S_ROWS, S_N), "y": S.audio_sets(name + "/y", 2, S_N)}
        if ragged:
            d["lengths"] = S.length_sets(S_ROWS, S_N, 64)
        return d
    return data


def _wrapper_case(ragged):
    name = "modcsd/" + ("ragged-wrapper" if ragged else "wrapper")

    def setup(env):
        from modulation_mfcc_amd import modulation_cross_spectra_batch, modulation_cross_spectra_ragged_batch
        if ragged:
            return lambda: modulation_cross_spectra_ragged_batch(env.buf["x"], env.buf["y"], env.buf["lengths"], FS, **SP)[1:]
        return lambda: modulation_cross_spectra_batch(env.buf["x"], env.buf["y"], FS, **SP)[1:]
    return S.Case(name, "mm_modcsd_f32", "modcsd", _data(name, ragged), setup, ragged=ragged)


def _ctypes_case():
    """One handle for both thread instances; every instance has its own buffers, outputs and workspace."""
    name = "modcsd/ragged-ctypes"

    def setup(env):
        import torch
        from modulation_mfcc_amd import _lib, modcsd, modpsd
        lib = _lib.load()
        spec = modcsd._spec(FS, **SP)
        plan = env.plan(lambda: modpsd._ModpsdPlan(spec, env.gpu))
        outs = [env.out((S_ROWS, spec.bins, 2) if j == 2 else (S_ROWS, spec.bins), torch.float32) for j in range(4)]
        need = int(lib.mm_modcsd_workspace_bytes(plan.h, S_ROWS, S_N))
        assert need > 0
        ws = env.work(need)

        def call():
            _lib.check(lib.mm_modcsd_f32(plan.h, env.buf["x"].data_ptr(), S_ROWS, S_N, S_N, env.buf["y"].data_ptr(), S_N, 3,
                                         env.buf["lengths"].data_ptr(), *[o.data_ptr() for o in outs], spec.bins,
                                         ws.data_ptr(), need, S.stream()), "mm_modcsd_f32")
            return outs
        return call
    return S.Case(name, "mm_modcsd_f32", "modcsd", _data(name, True), setup, ragged=True, threads=True)


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
    assert all(c.entry == "mm_modcsd_f32" for c in STREAM_CASES)


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
