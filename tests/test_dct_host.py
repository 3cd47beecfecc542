"""Host only: the per-coefficient bound of the top_db clamp + DCT-II stage (dct_oracle) means something.  The float64 reference
agrees with the oracle's MFCC on golden clips; the case set meets the conditions the GPU tests rely on; C_ref[k] lies where
the module's docstring says; the fused kernels' arithmetic (unclamped DCT + correction) stays inside the bound without being
part of C_ref; every deliberate break of the clip maximum, the threshold, the clamp's extent and the DCT table is rejected at
C1 (40 / 13), the reference default (128 mel, 26 empty filters) and C4 (80 / 40) at top_db 80 and 40; and mfcc_close, the
only check this stage had, lets a threshold off by 0.001 dB through.

What the bound does NOT see (measured here, printed, asserted as such): a DCT table built from a float32 angle stays under
the bound (0.3 .. 0.6 of it).  A threshold off by 0.001 dB is required to be rejected only at top_db 40 and on the 128-mel
plan: at 80 dB it can move c0 alone on the 40- and 80-filter plans, where c0's own float32 sum is the largest.  (Measured: it
is rejected on all six, at 4.1 .. 9.4 times the bound.)"""
import numpy as np
import pytest

import dct_oracle as D
import mfcc_oracle as O
import stage_oracle as S
from conftest import load_golden, mfcc_close

REF_DEFAULT = dict(sr=10000, n_fft=512, win_length=250, hop_length=50, n_mels=128, n_mfcc=13, fmin=100.0, fmax=10000.0)


def _golden(name):
    kw = load_golden(name)[0]
    return {k: kw[k] for k in ("sr", "n_fft", "win_length", "hop_length", "n_mels", "n_mfcc", "fmin", "fmax")}


PLANS = {"c1": _golden("c1_am"), "refdefault": REF_DEFAULT, "c4": _golden("c4_am")}
CASES = [(name, top_db) for name in PLANS for top_db in (80.0, 40.0)]


@pytest.mark.parametrize("name", ["c1_am", "c1_quiet_tail", "c1_impulse", "refdefault_am", "c4_am"])
def test_reference_agrees_with_the_oracle_on_golden_clips(name):
    import warnings
    kw, y, _ = load_golden(name)
    cfg = dict(_golden(name), preemph=kw.get("preemph", 0.0), top_db=80.0)
    st = S.reference_of(y[None, :], cfg)
    ref = D.reference_from(st.L, st.dL, cfg)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                     # "Empty filters detected"
        want = O.mfcc(y, O.OracleConfig(**{k: v for k, v in kw.items() if k in O.OracleConfig().__dict__}))
    assert ref.M.shape == (1, want.shape[1], want.shape[0])
    mfcc_close(ref.M[0].T, want, name)
    # and the oracle's float32 MFCC lies inside the bound of its configuration
    c = D.mfcc_error(want[None], ref)
    assert (c.max(axis=(0, 1)) <= D.bounds(cfg)).all(), c.max(axis=(0, 1))


@pytest.mark.parametrize("name", sorted(PLANS))
def test_case_set_and_lengths(name):
    cfg = PLANS[name]
    D.check_case_set(cfg)
    from modulation_mfcc_amd import MfccConfig
    mc = MfccConfig(**cfg)
    assert [mc.num_frames(n) for n in D.frame_lengths(cfg)] == list(D.FRAME_EDGES) and min(D.frame_lengths(cfg)) == 4
    assert all(mc.num_frames(D.aligned_length(cfg, n)) == T for n, T in zip(D.frame_lengths(cfg), D.FRAME_EDGES))
    assert D.reference(dict(cfg, top_db=-1.0), 4).thr[0, 0, 0] == -np.inf
    # a NaN, or a value that is off where the floor is the dB rounding alone, is an error
    ref = D.reference(dict(cfg, top_db=80.0), 4)
    got = np.swapaxes(ref.M, 1, 2).astype(np.float32)
    assert (D.mfcc_error(got, ref).max(axis=(0, 1)) <= 1.0).all()
    got[S.ROW_ZERO, 3, 0] = np.nan
    assert np.isinf(D.mfcc_error(got, ref)[S.ROW_ZERO, 0, 3])


@pytest.mark.parametrize("name,top_db", CASES + [(name, -1.0) for name in PLANS])
def test_c_ref_per_coefficient(name, top_db):
    """C_ref[0] is the long same-sign float32 sum (about 1.8 at 40 filters, 4 at 80, 5 at 128), C_ref[1] lies between and
    C_ref[k >= 2] stays below 1, so those coefficients are held to MARGIN itself.  The fused kernels' arithmetic (fused32)
    is not in C_ref and stays inside the bound (measured 0.25 .. 0.57 of it; asserted below 0.75)."""
    cfg = dict(PLANS[name], top_db=top_db)
    c = D.c_ref(cfg)
    assert c.shape == (cfg["n_mfcc"],) and np.array_equal(D.bounds(cfg), D.MARGIN * np.maximum(c, 1.0)) and D.MARGIN == 4.0
    print(f"dct-cref {name} top_db={top_db:g} C_ref[0]={c[0]:.2f} C_ref[1]={c[1]:.2f} C_ref[2:]={c[2:].min():.2f}..{c[2:].max():.2f}")
    assert 1.0 < c[0] < 8.0 and 0.3 < c[1] < 3.0 and 0.05 < c[2:].min() and c[2:].max() < 1.0, c
    Dm = D.dct64(cfg["n_mels"], cfg["n_mfcc"])
    r = 0.0
    for n in D.frame_lengths(cfg):
        got = D.fused32(D.host_logmel(cfg, n), D.top_db_of(cfg), Dm)
        r = max(r, float((D.mfcc_error(got, D.reference(cfg, n)).max(axis=(0, 1)) / D.bounds(cfg)).max()))
    print(f"dct-fused32 {name} top_db={top_db:g}: c / bound = {r:.3g}")
    assert r <= 0.75, r


# ---- mutants: pipeline (b) with one defect each ------------------------------------------------------------------------------

def _f32_angle_table(n_mels, n_mfcc):
    """The DCT-II table with the angle formed and rounded in float32 before the (float64) cosine."""
    m, k = np.arange(n_mels, dtype=np.float32)[None, :], np.arange(n_mfcc, dtype=np.float32)[:, None]
    ang = (np.float32(np.pi) * (m + np.float32(0.5)) * k / np.float32(n_mels)).astype(np.float32)
    T = np.cos(ang.astype(np.float64)) * np.sqrt(2.0 / n_mels)
    T[0] *= np.sqrt(0.5)
    return T


def mutants(cfg, n):
    """{name: MFCC [B, n_mfcc, T]} of the float32 sequential pipeline with one piece replaced."""
    lm, top_db = D.host_logmel(cfg, n), np.float32(D.top_db_of(cfg))
    Dm = D.dct64(cfg["n_mels"], cfg["n_mfcc"])
    mx = D.clip_max32(lm)
    x = D.clamp32(lm, top_db)
    out = {}
    early = lm[:, :, :-1].reshape(lm.shape[0], -1).max(-1) if lm.shape[2] > 1 else mx
    out["max-without-last-frame"] = D.sequential32(D.clamp32(lm, top_db, thr=early - top_db), Dm)
    out["top_db+0.01"] = D.sequential32(D.clamp32(lm, top_db, thr=mx - np.float32(top_db + np.float32(0.01))), Dm)
    out["top_db+0.001"] = D.sequential32(D.clamp32(lm, top_db, thr=mx - np.float32(top_db + np.float32(0.001))), Dm)
    y = x.copy()
    y[:, -1, :] = lm[:, -1, :]
    out["last-filter-unclamped"] = D.sequential32(y, Dm)
    y = x.copy()
    y[:, :, 0] = lm[:, :, 0]
    out["first-frame-unclamped"] = D.sequential32(y, Dm)
    out["table-10-bits"] = D.sequential32(x, Dm.astype(np.float16))
    out["table-float32-angle"] = D.sequential32(x, _f32_angle_table(cfg["n_mels"], cfg["n_mfcc"]))
    return out


@pytest.mark.parametrize("name,top_db", CASES)
def test_every_mutant_is_rejected(name, top_db):
    cfg = dict(PLANS[name], top_db=top_db)
    bound = D.bounds(cfg)
    worst = {}
    for n in D.frame_lengths(cfg):
        ref = D.reference(cfg, n)
        for mutant, got in mutants(cfg, n).items():
            r = float((D.mfcc_error(got, ref).max(axis=(0, 1)) / bound).max())     # rejected: at least one coefficient beyond
            worst[mutant] = max(worst.get(mutant, 0.0), r)
    for mutant, r in sorted(worst.items()):
        print(f"dct-mutant {name} top_db={top_db:g} {mutant}: c / bound = {r:.3g}")
    required = {"max-without-last-frame", "top_db+0.01", "last-filter-unclamped", "first-frame-unclamped", "table-10-bits"}
    if top_db == 40.0 or cfg["n_mels"] == 128:
        required.add("top_db+0.001")
    assert required | {"top_db+0.001", "table-float32-angle"} == set(worst)
    for mutant in sorted(required):
        assert worst[mutant] > 1.0, f"{name} top_db {top_db:g}: {mutant} passes (c = {worst[mutant]:.3g} of the bound)"
    assert worst["table-10-bits"] > 10.0
    # what the bound does not see, said as such: the float32-angle table is an honest float32 table
    assert worst["table-float32-angle"] <= 1.0, worst["table-float32-angle"]


def test_mfcc_close_lets_a_threshold_off_by_0_001_db_through():
    """The gap: the case clips of C1 at 65 frames through the sequential pipeline with top_db + 0.001.  c0 of a frame that is
    clamped throughout moves by 0.001 sqrt(n_mels) = 0.006.  The impulse clips have such frames on the amin floor (every
    frame that does not hold the impulse: c0 = -600): mfcc_close allows 0.06 there and accepts all four clips, the
    per-coefficient bound rejects all four.  (The step clip's threshold lies near 0 dB, so its clamped c0 is small and
    mfcc_close's absolute term sees it too; the tones' and the constant's frames carry filters at the edge of the leakage
    whose own log-mel floor is a fraction of a dB, so neither check sees 0.001 dB there.)  A clip that does not clamp is
    accepted by both."""
    cfg = dict(PLANS["c1"], top_db=80.0)
    n = D.frame_lengths(cfg)[7]
    good = D.host_mfccs(cfg, n)[1]
    bad = mutants(cfg, n)["top_db+0.001"]
    ref = D.reference(cfg, n)
    clamps, _ = D.clamp_census(ref)

    def accepted(b):
        try:
            mfcc_close(bad[b], good[b], f"clip {b}")
        except AssertionError:
            return False
        return True

    old = np.array([accepted(b) for b in range(S.N_CASES)])
    c = D.mfcc_error(bad, ref).max(axis=1) / D.bounds(cfg)      # [B, n_mfcc]
    rejected = c.max(-1) > 1.0
    assert not rejected[~clamps].any() and old[~clamps].all(), (c.max(-1), old)
    slipped = old & rejected
    assert slipped[S.ROW_IMP_LAST:S.ROW_IMP_LAST + 4].all() and rejected[S.ROW_STEP], (old, rejected)
