"""GPU: pYIN (modulation_mfcc_amd.pitch, csrc/mm_pitch.hip) beyond the one parameter set of test_gpu_pitch.py -- every
keyword of librosa.pyin at a non-default value, more Viterbi states than threads, band half-widths 0..50, one to three
frames, up to six 64-trough chunks per frame, more than one 16 384-frame CMND chunk, strided rows, the numpy wrapper,
fill_na, and the host-side refusals.  The reference is tests/pyin_oracle.py throughout.

Every oracle result is computed once per (signal, keywords) and shared (``_oracle``).

Measured on an MI355X when these were written: the CMND error of the sweep is 6e-17 .. 1.1e-14 of the row maximum (the
largest at fmin=C2, fmax=C7, where the oracle's FFT autocorrelation is itself 2e-15 away from a longdouble direct sum),
observations and voiced_prob within 8e-16: the project's 1e-12 bounds hold for every win_length and frame_length here."""
import ctypes as C

import numpy as np
import pytest
import torch

import pyin_oracle as O
from modulation_mfcc_amd import _lib, pitch, get_f0, pyin_batch

pytestmark = pytest.mark.gpu

DTYPES = [np.float32, np.float64]
CHUNK_FRAMES = 16384                    # kCmndChunkFrames of mm_pitch.hip
_CMND_KEYS = ("fmin", "fmax", "frame_length", "win_length", "hop_length", "center")
_NOT_RECORDS = ("center", "pad_mode", "fill_na")


def _dev(y, gpu):
    return torch.from_numpy(np.ascontiguousarray(y)).to(gpu)


def _nn(t):
    return torch.nan_to_num(t.double(), nan=-1.0)


def _tile_frames(z):
    """cmnd_tile_frames of mm_pitch.hip: frames per CMND workgroup, the most (<= 16) whose LDS fits 64 KiB."""
    p1 = z["max_period"] + 1
    for F in range(16, 0, -1):
        span = (F - 1) * z["hop_length"] + z["win_length"] + z["max_period"] + 1
        if 8 * (span + 8 + F * p1) <= 65536:
            return F
    return 0


def _trough_counts(cmnd):
    out = np.empty(len(cmnd), dtype=int)
    for i, fr in enumerate(cmnd):
        m = O.localmin(fr)
        m[0] = fr[0] < fr[1]
        out[i] = m.sum()
    return out


_ORACLE = {}


def _oracle(y, sr, kw, decode="dense"):
    """Stages, decoded states and (f0, voiced, voiced_prob) of the oracle; cached, callers must not modify the result."""
    key = (y.dtype.str, np.ascontiguousarray(y).tobytes(), sr, decode, tuple(sorted((k, str(v)) for k, v in kw.items())))
    if key not in _ORACLE:
        skw = {k: v for k, v in kw.items() if k != "fill_na"}
        st = O.pyin_stages(y, sr=sr, **skw)
        nb = st["sizes"]["n_bins"]
        if decode == "dense":
            sw = O.viterbi_dense(st["obs"], st["A"], st["p_init"])
        else:
            sw = O.viterbi_banded(st["obs"], st["A"], st["p_init"], nb)
        f0w, vw, vpw = O.finish(sw, st, kw["fmin"], kw.get("fill_na", np.nan))
        k, j = np.nonzero(st["A"][:nb, :nb])
        tr = _trough_counts(st["cmnd"])
        sizes = dict(st["sizes"], S=2 * nb, H=int(np.abs(k - j).max()), F=_tile_frames(st["sizes"]),
                     troughs=int(tr.max()), chunks=-(-st["sizes"]["n_frames"] // CHUNK_FRAMES))
        _ORACLE[key] = dict(st=st, states=sw, f0=f0w, voiced=vw, vprob=vpw, sizes=sizes, troughs=tr)
    return _ORACLE[key]


def _four_checks(gpu, y, sr, kw, cmnd_bound=1e-12):
    """(a) CMND, (b) observations, (c) decode against the oracle's dense Viterbi, (d) device states against the dense
    Viterbi of the device's own observations.  A non-constant pad_mode is padded on the host for the stage calls."""
    ref = _oracle(y, sr, kw)
    st, z = ref["st"], ref["sizes"]
    print("sizes", {k: z[k] for k in ("n_bins", "S", "H", "F", "troughs", "n_frames", "chunks", "max_period")})
    x = _dev(y, gpu)
    f0, v, vp, s = pyin_batch(x, sr, return_states=True, **kw)
    assert f0.device.type == "cuda" and f0.dtype == torch.float64
    s = s.cpu().numpy()
    # (a) and (b): the stages, with the case's keywords
    ckw = {k: kw[k] for k in _CMND_KEYS if k in kw}
    ys = y
    if kw.get("pad_mode", "constant") != "constant" and kw.get("center", True):
        ys = np.pad(y, kw.get("frame_length", 2048) // 2, mode=kw["pad_mode"])
        ckw["center"] = False
    cm = pitch.pyin_cmnd(_dev(ys, gpu), sr, **ckw)
    want = st["cmnd"]
    assert cm.shape == want.shape
    err_a = np.abs(cm.cpu().numpy() - want).max() / (np.abs(want).max() + 1e-300)
    rkw = {k: v for k, v in kw.items() if k not in _NOT_RECORDS}
    cnt, bins, probs, vp2 = (a.cpu().numpy() for a in pitch.pyin_records(cm, sr, **rkw))
    nb = z["n_bins"]
    obs = np.zeros_like(st["obs"])
    for t in range(len(cnt)):
        obs[bins[t, :cnt[t]], t] = probs[t, :cnt[t]]
    obs[nb:] = (1 - vp2)[None] / nb
    err_b = np.abs(obs - st["obs"]).max()
    err_vp = np.abs(vp.cpu().numpy() - ref["vprob"]).max()
    print(f"cmnd err / max {err_a:.3e} (bound {cmnd_bound:.1e}), obs err {err_b:.3e}, voiced_prob err {err_vp:.3e}, "
          f"voiced {int(ref['voiced'].sum())}/{len(s)}")
    assert err_a <= cmnd_bound
    assert err_b <= 1e-12
    # (c) voicing, f0 and every voiced state are the oracle's
    assert np.array_equal(v.cpu().numpy(), ref["voiced"])
    np.testing.assert_array_equal(f0.cpu().numpy(), ref["f0"])
    bad = np.nonzero((s != ref["states"]) & ref["voiced"])[0]
    assert len(bad) == 0, f"{len(bad)} voiced frames differ, first {bad[:5]}"
    assert err_vp <= 1e-12
    # (d) the device decode is the dense Viterbi of the device's own observations, state for state
    np.testing.assert_array_equal(s, O.viterbi_dense(obs, st["A"], st["p_init"]))
    return ref


# ---------------------------------------------------------------------------------------------------------------------
# 1. parameter sweep
# ---------------------------------------------------------------------------------------------------------------------
_BASE = dict(fmin=75, fmax=600, hop_length=160)
# id: (signal kind, sr, seconds), keywords, sizes the case must reach
SWEEP = {
    "c01_C2_C7_hop512": (("glide", 22050, 1.0), dict(fmin=65.406, fmax=2093.0), dict(n_bins=601, S=1202, H=50, n_frames=44)),
    "c02_resolution_0.05": (("glide", 16000, 1.0), dict(_BASE, resolution=0.05), dict(n_bins=721, S=1442, H=40)),
    "c03_resolution_0.3": (("glide", 16000, 1.0), dict(_BASE, resolution=0.3), dict(nbps=4, n_bins=145, H=8)),
    "c04_hop16_single_source_band": (("glide", 16000, 0.3), dict(fmin=75, fmax=600, hop_length=16),
                                     dict(width=1, H=0, n_frames=301)),
    "c05_frame512_sr8000": (("glide", 8000, 2.0), dict(frame_length=512, hop_length=40, fmin=100, fmax=500),
                            dict(n_bins=279, max_period=80, n_frames=401)),
    "c06_win512": (("glide", 16000, 1.0), dict(_BASE, win_length=512), dict(win_length=512, max_period=214)),
    "c07_win1500": (("glide", 16000, 1.0), dict(_BASE, win_length=1500), dict(win_length=1500, max_period=214)),
    "c08_center_false": (("glide", 16000, 1.0), dict(_BASE, center=False), dict(n_frames=88)),
    "c09_every_probability_keyword": (("glide", 16000, 1.0),
                                      dict(_BASE, n_thresholds=37, beta_parameters=(3, 10), boltzmann_parameter=3,
                                           switch_prob=0.05, no_trough_prob=0.1, max_transition_rate=60.0), dict(H=35)),
    "c10_noise_44100_fmin45": (("noise", 44100, 0.5), dict(fmin=45, fmax=600, hop_length=220),
                               dict(max_period=980)),
}


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", sorted(SWEEP))
def test_parameter_sweep_against_oracle(gpu, case, dtype):
    (kind, sr, seconds), kw, reach = SWEEP[case]
    y = O.synth(kind, sr, seconds, dtype)
    ref = _oracle(y, sr, kw)
    for k, v in reach.items():
        assert ref["sizes"][k] == v, (k, ref["sizes"][k], v)
    if case.startswith("c10"):
        # five or more 64-trough chunks of the candidate kernel really run; nothing is voiced, so (d) carries the decode
        assert pitch.max_troughs(ref["sizes"]["min_period"], ref["sizes"]["max_period"]) == 455
        assert ref["sizes"]["troughs"] > 256
        assert not ref["voiced"].any()
    _four_checks(gpu, y, sr, kw)


@pytest.mark.parametrize("pad_mode,dtype", [("reflect", np.float32), ("edge", np.float64), ("wrap", np.float32)])
def test_pad_modes_against_oracle(gpu, pad_mode, dtype):
    y = O.synth("glide", 16000, 1.0, dtype)
    # the device pads with torch; the padded signal is np.pad's, sample for sample
    got = pitch._pad_center(_dev(y, gpu)[None], 2048, pad_mode)[0].cpu().numpy()
    np.testing.assert_array_equal(got, np.pad(y, 1024, mode=pad_mode))
    _four_checks(gpu, y, 16000, dict(_BASE, pad_mode=pad_mode))


# ---------------------------------------------------------------------------------------------------------------------
# 2. one, two and three frames
# ---------------------------------------------------------------------------------------------------------------------
FEW = {1: 1, 2: 1, 159: 1, 160: 2, 161: 2, 321: 3}          # samples -> frames at hop 160


# The frames above are mostly padding and decode as unvoiced.  Whole frames of the glide 64 ms apart are voiced, each in
# another bin (H = 140), so an observation row read from the wrong buffer changes the states.
_FAR = dict(fmin=75, fmax=600, hop_length=1024, center=False)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", sorted(FEW))
def test_fewest_frames(gpu, n, dtype):
    y = O.synth("glide", 16000, 1.0, dtype)[4000:4000 + n]
    ref = _four_checks(gpu, y, 16000, _BASE)
    assert ref["sizes"]["n_frames"] == FEW[n]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("T", [1, 2, 3])
def test_fewest_frames_voiced(gpu, T, dtype):
    y = O.synth("glide", 16000, 1.0, dtype)[1000:1000 + 2048 + 1024 * (T - 1)]
    ref = _four_checks(gpu, y, 16000, _FAR)
    assert ref["sizes"]["n_frames"] == T and ref["sizes"]["H"] == 140
    # frame 0 is unvoiced by p_init; every later frame is voiced, in a bin of its own
    assert not ref["voiced"][0] and ref["voiced"][1:].all() and len(set(ref["states"])) == T


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", sorted(FEW))
def test_fewest_frames_six_row_batch(gpu, n, dtype):
    g = O.synth("glide", 16000, 1.0, dtype)
    z = O.synth("noise", 16000, 1.0, dtype, seed=3)
    rows = np.stack([g[4000:4000 + n], g[9000:9000 + n], z[:n], g[15000:15000 + n], np.zeros(n, dtype), g[6500:6500 + n]])
    out = pyin_batch(_dev(rows, gpu), 16000, return_states=True, **_BASE)
    assert out[0].shape == (6, FEW[n])
    for i in range(6):
        one = pyin_batch(_dev(rows[i], gpu), 16000, return_states=True, **_BASE)
        for a, b in zip(out, one):
            assert torch.equal(_nn(a[i]), _nn(b)), f"row {i}"
        ref = _oracle(rows[i], 16000, _BASE)
        assert np.array_equal(out[1][i].cpu().numpy(), ref["voiced"])
        np.testing.assert_array_equal(out[0][i].cpu().numpy(), ref["f0"])
        s = out[3][i].cpu().numpy()
        assert np.array_equal(s[ref["voiced"]], ref["states"][ref["voiced"]])
        assert np.abs(out[2][i].cpu().numpy() - ref["vprob"]).max() <= 1e-12


_D_KW = dict(fmin=75, fmax=600, hop_length=160, resolution=0.05)       # 721 bins, 1442 states, H 40


def _check_decode_of_records(gpu, rows):
    """mm_pyin_decode (the Viterbi kernel alone, through the C ABI) on records given as rows[b][t] = [(bin, prob), ...]
    -> device states [B, T], each row checked against the dense Viterbi of the same observations."""
    p, z = pitch.pyin_params(2048, 16000, **_D_KW)
    tabs = pitch._tables(p, z, 0.01, (2, 18), 2, gpu)
    p.band_h = tabs.H
    nb, R, B, T = z["n_bins"], int(p.max_troughs), len(rows), len(rows[0])
    assert 2 * nb == 1442 and tabs.H == 40
    A = O.transition_full(nb, z["width"], 0.01)
    p_init = np.zeros(2 * nb)
    p_init[nb:] = 1 / nb
    count = np.zeros((B, T), np.int32)
    bins = np.zeros((B, T, R), np.int32)
    probs = np.zeros((B, T, R))
    vp = np.zeros((B, T))
    obs = np.zeros((B, 2 * nb, T))
    for b in range(B):
        for t, cands in enumerate(rows[b]):
            k = len(cands)
            count[b, t] = k
            bins[b, t, :k] = [c[0] for c in cands]
            probs[b, t, :k] = [c[1] for c in cands]
            obs[b, bins[b, t, :k], t] = probs[b, t, :k]
            vp[b, t] = min(max(obs[b, :nb, t].sum(), 0), 1)
            obs[b, nb:, t] = (1 - vp[b, t]) / nb
    d = [_dev(a.reshape(B * T, -1), gpu) for a in (count, bins, probs, vp)]
    states = torch.empty((B, T), dtype=torch.int32, device=gpu)
    f0 = torch.empty((B, T), dtype=torch.float64, device=gpu)
    voiced = torch.empty((B, T), dtype=torch.uint8, device=gpu)
    lib = _lib.load()
    ws = torch.empty(int(lib.mm_pyin_decode_workspace_bytes(C.byref(p), B, T)), dtype=torch.uint8, device=gpu)
    with torch.cuda.device(gpu):
        _lib.check(lib.mm_pyin_decode(C.byref(p), C.byref(tabs.c), *(a.data_ptr() for a in d), B, T, states.data_ptr(),
                                      f0.data_ptr(), voiced.data_ptr(), ws.data_ptr(), ws.numel(),
                                      C.c_void_p(torch.cuda.current_stream(gpu).cuda_stream)), "mm_pyin_decode")
    s = states.cpu().numpy()
    freqs = pitch.pitch_freqs(75, nb, z["nbps"])
    want = np.stack([O.viterbi_dense(obs[b], A, p_init) for b in range(B)])
    for b in range(B):
        np.testing.assert_array_equal(s[b], want[b], err_msg=f"row {b}")
        np.testing.assert_array_equal(voiced[b].cpu().numpy().astype(bool), want[b] < nb)
        np.testing.assert_array_equal(f0[b].cpu().numpy(), np.where(want[b] < nb, freqs[want[b] % nb], np.nan))
    return s, want, vp, nb


@pytest.mark.parametrize("T", [1, 2, 3, 40])
def test_decode_of_random_records_with_more_states_than_threads(gpu, T):
    """A few candidates per frame at random bins, exact ties in row 1, voiced_prob == 1 frames: jumps far outside the
    band at 1442 states.  Three rows side by side."""
    rng = np.random.default_rng(T)
    rows = []
    for b in range(3):
        row = []
        for t in range(T):
            k = int(rng.integers(0, 4))
            bb = rng.choice(721, size=k, replace=False)
            pr = rng.dirichlet(np.ones(k)) * (1.0 if rng.random() < 0.3 else rng.random()) if k else np.zeros(0)
            if b == 1 and k:
                pr[:] = pr[0]                                 # exact ties between bins
            row.append(list(zip(bb.tolist(), pr.tolist())))
        rows.append(row)
    s, _, vp, nb = _check_decode_of_records(gpu, rows)
    if T == 40:
        assert (s >= 1024).any() and (s < nb).any() and (vp == 1).any()


def test_decode_jumps_out_of_a_state_beyond_the_first_1024(gpu):
    """The out-of-band source g and the last state, each at a state index >= 1024 (the second state of a thread).
    Row 0: two certain candidates at bin 700, then no candidate -- an unvoiced state near bin 700 (index > 1400) is the
    one best state -- then two certain candidates at bin 300, far outside the band: the only way in is g, which the
    backtrack must find.  Row 1 ends unvoiced at bin 700, so the final argmax is at state 1421."""
    rows = [[[], [(700, 1.0)], [(700, 1.0)], [], [(300, 1.0)], [(300, 1.0)]],
            [[], [], [], [(700, 1.0)], [(700, 1.0)], []]]
    s, want, _, nb = _check_decode_of_records(gpu, rows)
    assert want[0].tolist()[1:3] == [700, 700] and want[0][3] >= 1024 and want[0].tolist()[4:] == [300, 300]
    assert want[1].tolist()[3:] == [700, 700, nb + 700] and nb + 700 >= 1024


# ---------------------------------------------------------------------------------------------------------------------
# 3. more than one CMND chunk
# ---------------------------------------------------------------------------------------------------------------------
C5 = dict(frame_length=512, hop_length=40, fmin=100, fmax=500)
C5_SR = 8000
_ROW_KINDS = ["glide", "noise", "sine200", "fade", "silence", "sine800", "glide"]


def _c5_row_length():
    """7 rows of about 100 000 samples: the chunk boundary (flat frame 16 384) inside row 6 and inside a CMND tile."""
    n = 100000
    while True:
        z = O.sizes(n, C5_SR, C5["fmin"], C5["fmax"], C5["frame_length"], None, C5["hop_length"])
        at = CHUNK_FRAMES - 6 * z["n_frames"]
        if 0 < at < z["n_frames"] and at % _tile_frames(z) != 0:
            return n, z, at
        n += C5["hop_length"]


_C5_ROWS = {}


def _c5_rows():
    if not _C5_ROWS:
        n, z, at = _c5_row_length()
        rows = np.stack([O.synth(k, C5_SR, n / C5_SR, np.float32, seed=10 + i) for i, k in enumerate(_ROW_KINDS)])
        assert rows.shape == (7, n)
        _C5_ROWS.update(rows=rows, z=z, at=at)
    return _C5_ROWS["rows"], _C5_ROWS["z"], _C5_ROWS["at"]


_C5_WHOLE = {}


def _c5_whole(gpu):
    if not _C5_WHOLE:
        rows, _, _ = _c5_rows()
        _C5_WHOLE["out"] = pyin_batch(_dev(rows, gpu), C5_SR, return_states=True, **C5)
    return _C5_WHOLE["out"]


def test_two_chunk_batch_equals_single_rows_and_oracle(gpu):
    rows, z, at = _c5_rows()
    T = z["n_frames"]
    assert rows.shape[1] == 100000 and T == 2501 and 7 * T == 17507 > CHUNK_FRAMES
    F = _tile_frames(z)
    print(f"rows {rows.shape}, frames/row {T}, flat frames {7 * T}, F {F}, chunk boundary in row 6 at frame {at}")
    assert at == 1378 and at % F != 0
    out = _c5_whole(gpu)
    for i in range(7):
        one = pyin_batch(_dev(rows[i], gpu), C5_SR, return_states=True, **C5)        # one chunk
        for name, a, b in zip(("f0", "voiced", "voiced_prob", "states"), out, one):
            d = torch.nonzero(_nn(a[i]) != _nn(b)).flatten()
            assert d.numel() == 0, f"row {i} {name}: {d.numel()} frames differ, first {d[:5].tolist()}"
    for i in (0, 6):
        ref = _oracle(rows[i], C5_SR, C5, decode="banded")
        v = ref["voiced"]
        assert v.sum() > 500                                    # a glide: the voiced comparison is not empty
        s = out[3][i].cpu().numpy()
        assert np.array_equal(out[1][i].cpu().numpy(), v)
        assert np.array_equal(s[v], ref["states"][v])
        np.testing.assert_array_equal(out[0][i].cpu().numpy(), ref["f0"])
        assert np.abs(out[2][i].cpu().numpy() - ref["vprob"]).max() <= 1e-12


def test_two_chunk_single_row_against_banded_oracle(gpu):
    y = O.synth("glide", C5_SR, 85.0, np.float32)
    ref = _oracle(y, C5_SR, C5, decode="banded")
    assert ref["sizes"]["n_frames"] == 17001 and ref["sizes"]["chunks"] == 2
    v = ref["voiced"]
    print("voiced frames", int(v.sum()), "sizes", ref["sizes"])
    assert v.sum() > 10000 and v[CHUNK_FRAMES - 40:CHUNK_FRAMES + 40].any()     # voiced frames at the chunk boundary
    f0, vd, vp, s = pyin_batch(_dev(y, gpu), C5_SR, return_states=True, **C5)
    s = s.cpu().numpy()
    assert np.array_equal(vd.cpu().numpy(), v)
    assert np.array_equal(s[v], ref["states"][v])
    assert np.abs(vp.cpu().numpy() - ref["vprob"]).max() <= 1e-12


def test_two_chunk_batch_cut_into_three_row_calls(gpu, monkeypatch):
    rows, z, _ = _c5_rows()
    whole = _c5_whole(gpu)
    lib = _lib.load()
    p, _ = pitch.pyin_params(rows.shape[1], C5_SR, **C5)
    # room for three rows of scratch, not for four
    monkeypatch.setattr(pitch, "PYIN_WS_BYTES", int(lib.mm_pyin_workspace_bytes(C.byref(p), 4, rows.shape[1])) - 1)
    real, calls = lib.mm_pyin_f32, []

    def counted(*a):
        calls.append(a[3])
        return real(*a)

    monkeypatch.setattr(lib, "mm_pyin_f32", counted)
    parts = pyin_batch(_dev(rows, gpu), C5_SR, return_states=True, **C5)
    assert calls == [3, 3, 1]
    for a, b in zip(whole, parts):
        assert torch.equal(_nn(a), _nn(b))


def test_strided_rows_equal_contiguous(gpu):
    rows, _, _ = _c5_rows()
    n = rows.shape[1]
    whole = _c5_whole(gpu)
    big = torch.full((14, n), 0.25, dtype=torch.float32, device=gpu)
    big[::2] = _dev(rows, gpu)
    wide = torch.full((7, n + 5), 0.25, dtype=torch.float32, device=gpu)
    wide[:, :n] = _dev(rows, gpu)
    for view, pitch_ in ((big[::2], 2 * n), (wide[:, :n], n + 5)):
        assert view.stride() == (pitch_, 1) and not view.is_contiguous()
        got = pyin_batch(view, C5_SR, return_states=True, **C5)
        for a, b in zip(whole, got):
            assert torch.equal(_nn(a), _nn(b))
        cm = pitch.pyin_cmnd(view[5:], C5_SR, **C5)
        assert torch.equal(cm, pitch.pyin_cmnd(view[5:].contiguous(), C5_SR, **C5))


# ---------------------------------------------------------------------------------------------------------------------
# 4. wrappers and fill_na
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_pyin_numpy_wrapper_librosa_defaults(gpu, dtype):
    y = O.synth("glide", 22050, 1.0, dtype)
    ref = _oracle(y, 22050, dict(fmin=65.406, fmax=2093.0))
    out = pitch.pyin(y, fmin=65.406, fmax=2093.0)
    assert len(out) == 3 and all(isinstance(o, np.ndarray) for o in out)
    f0, v, vp = out
    assert f0.dtype == np.float64 and v.dtype == np.bool_ and f0.shape == (44,)
    assert ref["voiced"].any()
    np.testing.assert_array_equal(v, ref["voiced"])
    np.testing.assert_array_equal(f0, ref["f0"])
    assert np.abs(vp - ref["vprob"]).max() <= 1e-12
    # [B, n] in, [B, frames] out
    f2, v2, _ = pitch.pyin(np.stack([y, y[::-1]]), fmin=65.406, fmax=2093.0)
    assert f2.shape == (2, 44)
    np.testing.assert_array_equal(f2[0], f0)
    np.testing.assert_array_equal(v2[0], v)


@pytest.mark.parametrize("dtype", DTYPES)
def test_fill_na_none_and_numeric(gpu, dtype):
    y = O.synth("glide", 16000, 1.0, dtype)
    ref = _oracle(y, 16000, _BASE)
    nb = ref["sizes"]["n_bins"]
    uv = ~ref["voiced"]
    assert uv.any() and ref["voiced"].any()
    f0, v, vp, s = (a.cpu().numpy() for a in pyin_batch(_dev(y, gpu), 16000, fill_na=None, return_states=True, **_BASE))
    freqs = O.finish(np.arange(nb), ref["st"], 75)[0]
    assert np.isfinite(f0).all()
    np.testing.assert_array_equal(f0, freqs[s % nb])
    assert np.array_equal(v, ref["voiced"])
    want = _oracle(y, 16000, dict(_BASE, fill_na=None))
    assert np.isfinite(want["f0"]).all()
    print("unvoiced frames", int(uv.sum()), "of which the decoded bin is the oracle's", int(((s == want["states"]) & uv).sum()))
    np.testing.assert_array_equal(f0, want["f0"])
    f0z, vz, _ = (a.cpu().numpy() for a in pyin_batch(_dev(y, gpu), 16000, fill_na=0.0, **_BASE))
    wz = _oracle(y, 16000, dict(_BASE, fill_na=0.0))
    np.testing.assert_array_equal(f0z, wz["f0"])
    assert np.array_equal(f0z == 0.0, uv) and np.array_equal(vz, ref["voiced"])


def test_get_f0_non_default_pyin_keywords(gpu):
    sr = 16000
    y = O.synth("glide", sr, 3.0, np.float64)
    f0, f0t = get_f0(y, sr, method="pyin", outFiltCutOff=[12], pyinframe_length=1024, pyinwin_length=400, resolution=0.2,
                     n_thresholds=50, pyincenter=False)
    wf, wt = O.get_f0(y, sr, outFiltCutOff=[12], frame_length=1024, win_length=400, resolution=0.2, n_thresholds=50,
                      center=False)
    assert f0.shape == wf.shape == (1 + (len(y) - 1024) // 160,)
    np.testing.assert_array_equal(f0t, wt)
    assert np.abs(f0 - wf).max() <= 1e-9 * np.abs(wf).max()


def test_get_f0_pad_mode_reflect(gpu):
    sr = 16000
    y = O.synth("glide", sr, 3.0, np.float32)
    f0, f0t = get_f0(y, sr, method="pyin", outFiltCutOff=[12], pyinpad_mode="reflect")
    wf, wt = O.get_f0(y, sr, outFiltCutOff=[12], pad_mode="reflect")
    assert f0.shape == wf.shape
    np.testing.assert_array_equal(f0t, wt)
    assert np.abs(f0 - wf).max() <= 1e-9 * np.abs(wf).max()
    # the padding matters: the zero-padded track differs
    zf, _ = O.get_f0(y, sr, outFiltCutOff=[12])
    assert np.abs(zf - wf).max() > 1e-6 * np.abs(wf).max()


# ---------------------------------------------------------------------------------------------------------------------
# 5. refusals on the host
# ---------------------------------------------------------------------------------------------------------------------
_ENTRY_POINTS = ("mm_pyin_f32", "mm_pyin_f64", "mm_pyin_cmnd", "mm_pyin_candidates", "mm_pyin_decode")


@pytest.fixture
def no_launch(monkeypatch):
    """Every library entry point that launches a pYIN kernel fails the test when it is reached."""
    lib = _lib.load()

    def reached(*a):
        raise AssertionError("a launching entry point was reached")

    for name in _ENTRY_POINTS:
        monkeypatch.setattr(lib, name, reached)


def test_device_limit_is_refused_before_any_launch(gpu, no_launch):
    kw = dict(frame_length=4096, fmin=30, fmax=600, hop_length=240)
    z = O.sizes(48000, 48000, 30, 600, 4096, None, 240)
    assert pitch.max_troughs(z["min_period"], z["max_period"]) == 762          # > 512 trough slots of a wave
    x = torch.zeros(48000, dtype=torch.float32, device=gpu)
    with pytest.raises(NotImplementedError):
        pyin_batch(x, 48000, **kw)
    with pytest.raises(NotImplementedError):
        pitch.pyin_cmnd(x, 48000, **kw)
    with pytest.raises(NotImplementedError):
        pitch.pyin_params(48000, 48000, **kw)


def test_band_wider_than_bins_is_a_value_error(gpu, no_launch):
    y = O.synth("sine200", 16000, 0.5, np.float32)
    z = O.sizes(len(y), 16000, 150, 170, hop_length=160)
    assert z["width"] == 41 and z["n_bins"] == 22
    with pytest.raises(ValueError):
        O.pyin_dense(y, fmin=150, fmax=170, sr=16000, hop_length=160)
    with pytest.raises(ValueError):
        pyin_batch(_dev(y, gpu), 16000, fmin=150, fmax=170, hop_length=160)


def test_get_f0_narrow_quantiles_is_a_value_error(gpu):
    # a steady tone: the two quantiles of the first pass leave no room for the transition band in the second
    y = O.synth("sine200", 16000, 1.0, np.float64)
    with pytest.raises(ValueError):
        O.get_f0(y, 16000, minMaxQuant=[0.45, 0.55])
    with pytest.raises(ValueError):
        get_f0(y, 16000, method="pyin", outFiltCutOff=[12], minMaxQuant=[0.45, 0.55])


def test_too_short_without_centering_is_a_value_error(gpu, no_launch):
    x = torch.ones(2047, dtype=torch.float64, device=gpu)
    with pytest.raises(ValueError):
        pyin_batch(x, 16000, center=False, **_BASE)
    with pytest.raises(ValueError):
        pyin_batch(x[None].expand(3, 2047), 16000, center=False, **_BASE)


def test_expanded_rows_are_computed(gpu):
    y = O.synth("glide", 16000, 0.5, np.float32)
    x = _dev(y, gpu)[None].expand(3, len(y))
    assert x.stride() == (0, 1)
    one = pyin_batch(_dev(y, gpu), 16000, return_states=True, **_BASE)
    got = pyin_batch(x, 16000, return_states=True, **_BASE)
    for a, b in zip(got, one):
        assert a.shape == (3,) + b.shape
        for i in range(3):
            assert torch.equal(_nn(a[i]), _nn(b))
    cm = pitch.pyin_cmnd(x, 16000, **_BASE)
    assert torch.equal(cm[2], pitch.pyin_cmnd(_dev(y, gpu), 16000, **_BASE))
    # one row of such a view: its stride says nothing and is not handed on
    got1 = pyin_batch(x[1:2], 16000, return_states=True, **_BASE)
    for a, b in zip(got1, one):
        assert torch.equal(_nn(a[0]), _nn(b))
