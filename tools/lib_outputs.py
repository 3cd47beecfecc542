"""dev (GPU box): every output array of a fixed list of small cases on the library named by MODMFCC_LIB, saved to one .npz --
one process per library; two files are then compared bit for bit (a schedule move of a kernel must not change a bit).

    MODMFCC_LIB=$PWD/modulation_mfcc_amd/libmodmfcc_parent.so python tools/lib_outputs.py s16 parent.npz
    python tools/lib_outputs.py s16 branch.npz
    python tools/lib_outputs.py --compare parent.npz branch.npz

Case set `s16`: the smallest shapes that reach each code path of the staged n_fft-512 kernel (logmel512s_kernel) and the
matrix-pipe kernel.  n_fft 512, 16 kHz, win 400, 40 mel / 13 MFCC unless said otherwise.
Case set `tail`: every kernel of mm_tail.hip and its includes (tail_cases).
Case set `ragged`: every public *_ragged_batch function with host and with device lengths, and the four list front ends
(ragged_cases) -- for a change of the host code, run on two checkouts with the same library.
Case set `welch`: every instantiation and path of the Welch power and cross spectrum kernels (welch_cases).
Case set `gapfill`: every interp_NAN kind through the five gap-filling calls -- shapes, types, layouts, rows with too few valid
samples, counts, host inputs, get_f0 / get_f0_batch -- with every refusal's type and text (gapfill_cases); for a change of
the host code, run on two checkouts with the same library as well.
Case set `hilbert`: the three call paths of mm_hilbert.hip.inc (hilbert_cases), float32 and float64, contiguous rows, on the
oracle's case rows (tests/hilbert_oracle.py rows_for / take: the zero row is in).  Envelope: ENVELOPE_LENGTHS +
BLUESTEIN_LENGTHS with 1 / 2 / 5 / 37 rows, LONG_CASES with 5 float32 rows, test_many_rows' 256 x 1000, 625 x 1001 and
35 x 1000, nine rows of 625 / 9600 / 511 under a two-pair workspace bound, a NaN row and an infinity row at 9600 (direct) and
511 (chirps).  Forward transform: FORWARD_LENGTHS through calc.rfft_rows_long with 1 / 5 / 37 rows.  Ragged: RAGGED_M with
test_ragged's lengths.  Beyond 20 000 samples 5 rows only.  614 arrays, 211 MB: compare where they were written."""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np


def compare(a_path, b_path):
    a, b = np.load(a_path), np.load(b_path)
    bad = sorted(set(a.files) ^ set(b.files))
    bad += [k for k in a.files if k in b.files and
            (a[k].dtype != b[k].dtype or a[k].shape != b[k].shape or a[k].tobytes() != b[k].tobytes())]
    print("%d arrays, %d differ%s" % (len(a.files), len(bad), ": " + " ".join(bad) if bad else ""))
    return 1 if bad else 0


def clips(seed, batch, n, sr, quiet_every=0):
    """An amplitude-modulated tone in noise; every quiet_every-th clip with a tail 120 dB down (the top_db clamp fix-up runs)."""
    rng = np.random.default_rng(seed)
    t = np.arange(n, dtype=np.float64) / sr
    x = 0.05 * rng.standard_normal((batch, n), dtype=np.float32)
    x += (0.5 * (1.0 + 0.8 * np.sin(2 * np.pi * 4.0 * t)) * np.sin(2 * np.pi * 440.0 * t)).astype(np.float32)
    if quiet_every:
        x[quiet_every - 1::quiet_every, n // 2:] *= 1e-6
    return x


def s16_cases():
    import torch
    from modulation_mfcc_amd import MfccConfig, MfccPlan
    dev = torch.device("cuda", 0)
    out = {}
    base = dict(sr=16000.0, n_fft=512, win_length=400, hop_length=160, n_mels=40, n_mfcc=13, fmin=100.0, fmax=8000.0)

    def keep(name, **arrays):
        for k, v in arrays.items():
            out[name + "." + k] = v.cpu().numpy()

    def tile_mode(name, plan, d, power=True):
        """MODE 0 (power rows) and MODE 1 (log-mel rows + clip max, MFCC)"""
        if power:
            keep(name, stft_power=plan.stft_power(d))
        lm, mx = plan.logmel(d)
        keep(name, logmel=lm, clip_max=mx, mfcc=plan.mfcc(d))

    def plan_of(name, cfg=None, **kw):
        """a plan that the staged kernel takes with its DCT fused in: a case that dispatch sends elsewhere pins nothing"""
        plan = MfccPlan(cfg or MfccConfig(**{**base, **kw}))
        print(name, plan.kernel_path, "fused_dct", plan.fused_dct, flush=True)
        assert plan.kernel_path == "radix16-w16s" and plan.fused_dct, name
        return plan

    # staging groups per thread NR 1 / 2 / 3 / 4 (63 hop + 512 <= NR 4096): 10 240 samples = exactly 64 frames at hop 160,
    # + 4 = one more tile; 8 samples = a clip shorter than the centre pad; the third clip of three clamps
    for nr, hop in ((1, 50), (2, 100), (3, 160), (4, 240)):
        plan = plan_of("nr%d" % nr, hop_length=hop)
        for n in (10240, 10244, 8):
            tile_mode("nr%d.n%d" % (nr, n), plan, torch.from_numpy(clips(10 * nr + n % 7, 3, n, 16000, 3)).to(dev))
    # a window of at most 256 samples: the dft16_mid8 path (NR 1 / 2 only)
    plan = plan_of("halfwin", hop_length=50, win_length=250)
    tile_mode("halfwin", plan, torch.from_numpy(clips(50, 3, 10240, 16000, 3)).to(dev))
    # the reference's default call (10 kHz, win 250, hop 50, 128 mel up to 10 kHz): ONE log-mel tile (lt_single), the
    # skip-empty run tables and the analytic share of the filters above Nyquist.  W16 is not bit-equal to S16 here.
    plan = plan_of("refdefault", cfg=MfccConfig())
    tile_mode("refdefault", plan, torch.from_numpy(clips(51, 3, 10244, 10000, 3)).to(dev), power=False)
    # the template axes at NR 3
    tile_mode("odd", plan_of("odd", hop_length=161), torch.from_numpy(clips(52, 3, 10244, 16000, 3)).to(dev))
    tile_mode("pre", plan_of("pre", preemph=0.97), torch.from_numpy(clips(53, 3, 10244, 16000, 3)).to(dev))
    big = torch.zeros((3, 1 + 10241 + 2), dtype=torch.float32, device=dev)       # rows off a 16-byte boundary, n % 4 != 0
    big[:, 1:10242] = torch.from_numpy(clips(54, 3, 10241, 16000, 3)).to(dev)
    tile_mode("unal", plan_of("unal"), big[:, 1:10242])
    # the b32 exchange at NR 3 (the instantiations without the add-TID exchange).  The run table alone never excludes the
    # add-TID layout (setup_tile512: 10 880 bytes at 256 mel, 40 704 would be needed at NR 3); the fused-DCT layout does
    # (setup_s16f) where a log-mel tile layout has less than 2 KB to spare.  At hop 160, by a kernel trace over 41 .. 256
    # mel: 49 .. 52 mel (two log-mel tiles; 49 is the smallest) and 89 .. 92 mel (one tile).
    for nm in (49, 89):
        tile_mode("b32x.mel%d" % nm, plan_of("b32x.mel%d" % nm, n_mels=nm),
                  torch.from_numpy(clips(55, 3, 10244, 16000, 3)).to(dev), power=False)
    # mfcc_modspec on 256 clips, one in eight clamping.  16 000 samples (101 frames, n_mod 128): separate launches.
    # Clip mode (MODE 2, the tail inside the launch) takes at least a clip per CU and n_mod 512 / 1024: 48 000 samples
    # (301 frames) and 96 000 (601); 2048-point trajectories (164 000: 1026 frames) under the opt-in wider form.
    plan = plan_of("clip")
    for n in (16000, 48000, 96000, 1025 * 160):
        if n == 1025 * 160:
            plan.set_fuse_tail(2)
        d = torch.from_numpy(clips(56 + n % 5, 256, n, 16000, 8)).to(dev)
        n_mod = plan.cfg.mod_fft_len(plan.cfg.num_frames(n))
        print("clip.n%d fused_tail" % n, plan.fused_tail(256, n), "n_mod", n_mod, flush=True)
        assert n_mod == {16000: 128, 48000: 512, 96000: 1024}.get(n, 2048) and plan.fused_tail(256, n) == (n != 16000), n
        mfcc, mod = plan.mfcc_modspec(d)
        keep("clip.n%d" % n, mfcc=mfcc, mod=mod)
        del d, mfcc, mod
    # the matrix-pipe kernel: LDS-DMA staging (10 240) and register staging (10 241)
    plan = plan_of("m12")
    plan.set_variant("m12")
    assert plan.kernel_path == "radix16-m12"
    for n in (10240, 10241):
        dd = torch.from_numpy(clips(58, 3, n, 16000, 3)).to(dev)
        lm, mx = plan.logmel(dd)
        keep("m12.n%d" % n, logmel=lm, clip_max=mx, mfcc=plan.mfcc(dd))
    torch.cuda.synchronize()
    return out


def tail_cases():
    """Case set `tail`: every kernel of mm_tail.hip (sosfiltfilt on curves, the MFCC-change tail in its three forms and its
    ragged form, the banded stencil) at the smallest shape that reaches it."""
    import torch
    import scipy.signal
    from modulation_mfcc_amd import MfccConfig, MfccPlan, tail
    from modulation_mfcc_amd.calc import apply_stencil, apply_stencil_ragged, velocity_stencil
    from modulation_mfcc_amd.filters import fir_filtfilt_stencil, sosfiltfilt_batch, sosfiltfilt_ragged_batch
    dev = torch.device("cuda", 0)
    out = {}
    SEG = 1088                                  # MM_SEG_LEN: samples per segment of the segmented rows

    def keep(name, t):
        out[name] = t.cpu().numpy()

    def curves(seed, rows, n, dtype=np.float64):
        return torch.from_numpy(np.random.default_rng(seed).standard_normal((rows, n)).cumsum(axis=1).astype(dtype)).to(dev)

    # sosfiltfilt_batch.  1 - 4 sections: the segmented rows (instantiations 2 / 2 / 3 / 4), 3 rows a wave per segment, 130
    # (MM_ROW_MIN is 128) a workgroup per row; 5, 8, 16 sections: the time-major kernels (instantiations 6 / 8 / 16; the
    # sequential one -- the chunked form stops at 4 sections).  Lengths: padlen + 1, one segment exactly, one more, ~3000
    for ns in (1, 2, 3, 4, 5, 8, 16):
        sos = scipy.signal.butter(2 * ns, 0.2, output="sos")
        pad = 3 * (2 * ns + 1)
        for rows in (3, 130):
            for n in (pad + 1, SEG - 2 * pad, SEG - 2 * pad + 1, 3001):
                keep("sos.ns%d.r%d.n%d" % (ns, rows, n), sosfiltfilt_batch(curves(ns + n, rows, n), sos))
    sos = scipy.signal.butter(6, 0.05, output="sos")
    pad = 21
    # 18 501 samples are more than 16 segments: the row stream takes a second round
    keep("sos.long.r130", sosfiltfilt_batch(curves(1, 130, 18501), sos))
    keep("sos.long.r3", sosfiltfilt_batch(curves(2, 3, 18501), sos))
    for rows in (3, 130):                       # float32 rows, and a strided batch (every other row of a wider buffer)
        keep("sos.f32.r%d" % rows, sosfiltfilt_batch(curves(3, rows, 3001, np.float32), sos))
        keep("sos.strided.r%d" % rows, sosfiltfilt_batch(curves(4, rows, 2 * 3100)[:, 50:3051], sos))
    keep("sos.f32.ns5", sosfiltfilt_batch(curves(5, 3, 3001, np.float32), scipy.signal.butter(10, 0.2, output="sos")))
    # sosfiltfilt_ragged_batch: device lengths 1, padlen (refused: a NaN row), padlen + 1, a segment boundary, n_max
    for rows in (3, 130):
        n_max = 3 * SEG + 7
        lens = np.random.default_rng(rows).integers(pad + 1, n_max + 1, rows)
        lens[:3] = (1, SEG - 2 * pad, n_max)
        if rows > 3:
            lens[3:7] = (pad, pad + 1, SEG - 2 * pad + 1, 2 * SEG - 2 * pad)
        else:
            keep("sosrag.short.r3", sosfiltfilt_ragged_batch(curves(6, 3, n_max), torch.tensor([pad, pad + 1, 2 * SEG - 2 * pad], device=dev), sos))
        ld = torch.from_numpy(lens.astype(np.int64)).to(dev)
        for dt in (np.float64, np.float32):
            keep("sosrag.r%d.%s" % (rows, np.dtype(dt).name), sosfiltfilt_ragged_batch(curves(7, rows, n_max, dt), ld, sos))
        for ns in (2, 4):                       # (the lengths of this batch suit every padlen up to 21: four sections pad 27)
            s_ns = scipy.signal.butter(2 * ns, 0.05, output="sos")
            keep("sosrag.r%d.ns%d" % (rows, ns), sosfiltfilt_ragged_batch(curves(7, rows, n_max), torch.clamp(ld, min=28), s_ns))

    # mfcc_change_device on the shapes of tests/test_gpu_sos.py (segmented with a wave per segment, clip-resident in three
    # groups of rows, segmented with a workgroup per row) and a short clip; fused, and on the time-major kernels (chunked
    # at n_ext >= 256, sequential at 101 frames)
    base = dict(sr=16000.0, n_fft=512, win_length=400, hop_length=160, n_mels=40, n_mfcc=13, fmin=100.0, fmax=8000.0)
    sets = {"default": dict(outFiltCutOff=[12]), "sg": dict(diffMethod="sg", outFiltCutOff=[12]), "nofilt": dict(outFilter=None),
            "sec1v4": dict(filtOrd=2, outFiltLen=8, outFiltCutOff=[12]), "sec4v1": dict(filtOrd=8, outFiltLen=1, outFiltCutOff=[12]), "sec2": dict(filtOrd=4, outFiltLen=4, outFiltCutOff=[12])}
    plan = MfccPlan(MfccConfig(**base))
    for B, T in ((2, 5500), (3, 3001), (130, 5500), (3, 101)):
        m = torch.from_numpy(np.random.default_rng(4).standard_normal((B, 13, T)).cumsum(axis=2).astype(np.float32)).to(dev)
        for fuse in (True, False):
            prev = plan.set_fuse_tail(fuse)
            for name, kw in sets.items():
                if B < 128 or name in ("default", "sg"):
                    keep("chg.%dx%d.%s.%s" % (B, T, "fused" if fuse else "tm", name), tail.mfcc_change_device(plan, m, tStep=0.005, **kw))
            plan.set_fuse_tail(prev)
    # more than 64 rows after c0 on the time-major kernels: chg_norm_rows_kernel
    plan70 = MfccPlan(MfccConfig(**dict(base, n_mels=80, n_mfcc=70)))
    m = torch.from_numpy(np.random.default_rng(5).standard_normal((3, 70, 301)).cumsum(axis=2).astype(np.float32)).to(dev)
    plan70.set_fuse_tail(False)
    for name in ("default", "sg"):
        keep("chg.rows69.%s" % name, tail.mfcc_change_device(plan70, m, tStep=0.005, **sets[name]))
    # mfcc_change_ragged: frame counts 1, a refused one, padlen + 1, T_max; T_max 1001 takes the 12 rows in two groups
    for T in (301, 1001):
        fr = np.random.default_rng(T).integers(22, T + 1, 9)
        fr[:4] = (1, 15, 22, T)
        fd = torch.from_numpy(fr.astype(np.int64)).to(dev)
        m = torch.from_numpy(np.random.default_rng(6).standard_normal((9, 13, T)).cumsum(axis=2).astype(np.float32)).to(dev)
        for name in ("default", "sg", "nofilt", "sec1v4", "sec2"):
            keep("chgrag.T%d.%s" % (T, name), tail.mfcc_change_ragged_device(plan, m, fd, tStep=0.005, **sets[name]))

    # apply_stencil / apply_stencil_ragged: np.gradient, Savitzky-Golay window 5, a 6-tap FIR filtfilt
    x = curves(8, 5, 700)
    ld = torch.tensor([700, 1, 9, 350, 699], dtype=torch.int64, device=dev)
    stencils = {"grad": velocity_stencil(100.0, 1, "gradient")[0], "sg5": velocity_stencil(100.0, 1, "sg", width=5)[0],
                "fir6": fir_filtfilt_stencil(scipy.signal.firwin(6, 0.3))}
    for name, st in stencils.items():
        keep("stencil." + name, apply_stencil(x, st))
        keep("stencilrag." + name, apply_stencil_ragged(x, ld, st, 19 if name == "fir6" else 0))
    torch.cuda.synchronize()
    return out


RAGGED_LENS = [4000, 2500, 4000, 3100, 2500]


def ragged_list(dev):
    """Five clips at 16 kHz: numpy float32, numpy float64, numpy int16, device float32, device float64 -- two dtype groups,
    a repeated length within and across them, both return types."""
    import torch
    x = [clips(70 + i, 1, n, 16000)[0].astype(np.float64) for i, n in enumerate(RAGGED_LENS)]
    return [x[0].astype(np.float32), x[1], np.round(x[2] * 20000).astype(np.int16), torch.from_numpy(x[3].astype(np.float32)).to(dev),
            torch.from_numpy(x[4]).to(dev)]


def ragged_cases():
    """Case set `ragged`: only names the package exports, so that the same code runs on an older checkout."""
    import torch
    import scipy.signal
    import modulation_mfcc_amd as M
    dev = torch.device("cuda", 0)
    out = {}

    def flat(r):
        if isinstance(r, (tuple, list)):
            return [a for part in r for a in flat(part)]
        return [r.cpu().numpy()] if isinstance(r, torch.Tensor) else [r] if isinstance(r, np.ndarray) else []

    def keep(name, call):
        """every array of the call's result, in order; a refusal is kept as its type and text"""
        try:
            for k, a in enumerate(flat(call())):
                out["%s.%d" % (name, k)] = a
        except (ValueError, IndexError, TypeError, NotImplementedError) as e:
            out[name + ".error"] = np.frombuffer(("%s: %s" % (type(e).__name__, e)).encode(), dtype=np.uint8)
            print(name, "raised", type(e).__name__, e, flush=True)

    lens = np.array(RAGGED_LENS, dtype=np.int64)
    n_max = int(lens.max())
    x64 = np.full((5, n_max + 3), np.nan)
    for b, n in enumerate(lens):
        x64[b, :n] = clips(60 + b, 1, n, 16000)[0]
    rows = {"f32": torch.from_numpy(x64.astype(np.float32)).to(dev)[:, :n_max], "f64": torch.from_numpy(x64).to(dev)[:, :n_max]}
    cfg = M.MfccConfig(sr=16000.0, n_fft=512, win_length=400, hop_length=32, n_mels=40, n_mfcc=13, fmin=100.0, fmax=8000.0)
    sos = scipy.signal.butter(6, 0.05, output="sos")
    pyin = dict(fmin=100.0, fmax=500.0, frame_length=512, hop_length=32)
    for where in ("host", "dev"):
        L = lens if where == "host" else torch.from_numpy(lens).to(dev)
        f32, f64 = rows["f32"], rows["f64"]
        keep("mfcc." + where, lambda: M.mfcc_ragged_batch(f32, L, cfg))
        keep("modspec." + where, lambda: M.mfcc_modspec_ragged_batch(f32, L, cfg))
        for name, kw in (("iir", dict(outFiltCutOff=[12])), ("sg", dict(outFilter="sg", outFiltCutOff=[12], outFiltLen=7)), ("none", dict(outFilter=None))):
            keep("change.%s.%s" % (name, where), lambda: M.mfcc_change_ragged_batch(f32, L, cfg, **kw))
        for center in (True, False):
            keep("rms.c%d.%s" % (center, where), lambda: M.rms_ragged_batch(f32, L, 160, 32, center))
        for dt, x in rows.items():
            keep("hilbert.%s.%s" % (dt, where), lambda: M.hilbert_envelope_ragged_batch(x, L))
            for method in ("RMS", "Hilb"):
                keep("envelope.%s.%s.%s" % (method, dt, where), lambda: M.amplitude_envelope_ragged_batch(x, L, 16000, method=method, winLen=0.01, hopLen=0.002)[:2])
            keep("sos.%s.%s" % (dt, where), lambda: M.sosfiltfilt_ragged_batch(x, L, sos))
            keep("fir.%s.%s" % (dt, where), lambda: M.fir_filtfilt_ragged_batch(x, L, scipy.signal.firwin(31, 0.2)))
            keep("savgol.%s.%s" % (dt, where), lambda: M.savgol_ragged_batch(x, L, 21, 3))
            for name, kw in (("iir", dict(filt="iir", cutOff=[1000])), ("iir10", dict(filt="iir", cutOff=[1000], filtLen=10)), ("fir6", dict(filt="fir", cutOff=[1000], filtLen=6)),
                             ("fir101", dict(filt="fir", cutOff=[1000], filtLen=101)), ("sg7", dict(filt="sg", cutOff=[1000], filtLen=7)),
                             ("sg101", dict(filt="sg", cutOff=[1000], filtLen=101))):
                keep("apply.%s.%s.%s" % (name, dt, where), lambda: M.apply_filter_ragged_batch(x, L, 16000.0, **kw))
            keep("pyin.%s.%s" % (dt, where), lambda: M.pyin_ragged_batch(x, L, 16000, return_states=True, **pyin))
            f0 = M.pyin_ragged_batch(x, L, 16000, **pyin)
            for method in ("linear", "pchip"):
                keep("interp.%s.%s.%s" % (method, dt, where), lambda: M.interp_nan_ragged_batch(f0[0], f0[3] if where == "dev" else f0[3].cpu().numpy(), method))
    lst = ragged_list(dev)
    keep("list.f0", lambda: M.get_f0_batch(lst, 16000, method="pyin", hopSize=0.002, minPitch=100, maxPitch=500, pyinframe_length=512,
                                   interpUnvoiced="linear", outFilter="iir", outFiltCutOff=[10]))
    for method in ("RMS", "Hilb"):
        keep("list.envelope." + method, lambda: M.calculate_amplitude_envelope_batch(lst, 16000, method=method, winLen=0.01, hopLen=0.002,
                                                                             outFilter="iir"))
    keep("list.change", lambda: M.get_MFCCS_change_batch(lst, 16000, outFiltCutOff=[12]))
    for kw in (dict(filt="sg", cutOff=[1000], filtLen=7), dict(filt="iir", cutOff=[1000])):
        keep("list.apply." + kw["filt"], lambda: M.applyFilter_batch(lst, 16000.0, **kw))
    for i in (0, 2, 3, 4):      # the single calls, which share their first steps with the list forms
        keep("single.f0.%d" % i, lambda: M.get_f0(lst[i], 16000, method="pyin", hopSize=0.002, minPitch=100, maxPitch=500,
                                                  pyinframe_length=512, interpUnvoiced="linear", outFilter="iir", outFiltCutOff=[10]))
        keep("single.envelope.%d" % i, lambda: M.calculate_amplitude_envelope(lst[i], 16000, method="Hilb", winLen=0.01, hopLen=0.002,
                                                                              outFilter="iir"))
        keep("single.change.%d" % i, lambda: M.get_MFCCS_change(lst[i], 16000, outFiltCutOff=[12]))
    torch.cuda.synchronize()
    return out


def welch_cases():
    """Case set `welch`: every instantiation and path of mm_modpsd.hip / mm_modcsd.hip (and what mm_welch.hip.inc holds for
    both) at the smallest shape that reaches it.  Float32 noise, device lengths throughout."""
    import torch
    import modulation_mfcc_amd as M
    dev = torch.device("cuda", 0)
    out = {}
    FS = 200.0

    def keep(name, result):
        for k, t in enumerate(result[1:]):                         # (result[0] is the host frequency grid)
            out["%s.%d" % (name, k)] = t.cpu().numpy()

    def noise(seed, rows, n):
        return torch.from_numpy(np.random.default_rng(seed).standard_normal((rows, n), dtype=np.float32)).to(dev)

    def lengths(*lens):
        return torch.tensor(lens, dtype=torch.int64, device=dev)

    def one_launch(nperseg):
        """no segment (a NaN row), one segment, five (half overlap): wave 0 takes a second segment, wave 1 .. 3 one each"""
        return 3 * nperseg, (nperseg - 1, nperseg, 3 * nperseg)

    # nperseg 8, noverlap 7: a segment per sample from the 8th on; 32 segments end the first chunk, 33 put one into the
    # second, 65 make three chunks -- the workspace and the finish kernels
    TWO = dict(nperseg=8, noverlap=7)
    TWO_N, TWO_LENS = 72, (39, 40, 72)

    def cross(name, x, y, ld, **kw):
        """all four outputs in one call, Pxy alone, Cxy alone"""
        keep(name + ".all", M.modulation_cross_spectra_ragged_batch(x, y, ld, FS, **kw))
        keep(name + ".csd", M.modulation_csd_ragged_batch(x, y, ld, FS, **kw))
        keep(name + ".coh", M.modulation_coherence_ragged_batch(x, y, ld, FS, **kw))

    for log2n in range(5, 13):
        nfft = 1 << log2n
        n, lens = one_launch(nfft)
        x, y = noise(log2n, 6, n), noise(100 + log2n, 3, n)
        keep("psd.n%d" % nfft, M.modulation_psd_ragged_batch(x[:3], lengths(*lens), FS, nperseg=nfft, nfft=nfft))
        if nfft <= 2048:
            cross("csd.n%d" % nfft, x[:3], y, lengths(*lens), nperseg=nfft, nfft=nfft)
            cross("csd.n%d.group3" % nfft, x, y[:2], lengths(*(lens + lens)), nperseg=nfft, nfft=nfft)
        if nfft in (32, 2048, 4096):
            x, y = noise(200 + log2n, 6, TWO_N), noise(300 + log2n, 3, TWO_N)
            if nfft != 2048:
                keep("psd2.n%d" % nfft, M.modulation_psd_ragged_batch(x[:3], lengths(*TWO_LENS), FS, nfft=nfft, **TWO))
            if nfft != 4096:
                cross("csd2.n%d" % nfft, x[:3], y, lengths(*TWO_LENS), nfft=nfft, **TWO)
                cross("csd2.n%d.group3" % nfft, x, y[:2], lengths(*(TWO_LENS + TWO_LENS)), nfft=nfft, **TWO)
    # nfft 64 over a segment of 50 samples (zeros behind it): the detrends and scalings, and a window given as an array
    n, lens = one_launch(50)
    x = noise(400, 3, n)
    for detrend in (False, "constant", "linear"):
        for scaling in ("density", "spectrum"):
            keep("psd.n64.%s.%s" % (detrend, scaling), M.modulation_psd_ragged_batch(
                x, lengths(*lens), FS, nperseg=50, nfft=64, detrend=detrend, scaling=scaling))
    keep("psd.n64.window", M.modulation_psd_ragged_batch(x, lengths(*lens), FS, window=np.hamming(50).astype(np.float32),
                                                         nperseg=50, nfft=64, detrend="linear"))
    # the cross kernel's factor 0 (a side of zeros), its half exponents (a side at 1e-6) and what lies behind a length
    y = torch.stack([torch.zeros(n, device=dev), 1e-6 * noise(401, 1, n)[0], noise(402, 1, n)[0]])
    y[2, 120:] = float("nan")
    x = x.clone()
    x[2, 120:] = float("nan")
    cross("csd.n64.sides", x, y, lengths(n, n, 120), nperseg=50, nfft=64, detrend="linear")
    torch.cuda.synchronize()
    return out


GAP_METHODS = ("linear", "pchip", "nearest", "nearest-up", "previous", "next", "zero", "slinear", "quadratic", "cubic", "akima")
GAP_SOME = ("linear", "pchip", "cubic")


def gap_rows(seed, rows, n):
    """A random walk per row with a third of its samples NaN, a gap before the first and behind the last valid sample."""
    rng = np.random.default_rng(seed)
    x = np.cumsum(rng.standard_normal((rows, n)), axis=1)
    if n > 8:
        x[rng.random((rows, n)) < 0.3] = np.nan
        x[:, 2:7] = rng.standard_normal((rows, 5))          # five valid samples whatever was drawn
        x[:, :2] = np.nan
        x[:, n - 3:] = np.nan
    else:
        x[:, 0] = np.nan
        x[:, n - 1] = np.nan
    return x


def gapfill_cases():
    """Case set `gapfill`: every interp_NAN kind through the five gap-filling calls, what they return and what they
    refuse with.  Only names the package exports, so that the same code runs on an older checkout."""
    import torch
    import modulation_mfcc_amd as M
    dev = torch.device("cuda", 0)
    out = {}

    def keep(name, call):
        """the call's result (a tensor, an array, or get_f0's pairs); a refusal is kept as its type and text"""
        try:
            r = call()
            parts = [a for pair in r for a in pair] if isinstance(r, list) else list(r) if isinstance(r, tuple) else [r]
            for k, a in enumerate(parts):
                out["%s.%d" % (name, k)] = a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
        except Exception as e:
            out[name + ".error"] = np.frombuffer(("%s: %s" % (type(e).__name__, e)).encode(), dtype=np.uint8)

    def every_call(name, x, counts, methods):
        """the five calls on one tensor; the ragged ones (two dimensions only) with host and with device counts"""
        for m in methods:
            keep("%s.NAN.%s" % (name, m), lambda: M.interp_NAN(x, m))
            keep("%s.batch.%s" % (name, m), lambda: M.interp_nan_batch(x, m))
            keep("%s.spline.%s" % (name, m), lambda: M.interp_nan_spline_batch(x, m))
            if counts is not None:
                for where, c in (("host", list(counts)), ("dev", torch.tensor(list(counts), dtype=torch.int64, device=dev))):
                    keep("%s.ragged.%s.%s" % (name, where, m), lambda: M.interp_nan_ragged_batch(x, c, m))
                    keep("%s.splragged.%s.%s" % (name, where, m), lambda: M.interp_nan_spline_ragged_batch(x, c, m))

    def put(a):
        return torch.from_numpy(np.ascontiguousarray(a)).to(dev)

    # shapes and types: 1030 crosses a segment border and makes the spline solve take two chunks
    for n in (5, 1024, 1025, 1030, 2100):
        x = gap_rows(n, 3, n)
        counts = (n, max(1, n // 2), max(1, n - 3))
        for dt in (np.float64, np.float32):
            name = "n%d.%s" % (n, np.dtype(dt).name)
            every_call(name + ".rows", put(x.astype(dt)), counts, GAP_METHODS)
            every_call(name + ".one", put(x[1].astype(dt)), None, GAP_METHODS)
    # layouts: a wider row pitch, a non-unit inner stride; an integer tensor; no row, no column
    x = gap_rows(77, 3, 1030)
    wide = put(np.concatenate([x, np.zeros((3, 7))], axis=1))[:, :1030]
    every_call("pitch", wide, (1030, 600, 1027), GAP_SOME)
    every_call("stride", put(np.repeat(x, 2, axis=1))[:, ::2], (1030, 600, 1027), GAP_SOME)
    every_call("stride.one", put(np.repeat(x[0], 2))[::2], None, GAP_SOME)
    every_call("int64", torch.arange(60, device=dev).reshape(3, 20), (20, 7, 1), GAP_SOME)
    every_call("int64.one", torch.arange(20, device=dev), None, GAP_SOME)
    every_call("norow", torch.zeros((0, 7), dtype=torch.float64, device=dev), (), GAP_SOME)
    every_call("nocolumn", torch.zeros((3, 0), dtype=torch.float64, device=dev), (1, 1, 1), GAP_SOME)
    # rows with exactly v valid samples (v = 12: no NaN), alone and between two good rows; then the same below a count of
    # 12 with valid samples behind it.  A clean row below a count of 2 has fewer samples than any kind with a NaN needs.
    spots = (2, 5, 7, 9, 10)
    good = gap_rows(5, 2, 20)
    for v in (0, 1, 2, 3, 4, 12):
        row = np.full(20, np.nan)
        if v == 12:
            row[:12] = np.arange(12) * 0.5 + 1.0
        else:
            row[list(spots[:v])] = 1.0 + np.arange(v) ** 2
        every_call("few%d.one" % v, put(row[:12]), None, GAP_METHODS)
        every_call("few%d.row" % v, put(row[None, :12]), (12,), GAP_METHODS)
        every_call("few%d.batch" % v, put(np.stack([good[0, :12], row[:12], good[1, :12]])), (12, 12, 12), GAP_METHODS)
        row[12:] = 3.0                                             # valid samples behind the count
        if v == 12:
            row[15] = np.nan
        every_call("few%d.below" % v, put(np.stack([good[0], row, good[1]])), (20, 12, 20), GAP_METHODS)
        every_call("few%d.below.row" % v, put(row[None, :]), (12,), GAP_METHODS)
    clean = np.stack([good[0], np.r_[1.0, 2.0, np.full(18, np.nan)], good[1]])
    every_call("clean2.below", put(clean), (20, 2, 20), GAP_METHODS)
    every_call("clean1.below", put(clean), (20, 1, 20), GAP_METHODS)
    # counts: host values out of range are refused, device values are clamped
    x = put(gap_rows(9, 3, 40))
    for m in GAP_SOME:
        for name, c in (("zero", [0, 40, 40]), ("beyond", [40, 41, 40]), ("short", [40, 40]), ("float", [40.0, 40.0, 40.0])):
            keep("counts.host.%s.%s" % (name, m), lambda: M.interp_nan_ragged_batch(x, c, m))
            keep("counts.host.%s.spl.%s" % (name, m), lambda: M.interp_nan_spline_ragged_batch(x, c, m))
        c = torch.tensor([0, 45, 30], dtype=torch.int64, device=dev)
        keep("counts.dev.%s" % m, lambda: M.interp_nan_ragged_batch(x, c, m))
        keep("counts.dev.spl.%s" % m, lambda: M.interp_nan_spline_ragged_batch(x, c, m))
        keep("counts.dev.int32.%s" % m, lambda: M.interp_nan_ragged_batch(x, c.int(), m))
    # host inputs: numpy curves into interp_NAN; host data into the device-only calls
    curve = gap_rows(11, 1, 50)[0]
    whole = np.cumsum(np.random.default_rng(12).standard_normal(50))
    for m in GAP_SOME:
        keep("numpy.gaps.%s" % m, lambda: M.interp_NAN(curve, m))
        keep("numpy.whole.%s" % m, lambda: M.interp_NAN(whole, m))
        keep("numpy.f32.%s" % m, lambda: M.interp_NAN(curve.astype(np.float32), m))
        for name, h in (("numpy", curve[None, :]), ("cpu", torch.from_numpy(curve[None, :]))):
            keep("host.%s.batch.%s" % (name, m), lambda: M.interp_nan_batch(h, m))
            keep("host.%s.ragged.%s" % (name, m), lambda: M.interp_nan_ragged_batch(h, [50], m))
            keep("host.%s.spline.%s" % (name, m), lambda: M.interp_nan_spline_batch(h, m))
            keep("host.%s.splragged.%s" % (name, m), lambda: M.interp_nan_spline_ragged_batch(h, [50], m))
    # end to end: two short clips with a silent stretch (unvoiced frames), one numpy, one on the device
    sig = [clips(80 + i, 1, n, 16000)[0].astype(np.float64) for i, n in enumerate((4000, 3100))]
    for s in sig:
        s[len(s) // 3:len(s) // 2] *= 1e-4
        s[:200] *= 1e-4
    lst = [sig[0], torch.from_numpy(sig[1].astype(np.float32)).to(dev)]
    kw = dict(method="pyin", hopSize=0.002, minPitch=100, maxPitch=500, pyinframe_length=512)
    for m in (None,) + GAP_SOME:
        filt = dict(outFilter=None) if m is None else dict(outFilter="iir", outFiltCutOff=[10])
        keep("f0.batch.%s" % m, lambda: M.get_f0_batch(lst, 16000, interpUnvoiced=m, **filt, **kw))
        keep("f0.batch.nofilter.%s" % m, lambda: M.get_f0_batch(lst, 16000, interpUnvoiced=m, outFilter=None, **kw))
        for i, s in enumerate(lst):
            keep("f0.one%d.%s" % (i, m), lambda: M.get_f0(s, 16000, interpUnvoiced=m, **filt, **kw))
            keep("f0.one%d.nofilter.%s" % (i, m), lambda: M.get_f0(s, 16000, interpUnvoiced=m, outFilter=None, **kw))
    torch.cuda.synchronize()
    print("%d results, %d of them refusals" % (len(out), sum(k.endswith(".error") for k in out)), flush=True)
    return out


def hilbert_cases():
    """Case set `hilbert`: the three call paths of csrc/mm_hilbert.hip.inc on the length lists of tests/hilbert_oracle.py (which
    tests/test_hilbert_host.py proves to reach every kernel instantiation), on the oracle's case rows, contiguous."""
    import torch
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import hilbert_oracle as H
    import modspec_oracle as MO
    from test_gpu_hilbert import BIG, _ragged_lengths
    from modulation_mfcc_amd import _lib, calc
    dev = torch.device("cuda", 0)
    out = {}
    DTYPES = ("float32", "float64")

    def put(a):
        return torch.from_numpy(np.ascontiguousarray(a)).to(dev)

    def envelope(name, x):
        out[name] = calc.hilbert_envelope_batch(put(x)).cpu().numpy()

    def row_counts(n, counts):
        return (5,) if n > BIG else counts

    # mm_hilbert_envelope: every direct and chirp plan, 1 row (unpaired), 2, 5 (the last clip without a partner) and 37
    for n in H.ENVELOPE_LENGTHS + H.BLUESTEIN_LENGTHS:
        for dt in DTYPES:
            rows = H.rows_for(n, dt)
            for R in row_counts(n, H.ENVELOPE_ROWS):
                envelope("env.n%d.%s.r%d" % (n, dt, R), H.take(rows, R)[0])
    for n in H.LONG_CASES:
        envelope("env.long.n%d" % n, H.take(H.rows_for(n, "float32"), 5)[0])
    # the XCD-ordered block lists with a block count that is no multiple of eight, and a plain plan beside them
    for n, R in ((256, 1000), (625, 1001), (35, 1000)):
        for dt in DTYPES:
            envelope("env.many.n%d.%s.r%d" % (n, dt, R), H.take(H.rows_for(n, dt), R)[0])
    # nine rows under a workspace bound that takes two pairs: library calls of 4, 4 and 1 rows
    for n in (625, 9600, 511):
        for code, dt in enumerate(DTYPES):
            per_pair = int(_lib.load().mm_hilbert_workspace_bytes(calc._hilbert_plan(n, code, dev).h, 2))
            old = calc.HILBERT_WS_BYTES
            try:
                calc.HILBERT_WS_BYTES = 2 * per_pair
                envelope("env.chunked.n%d.%s" % (n, dt), H.take(H.rows_for(n, dt), 9)[0])
            finally:
                calc.HILBERT_WS_BYTES = old
    # a row with a NaN and a row with an infinity beside four finite ones: a direct length and a chirp length
    for n in (9600, 511):
        for dt in DTYPES:
            for value in (np.nan, np.inf):
                x = H.take(H.rows_for(n, dt), 5)[0].copy()
                x[0, n // 3] = value
                envelope("env.%s.n%d.%s" % (value, n, dt), x)
    print("envelope: %d arrays" % len(out), flush=True)
    # mm_hilbert_rfft_f32: the forward passes alone, all samples valid and zeros behind the last three
    for n in H.FORWARD_LENGTHS:
        rows = H.rows_for(n, "float32")
        for R in row_counts(n, (1, 5, 37)):
            x = H.take(rows, R)[0]
            for T in sorted({n, max(1, n - 3)}):
                out["rfft.n%d.T%d.r%d" % (n, T, R)] = calc.rfft_rows_long(put(x[:, :T]), n).cpu().numpy()
    print("envelope + forward transform: %d arrays" % len(out), flush=True)
    # mm_hilbert_envelope_ragged with device lengths: test_ragged's clips, NaN behind every one of them
    for M_fft in H.RAGGED_M:
        n_max = M_fft // 2
        lengths = _ragged_lengths(n_max)
        for dt in DTYPES:
            x = np.full((len(lengths), n_max), np.nan, dtype=dt)
            for b, L in enumerate(lengths):
                x[b, :L] = H.rows_for(L, dt)[(H.ROW_LOUD + 3 * b) % MO.N_CASES]
            lens = torch.tensor(lengths, dtype=torch.int64, device=dev)
            out["ragged.M%d.%s" % (M_fft, dt)] = calc.hilbert_envelope_ragged_batch(put(x), lens).cpu().numpy()
    torch.cuda.synchronize()
    return out


CASESETS = {"s16": s16_cases, "tail": tail_cases, "ragged": ragged_cases, "welch": welch_cases, "gapfill": gapfill_cases,
            "hilbert": hilbert_cases}

if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "--compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    if len(sys.argv) != 3 or sys.argv[1] not in CASESETS:
        sys.exit("usage: lib_outputs.py {%s} OUT.npz | --compare A.npz B.npz" % ",".join(CASESETS))
    arrays = CASESETS[sys.argv[1]]()
    np.savez(sys.argv[2], **arrays)
    print(os.path.basename(os.environ.get("MODMFCC_LIB", "product")), sys.argv[1], "%d arrays, %.1f MB" %
          (len(arrays), sum(a.nbytes for a in arrays.values()) / 1e6), flush=True)
