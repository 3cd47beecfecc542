"""dev (GPU box): every output array of a fixed list of small cases on the library named by MODMFCC_LIB, saved to one .npz --
one process per library; two files are then compared bit for bit (a schedule move of a kernel must not change a bit).

    MODMFCC_LIB=$PWD/modulation_mfcc_amd/libmodmfcc_parent.so python tools/lib_outputs.py s16 parent.npz
    python tools/lib_outputs.py s16 branch.npz
    python tools/lib_outputs.py --compare parent.npz branch.npz

Case set `s16`: the smallest shapes that reach each code path of the staged n_fft-512 kernel (logmel512s_kernel) and the
matrix-pipe kernel.  n_fft 512, 16 kHz, win 400, 40 mel / 13 MFCC unless said otherwise."""
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


CASESETS = {"s16": s16_cases}

if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "--compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    if len(sys.argv) != 3 or sys.argv[1] not in CASESETS:
        sys.exit("usage: lib_outputs.py {%s} OUT.npz | --compare A.npz B.npz" % ",".join(CASESETS))
    arrays = CASESETS[sys.argv[1]]()
    np.savez(sys.argv[2], **arrays)
    print(os.path.basename(os.environ.get("MODMFCC_LIB", "product")), sys.argv[1], "%d arrays, %.1f MB" %
          (len(arrays), sum(a.nbytes for a in arrays.values()) / 1e6), flush=True)
