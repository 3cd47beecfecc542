"""Ragged-batch timing (GPU box): MfccPlan.mfcc_ragged on 1024 clips, n_max = 160 000, the headline configuration
(16 kHz, n_fft 512, win 400, hop 160, 40 mel, 13 MFCC), against the calls a user had before it:
    (a) full     every length = n_max            vs  plan.mfcc(audio) with set_fuse_dct(False): the same log-mel kernel
                                                     followed by the separate clamp + DCT launch, the nearest existing path
    (b) ragged   lengths uniform in [0.3, 1] n_max  vs  a loop of plan.mfcc over the distinct lengths (one call per length,
                                                     each on the rows of that length cut to it)
Device events around the whole call, warm-up first, the two sides alternating in one process, median over the repeats; the
results are compared before anything is timed ((a): mfcc_close-style bound against plan.mfcc; (b): the looped rows).
    python tools/ragged_time.py [--root TREE] [--batch B] [--reps N] [--loop-reps N] [--only-ragged K]
--root TREE imports the package from another checkout.  --only-ragged K runs K ragged calls of case (a) and nothing else
(for a kernel trace of the path's launches)."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KW = dict(sr=16000, n_fft=512, win_length=400, hop_length=160, n_mels=40, n_mfcc=13, fmin=100.0, fmax=8000.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=ROOT)
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--n-max", type=int, default=160000)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--loop-reps", type=int, default=3, help="repeats of the per-length loop of case (b) (about 1000 calls each)")
    ap.add_argument("--only-ragged", type=int, default=0)
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))
    import torch
    import modulation_mfcc_amd
    from modulation_mfcc_amd import MfccConfig, MfccPlan
    print(f"package: {os.path.dirname(modulation_mfcc_amd.__file__)}", flush=True)
    print(f"device: {torch.cuda.get_device_name(0)}; {args.batch} clips, n_max {args.n_max}, {KW}", flush=True)
    dev = torch.device("cuda", 0)
    B, n = args.batch, args.n_max

    g = torch.Generator(device=dev).manual_seed(0)
    t = torch.arange(n, device=dev, dtype=torch.float32) / KW["sr"]
    audio = 0.3 * torch.sin(2 * np.pi * 220 * t) * (1 + 0.5 * torch.sin(2 * np.pi * 4 * t)) \
        + 0.05 * torch.randn((B, n), device=dev, generator=g)
    plan = MfccPlan(MfccConfig(**KW))          # the ragged calls
    ref = MfccPlan(MfccConfig(**KW))           # the existing calls, DCT in its own launch
    ref.set_fuse_dct(False)
    T = plan.cfg.num_frames(n)
    out = torch.empty((B, KW["n_mfcc"], T), dtype=torch.float32, device=dev)
    out_ref = torch.empty_like(out)
    full = torch.full((B,), n, dtype=torch.int64, device=dev)

    if args.only_ragged:
        for _ in range(args.only_ragged):
            plan.mfcc_ragged(audio, full, out=out)
        torch.cuda.synchronize()
        return

    def one_ms(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b)

    def stats(ts):
        ts = sorted(ts)
        return f"{ts[len(ts) // 2]:.3f} ms (min {ts[0]:.3f}, max {ts[-1]:.3f}; {len(ts)} calls)"

    def close(a, b):
        scale = float(b.abs().amax())
        return float((a - b).abs().amax()) / scale

    # ---- (a) every length = n_max ----
    f_rag = lambda: plan.mfcc_ragged(audio, full, out=out)                      # noqa: E731
    f_ref = lambda: ref.mfcc(audio, out=out_ref)                                # noqa: E731
    f_rag(), f_ref()
    torch.cuda.synchronize()
    err = close(out, out_ref)
    assert err <= 1e-4, err
    for _ in range(3):
        f_rag(), f_ref()
    torch.cuda.synchronize()
    ta, tr = [], []
    for _ in range(args.reps):                                                  # alternating
        ta.append(one_ms(f_rag))
        tr.append(one_ms(f_ref))
    ma, mr = sorted(ta)[len(ta) // 2], sorted(tr)[len(tr) // 2]
    print(f"(a) all lengths = n_max; max difference {err:.1e} of the largest coefficient", flush=True)
    print(f"    mfcc_ragged:                   {stats(ta)}", flush=True)
    print(f"    mfcc, set_fuse_dct(False):     {stats(tr)}", flush=True)
    print(f"    ratio {ma / mr:.3f}", flush=True)
    ws_r = int(plan._lib.mm_ragged_workspace_bytes(plan._h, B, n))
    ws_m = int(plan._lib.mm_workspace_bytes(plan._h, B, n))
    print(f"    workspace: ragged {ws_r / 2 ** 20:.1f} MiB, mfcc {ws_m / 2 ** 20:.1f} MiB", flush=True)

    # ---- (b) lengths uniform in [0.3, 1] n_max ----
    rng = np.random.default_rng(1)
    lens = rng.integers(int(0.3 * n), n + 1, B)
    lens_dev = torch.from_numpy(lens).to(dev)
    groups = {}
    for b, L in enumerate(lens.tolist()):
        groups.setdefault(L, []).append(b)
    groups = [(L, torch.tensor(idx, device=dev)) for L, idx in sorted(groups.items())]

    def loop():
        res = []
        for L, idx in groups:
            rows = audio[idx[0]:idx[0] + 1, :L] if idx.numel() == 1 else audio[idx][:, :L]
            res.append(ref.mfcc(rows))
        return res

    f_rag_b = lambda: plan.mfcc_ragged(audio, lens_dev, out=out)                # noqa: E731
    f_rag_b()
    res = loop()
    torch.cuda.synchronize()
    worst = 0.0
    for (L, idx), m in zip(groups[::max(1, len(groups) // 32)], res[::max(1, len(groups) // 32)]):
        Tb = m.shape[2]
        worst = max(worst, close(out[idx][:, :, :Tb], m))
        assert float(out[idx][:, :, Tb:].abs().amax()) == 0.0 if Tb < T else True
    assert worst <= 1e-4, worst
    for _ in range(3):
        f_rag_b()
    torch.cuda.synchronize()
    tb, tl = [], []
    for _ in range(args.loop_reps):
        tb += [one_ms(f_rag_b) for _ in range(max(1, args.reps // args.loop_reps))]
        tl.append(one_ms(loop))
    mb, ml = sorted(tb)[len(tb) // 2], sorted(tl)[len(tl) // 2]
    print(f"(b) lengths uniform in [0.3, 1] n_max: {len(groups)} distinct lengths, {int(lens.sum())} valid samples of "
          f"{B * n}; max difference on the sampled rows {worst:.1e}", flush=True)
    print(f"    mfcc_ragged:                   {stats(tb)}", flush=True)
    print(f"    loop of mfcc over the lengths: {stats(tl)}", flush=True)
    print(f"    ratio {mb / ml:.4f}", flush=True)


if __name__ == "__main__":
    main()
