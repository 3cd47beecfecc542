"""Welch cross spectrum / coherence timing (GPU box): the routes to scipy.signal.csd / coherence of pairs of float32 curves
that are already on the device, in one process.
    (a)  modulation_cross_spectra_batch (mm_modcsd_f32, all four outputs) and modulation_coherence_batch (the coherence
         alone: three NULL outputs), row for row and with y shared by 13 rows (y_group = 13), and the ragged form
    (p)  two modulation_psd_batch calls on the same rows: what the two auto spectra alone cost at the parent commit
    (b)  the curves copied to the host and scipy.signal.csd + coherence there (the copies included)
    (c)  a torch composition on the device: unfold, detrend, window, torch.fft.rfft, products, mean over the segments
on 1024 clips x 13 trajectories x 1001 frames at fs 200, nperseg 256 (Hann, half overlap, constant detrend), and the same
batch ragged at 200 .. 1001 frames ((a) only).  Device events around each call (the host route: a host clock), warm-up
first, median over the repeats; (a) and (c) are compared with (b) before anything is timed.
    python tools/modcsd_time.py [--root TREE] [--clips B] [--reps N]"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=ROOT)
    ap.add_argument("--clips", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))
    import scipy.signal
    import torch
    import modulation_mfcc_amd
    from modulation_mfcc_amd import (modulation_coherence_batch, modulation_coherence_ragged_batch,
                                     modulation_cross_spectra_batch, modulation_cross_spectra_ragged_batch, modulation_psd_batch)
    print(f"package: {os.path.dirname(modulation_mfcc_amd.__file__)}", flush=True)
    dev = torch.device("cuda", 0)
    print(f"device: {torch.cuda.get_device_name(0)}", flush=True)

    def event_ms(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b)

    def wall_ms(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    def stats(ts):
        ts = sorted(ts)
        return f"{ts[len(ts) // 2]:.3f} ms (min {ts[0]:.3f}, max {ts[-1]:.3f}; {len(ts)} calls)"

    def timed(fn, clock=event_ms, reps=args.reps, warm=3):
        for _ in range(warm):
            fn()
        torch.cuda.synchronize()
        return stats([clock(fn) for _ in range(reps)])

    fs, nperseg, n, B = 200.0, 256, 1001, args.clips
    rows = B * 13

    def torch_csd(x, y):
        """Route (c): Hann, half overlap, constant detrend, 'density', nfft = nperseg; y [B, n] against x [B, 13, n]."""
        w = torch.hann_window(nperseg, periodic=True, device=x.device, dtype=torch.float32)

        def segs(t):
            s = t.unfold(-1, nperseg, nperseg // 2)
            return torch.fft.rfft((s - s.mean(dim=-1, keepdim=True)) * w, dim=-1)
        X, Y = segs(x), segs(y)
        if Y.dim() < X.dim():
            Y = Y.unsqueeze(1)
        sxx, syy, sxy = X.abs().square().mean(dim=-2), Y.abs().square().mean(dim=-2), (X.conj() * Y).mean(dim=-2)
        coh = sxy.abs().square() / (sxx * syy)
        k = 1.0 / (fs * float((w.double() ** 2).sum()))
        d = torch.full((nperseg // 2 + 1,), 2.0, device=x.device)
        d[0] = d[-1] = 1.0
        return sxx * (k * d), syy.expand_as(sxx) * (k * d), sxy * (k * d), coh

    def host_csd(x, y):
        """Route (b)."""
        xh, yh = x.cpu().numpy(), y.cpu().numpy()
        if yh.ndim < xh.ndim:
            yh = yh[:, None, :]
        return (scipy.signal.csd(xh, yh, fs=fs, nperseg=nperseg, axis=-1)[1],
                scipy.signal.coherence(xh, yh, fs=fs, nperseg=nperseg, axis=-1)[1])

    g = torch.Generator(device=dev).manual_seed(0)
    t = torch.arange(n, device=dev, dtype=torch.float32) / fs
    env = 0.05 + 0.02 * torch.sin(2 * np.pi * 4.0 * t) + 0.005 * torch.randn((B, n), device=dev, generator=g)       # [B, n]
    x = 20.0 + 30.0 * env[:, None, :] + 0.5 * torch.randn((B, 13, n), device=dev, generator=g)                     # [B, 13, n]
    ymat = env[:, None, :].expand(B, 13, n).contiguous()
    ref_csd, ref_coh = host_csd(x, env)
    for what, got in (("(a)", modulation_cross_spectra_batch(x, env, fs, nperseg=nperseg)), ("(c)", (None,) + torch_csd(x, env))):
        e1 = float(np.abs(got[3].cpu().numpy() - ref_csd).max() / np.abs(ref_csd).max())
        e2 = float(np.abs(got[4].cpu().numpy() - ref_coh).max())
        print(f"{what} differs from (b): Pxy by {e1:.1e} of the largest value, the coherence by {e2:.1e}", flush=True)
        assert e1 <= 1e-5 and e2 <= 1e-3, (e1, e2)          # ((b) is scipy on float32 input: its own means are float32)
    print(f"{rows} pairs x {n} samples, fs {fs}, nperseg {nperseg}, {(n - nperseg // 2) // (nperseg - nperseg // 2)} segments "
          f"per pair", flush=True)
    kw = dict(nperseg=nperseg)
    print(f"    (a) four outputs, y shared by 13 rows:      {timed(lambda: modulation_cross_spectra_batch(x, env, fs, **kw))}", flush=True)
    print(f"    (a) four outputs, row for row:              {timed(lambda: modulation_cross_spectra_batch(x, ymat, fs, **kw))}", flush=True)
    print(f"    (a) coherence alone, y shared by 13 rows:   {timed(lambda: modulation_coherence_batch(x, env, fs, **kw))}", flush=True)
    print(f"    (a) coherence alone, row for row:           {timed(lambda: modulation_coherence_batch(x, ymat, fs, **kw))}", flush=True)
    print(f"    (p) modulation_psd_batch of x:              {timed(lambda: modulation_psd_batch(x, fs, **kw))}", flush=True)
    print(f"    (p) modulation_psd_batch of x and of y:     "
          f"{timed(lambda: (modulation_psd_batch(x, fs, **kw), modulation_psd_batch(ymat, fs, **kw)))}", flush=True)
    print(f"    (c) torch unfold / rfft / products / mean:  {timed(lambda: torch_csd(x, env))}", flush=True)
    print(f"    (b) copy to the host + scipy csd, coherence: {timed(lambda: host_csd(x, env), wall_ms, 2, 1)}", flush=True)

    rng = np.random.default_rng(1)
    lens = rng.integers(200, 1002, size=rows).astype(np.int64)
    lens[0] = 1001
    lens_dev = torch.from_numpy(lens).to(dev)
    x2 = x.reshape(rows, n)
    out = modulation_cross_spectra_ragged_batch(x2, env, lens_dev, fs, **kw)[1:]
    for b in (0, 1, 2, rows - 1):
        if lens[b] >= nperseg:
            alone = modulation_cross_spectra_batch(x2[b, :int(lens[b])], env[b // 13, :int(lens[b])], fs, **kw)[1:]
            assert all(torch.equal(torch.view_as_real(o[b]) if o.is_complex() else o[b],
                                   torch.view_as_real(a) if a.is_complex() else a) for o, a in zip(out, alone)), b
    print(f"ragged at {lens.min()} .. {lens.max()} frames ({int((lens < nperseg).sum())} pairs below nperseg: NaN), sampled "
          f"pairs equal the pairs alone bit for bit", flush=True)
    print(f"    (a) four outputs, ragged, device lengths:   "
          f"{timed(lambda: modulation_cross_spectra_ragged_batch(x2, env, lens_dev, fs, **kw))}", flush=True)
    print(f"    (a) coherence alone, ragged:                "
          f"{timed(lambda: modulation_coherence_ragged_batch(x2, env, lens_dev, fs, **kw))}", flush=True)


if __name__ == "__main__":
    main()
