"""Ragged amplitude-envelope timing (GPU box): 1024 float32 clips of 2 .. 10 s at 16 kHz, all lengths distinct (the pYIN
ragged workload), the longest exactly 160 000 samples.
    'Hilb'  hilbert_envelope_ragged_batch with host lengths (one call per power-of-two class) and with device lengths (one
            class, that of n_max)  vs  the only correct route before it: one hilbert_envelope_batch per distinct length, once
            with a cold plan cache and once more (1024 lengths through an LRU of HILBERT_MAX_PLANS: every call still builds
            its tables), and the single-length call on all rows at the longest length (160 000, transformed directly) and at
            159 999 (through chirps, the ragged call's transform length)
    'RMS'   rms_ragged_batch at the reference's defaults (winLen 0.1 s, hopLen 0.01 s)  vs  one rms_batch per distinct length,
            and rms_batch on all rows at the longest length
Device events around each call (the loops: a host clock around the loop and a synchronise), warm-up first, median over the
repeats; the ragged results are compared with the looped rows before anything is timed.
    python tools/envelope_ragged_time.py [--root TREE] [--batch B] [--reps N] [--loop-reps N]"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SR = 16000


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=ROOT)
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--loop-reps", type=int, default=2, help="repeats of the per-length loops after the cold one")
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))
    import torch
    import modulation_mfcc_amd
    from modulation_mfcc_amd import calc
    from modulation_mfcc_amd.batch import rms_batch, rms_ragged_batch, rms_ragged_frames
    print(f"package: {os.path.dirname(modulation_mfcc_amd.__file__)}", flush=True)
    dev = torch.device("cuda", 0)
    B, n_max = args.batch, 10 * SR
    rng = np.random.default_rng(1)
    lens = rng.choice(np.arange(2 * SR, n_max), B - 1, replace=False).astype(np.int64)
    lens = np.concatenate([lens, [n_max]])
    rng.shuffle(lens)
    lens_dev = torch.from_numpy(lens).to(dev)
    print(f"device: {torch.cuda.get_device_name(0)}; {B} clips, {lens.min()} .. {lens.max()} samples, {len(set(lens.tolist()))} "
          f"distinct lengths, {int(lens.sum())} valid samples of {B * n_max}", flush=True)
    g = torch.Generator(device=dev).manual_seed(0)
    t = torch.arange(n_max, device=dev, dtype=torch.float32) / SR
    x = 0.3 * torch.sin(2 * np.pi * 220 * t) * (1 + 0.5 * torch.sin(2 * np.pi * 4 * t)) \
        + 0.05 * torch.randn((B, n_max), device=dev, generator=g)

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
        return f"{ts[len(ts) // 2]:.2f} ms (min {ts[0]:.2f}, max {ts[-1]:.2f}; {len(ts)} calls)"

    def timed(fn, reps=args.reps, warm=2):
        for _ in range(warm):
            fn()
        torch.cuda.synchronize()
        return stats([event_ms(fn) for _ in range(reps)])

    order = np.argsort(lens)

    # ---- 'Hilb' ----
    classes = [(M, len(idx)) for M, idx in calc._hilbert_ragged_classes(lens)]
    print(f"'Hilb': classes (transform length, clips) {classes}; device lengths: one class, {calc.hilbert_ragged_fft_size(n_max)}",
          flush=True)
    res = {}

    def hilb_loop():
        for b in order:
            res[int(b)] = calc.hilbert_envelope_batch(x[b:b + 1, :int(lens[b])])
    cold = wall_ms(hilb_loop)
    env_h = calc.hilbert_envelope_ragged_batch(x, lens)
    env_d = calc.hilbert_envelope_ragged_batch(x, lens_dev)
    worst = 0.0
    for b in order[::max(1, B // 32)]:
        n, ref = int(lens[b]), res[int(b)][0]
        for env in (env_h, env_d):
            worst = max(worst, float((env[b, :n] - ref).abs().amax()) / float(ref.amax()))
            assert float(env[b, n:].abs().amax()) == 0.0 if n < n_max else True
    assert worst <= 4e-5, worst                              # both sides within 2e-5 of scipy
    print(f"    largest difference between the ragged and the looped rows (sampled): {worst:.1e} of the row's maximum", flush=True)
    del env_h, env_d
    res.clear()
    loops = [wall_ms(hilb_loop) for _ in range(args.loop_reps)]
    res.clear()
    print(f"    loop of hilbert_envelope_batch over the lengths, cold plan cache: {cold:.1f} ms", flush=True)
    print(f"    the same loop again (LRU of {calc.HILBERT_MAX_PLANS} lengths):                  {stats(loops)}", flush=True)
    print(f"    hilbert_envelope_ragged_batch, host lengths:   {timed(lambda: calc.hilbert_envelope_ragged_batch(x, lens))}", flush=True)
    print(f"    hilbert_envelope_ragged_batch, device lengths: {timed(lambda: calc.hilbert_envelope_ragged_batch(x, lens_dev))}",
          flush=True)
    print(f"    hilbert_envelope_batch, all rows at {n_max}:  {timed(lambda: calc.hilbert_envelope_batch(x))}", flush=True)
    print(f"    hilbert_envelope_batch, all rows at {n_max - 1}:  {timed(lambda: calc.hilbert_envelope_batch(x[:, :n_max - 1]))}",
          flush=True)

    # ---- 'RMS' at the reference's defaults ----
    frame, hop = int(0.1 * SR), int(0.01 * SR)
    T = rms_ragged_frames(lens, frame, hop)

    def rms_loop():
        for b in order:
            res[int(b)] = rms_batch(x[b:b + 1, :int(lens[b])], frame, hop)
    cold = wall_ms(rms_loop)
    env = rms_ragged_batch(x, lens_dev, frame, hop)
    for b in order[::max(1, B // 32)]:
        assert torch.equal(env[b, :T[b]], res[int(b)][0]) and float(env[b, T[b]:].abs().sum()) == 0.0, b
    res.clear()
    loops = [wall_ms(rms_loop) for _ in range(max(args.loop_reps, 3))]
    res.clear()
    print(f"'RMS' frame {frame}, hop {hop}: the sampled rows equal the looped ones bit for bit", flush=True)
    print(f"    loop of rms_batch over the lengths, first pass: {cold:.1f} ms; again: {stats(loops)}", flush=True)
    print(f"    rms_ragged_batch, device lengths: {timed(lambda: rms_ragged_batch(x, lens_dev, frame, hop))}", flush=True)
    print(f"    rms_ragged_batch, host lengths:   {timed(lambda: rms_ragged_batch(x, lens, frame, hop))}", flush=True)
    print(f"    rms_batch, all rows at {n_max}:    {timed(lambda: rms_batch(x, frame, hop))}", flush=True)


if __name__ == "__main__":
    main()
