"""pYIN timing (GPU box): pyin_batch on 1024 clips x 10 s x 16 kHz at the reference defaults (hopSize 0.01, 75-600 Hz:
1 025 024 frames), one 5-minute 44.1 kHz recording at hopSize 0.005 (the UI's single call: ~60 k sequential Viterbi
frames), and the oracle's CMND + banded Viterbi per clip on 16 host processes as the CPU baseline.
    python tools/f0_time.py [--skip-cpu]"""
import os, sys, time
from concurrent.futures import ProcessPoolExecutor
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np


def _cpu_clip(seed):
    import pyin_oracle as O
    y = O.synth("glide", 16000, 10.0, np.float32, seed=seed)
    t0 = time.perf_counter()
    st = O.pyin_stages(y, fmin=75, fmax=600, sr=16000, hop_length=160)
    O.viterbi_banded(st["obs"], st["A"], st["p_init"], st["sizes"]["n_bins"])
    return time.perf_counter() - t0


def main():
    import torch
    from modulation_mfcc_amd import pyin_batch
    dev = torch.device("cuda", 0)

    def timed(fn, k):
        fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(k):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / k * 1e3

    g = torch.Generator(device=dev).manual_seed(0)
    B, n = 1024, 160000
    t = torch.arange(n, device=dev, dtype=torch.float64) / 16000.0
    f = 110 + 80 * torch.rand((B, 1), generator=g, device=dev, dtype=torch.float64)
    audio = (0.4 * torch.sin(2 * np.pi * f * t[None]) + 0.02 * torch.randn((B, n), generator=g, device=dev,
                                                                           dtype=torch.float64)).float()
    kw = dict(fmin=75, fmax=600, hop_length=160)
    ms = timed(lambda: pyin_batch(audio, 16000, **kw), 3)
    print(f"pyin_batch 1024 x 10 s x 16 kHz (1 025 024 frames, float32): {ms:.1f} ms  "
          f"({1024 * 1001 / ms * 1e3 / 1e6:.2f} M frames/s)", flush=True)
    n2 = 300 * 44100
    t2 = torch.arange(n2, device=dev, dtype=torch.float64) / 44100.0
    rec = (0.4 * torch.sin(2 * np.pi * (150 + 40 * torch.sin(2 * np.pi * 0.3 * t2)) * t2)).float()
    hop2 = int(0.005 * 44100)
    ms2 = timed(lambda: pyin_batch(rec, 44100, fmin=75, fmax=600, hop_length=hop2), 2)
    frames2 = 1 + n2 // hop2
    print(f"pyin_batch one 5 min 44.1 kHz recording, hop {hop2} ({frames2} frames): {ms2:.1f} ms", flush=True)
    if "--skip-cpu" not in sys.argv:
        with ProcessPoolExecutor(16) as ex:
            t0 = time.perf_counter()
            per = list(ex.map(_cpu_clip, range(32)))
            wall = time.perf_counter() - t0
        print(f"CPU oracle (CMND + banded Viterbi), 16 processes: {np.median(per):.2f} s per 10 s clip, "
              f"{32 / wall:.2f} clips/s -> 1024 clips ~{1024 / (32 / wall):.0f} s", flush=True)


if __name__ == "__main__":
    main()
