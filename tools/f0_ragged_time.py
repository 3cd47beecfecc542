"""Ragged pYIN timing (GPU box): 1024 float32 clips at 16 kHz, 2 .. 10 s (sample counts drawn uniformly, seed 0), the
reference's get_f0 defaults (75 .. 600 Hz, frame_length 2048, 10 ms hop).  The signals are synthesised on the device
(harmonic glides with gaps and light noise, seed 0).  Timed with device events around the whole Python call -- workspace
allocation, table look-up, every launch -- which is what a user pays; the candidates alternate in one process, and the
results are compared before anything is timed.
    (a) pyin_ragged_batch: the padded batch with a length per clip
    (b) what was the only correct route before it: one pyin_batch per distinct length
    (c) pyin_batch of the zero-padded batch at n_max: wrong for every shorter clip, the cost ceiling of (a)
    python tools/f0_ragged_time.py [clips]"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np


def main():
    import torch
    from modulation_mfcc_amd import pyin_batch, pyin_ragged_batch, pyin_ragged_frames
    from modulation_mfcc_amd.plan import by_length
    dev = torch.device("cuda", 0)
    B = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
    sr, kw = 16000, dict(fmin=75, fmax=600, frame_length=2048, hop_length=160)
    rng = np.random.default_rng(0)
    lengths = rng.integers(2 * sr, 10 * sr + 1, B).astype(np.int64)
    lengths[0] = 10 * sr
    n_max = int(lengths.max())
    frames = pyin_ragged_frames(lengths, 2048, 160)
    T_max = int(frames.max())
    # harmonic glides f_b -> 2 f_b over ten seconds, gated 0.45 s of every 0.6 s, light noise; zeros behind every clip
    torch.manual_seed(0)
    audio = torch.empty((B, n_max), dtype=torch.float32, device=dev)
    t = torch.arange(n_max, device=dev, dtype=torch.float64) / sr
    gate = ((t % 0.6) < 0.45).double()
    for b in range(B):
        f = (90.0 + 2.0 * (b % 100)) * 2.0 ** (t / 10.0)
        ph = 2 * np.pi * torch.cumsum(f, 0) / sr
        y = sum((0.5 / k) * torch.sin(k * ph) for k in (1, 2, 3, 4)) * gate
        audio[b] = (y + 0.003 * torch.randn(n_max, device=dev, dtype=torch.float64)).float()
        audio[b, int(lengths[b]):] = 0.0
    groups = by_length(lengths)
    lens_dev = torch.from_numpy(lengths).to(dev)

    def ragged():
        return pyin_ragged_batch(audio, lens_dev, sr, **kw)

    def per_length():
        out = torch.zeros((B, T_max), dtype=torch.float64, device=dev)
        for n, idx in groups:
            T = 1 + n // 160
            if len(idx) == 1:
                out[int(idx[0]), :T] = pyin_batch(audio[int(idx[0]), :n], sr, **kw)[0]
            else:
                out[torch.from_numpy(idx).to(dev), :T] = pyin_batch(audio[torch.from_numpy(idx).to(dev), :n], sr, **kw)[0]
        return out

    def padded():
        return pyin_batch(audio, sr, **kw)

    # results first: (a) against (b) frame for frame; how many frames of real clips (c) gets wrong
    a, b_, c = ragged(), per_length(), padded()
    nn = lambda x: torch.nan_to_num(x, nan=-1.0)
    assert a[3].cpu().tolist() == frames.tolist()
    assert torch.equal(nn(a[0]), nn(b_)), "ragged and per-length results differ"
    live = torch.arange(T_max, device=dev)[None, :] < a[3][:, None]
    wrong = int(((nn(c[0]) != nn(b_)) & live).sum())
    clips_wrong = int((((nn(c[0]) != nn(b_)) & live).any(dim=1)).sum())
    voiced = int(a[1].sum())
    print(f"{B} clips, {lengths.min()} .. {n_max} samples ({len(groups)} distinct lengths), frames {frames.min()} .. {T_max}, "
          f"sum T_b / (B T_max) = {frames.sum() / (B * T_max):.3f}, {voiced} of {int(frames.sum())} frames voiced")
    print(f"    ragged == per-length on every frame; the zero-padded batch differs on {wrong} real frames of {clips_wrong} clips",
          flush=True)
    del a, b_, c

    def one_ms(fn):
        s, u = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        u.record()
        torch.cuda.synchronize()
        return s.elapsed_time(u)

    def stats(v):
        v = sorted(v)
        return f"{v[len(v) // 2]:.1f} ms (min {v[0]:.1f}, max {v[-1]:.1f}; {len(v)} calls)"

    fns = {"(a) ragged, a length per clip": ragged, "(c) zero-padded batch, one length": padded,
           "(b) one pyin_batch per distinct length": per_length}
    ragged(), padded()                                  # (warm: every shape above has run once already)
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for rep in range(3):                                # alternating: 4 calls each of (a) and (c), then one of (b)
        for _ in range(4):
            for k in list(fns)[:2]:
                ms[k].append(one_ms(fns[k]))
        ms["(b) one pyin_batch per distinct length"].append(one_ms(per_length))
    for k in fns:
        print(f"    {k}: {stats(ms[k])}", flush=True)


if __name__ == "__main__":
    main()
