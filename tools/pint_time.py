"""Praat intensity contour timing (GPU box): praat_intensity_batch (mm_pint_f32) against
  (a) a float64 torch composition on the device: the frames gathered by the same table, mean, centre, square, weight, sum,
      divide -- in chunks of about 1 GiB of frames;
  (b) the route through the host: the sound copied to the host, the numpy restatement, the contour copied back;
  (c) a float4 device-to-device copy of the input's plus the output's bytes (mm_devcopy_f32): the floor of any kernel that
      reads the sound and writes the contour once,
on one five-minute 44.1 kHz recording at the defaults, the same recording in the dense 'RMSpraat' form (120 Hz, a frame per
sample: 13.2 M frames of 2353 taps) and 1024 clips of 10 s at 16 kHz at the defaults.  Every call is timed whole with device
events, warmed, repeated, the median printed with the extremes; the routes alternate in one process; the results are
compared before anything is timed.  The dense form's composition and host route are timed on a slice of the frames and
scaled (said in the output): whole, they take seconds and minutes.  For the dense form the achieved float64 operation
rate is printed against the vector peak (4 operations per tap and frame; 256 CUs x 4 SIMDs x 16 lanes x 2.4 GHz).
    python tools/pint_time.py [--no-host]"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

PEAK_F64_OPS = 256 * 4 * 16 * 2.4e9          # vector float64 instructions x lanes per second (an FMA counted once)


def host_restatement(x, p, k0, k1):
    """numpy float64 on frames k0 .. k1 of every row of x [rows, n], in blocks."""
    out = np.empty((x.shape[0], k1 - k0), dtype=np.float64)
    ar = np.arange(-p.hw, p.hw + 1)
    sw = p.window.sum()
    for b in range(x.shape[0]):
        xb = x[b].astype(np.float64)
        for a in range(k0, k1, 4096):
            c = p.centres[a:min(a + 4096, k1)].astype(np.int64)
            v = xb[np.clip(c[:, None] + ar[None, :], 0, xb.size - 1)]
            d = v - v.mean(axis=1, keepdims=True)
            out[b, a - k0:a - k0 + len(c)] = (d * d * p.window).sum(axis=1) / sw
    return out


def main():
    import torch
    from modulation_mfcc_amd import _lib, praat_intensity_batch, praat_intensity_params
    dev = torch.device("cuda", 0)
    lib = _lib.load()
    with_host = "--no-host" not in sys.argv

    def one_ms(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b)

    def stats(t):
        t = sorted(t)
        return f"{t[len(t) // 2]:.3f} ms (min {t[0]:.3f}, max {t[-1]:.3f}; {len(t)} calls)"

    r = np.random.default_rng(7)
    # name, rows, n, sr, keywords, frames of the composition (None: all), rows x frames of the host route
    cases = (("5 min at 44.1 kHz, defaults", 1, 300 * 44100, 44100, {}, None, (1, None)),
             ("5 min at 44.1 kHz, dense (120 Hz, a frame per sample)", 1, 300 * 44100, 44100,
              dict(minimum_pitch=120.0, time_step=1 / 44100), 1 << 19, (1, 1 << 15)),
             ("1024 clips x 10 s at 16 kHz, defaults", 1024, 160000, 16000, {}, None, (32, None)))
    FLOOR = "float4 copy of the input's and output's bytes (the floor)"
    KERNEL = "kernel (praat_intensity_batch)"
    for name, rows, n, sr, kw, comp_frames, (host_rows, host_frames) in cases:
        p = praat_intensity_params(n, sr, **kw)
        x = (0.1 * r.standard_normal((rows, n))).astype(np.float32)
        d = torch.from_numpy(x).to(dev)
        call = lambda: praat_intensity_batch(d, sr, db=False, **kw)[1]
        got = call()
        in_bytes, out_bytes = d.numel() * 4, got.numel() * 8
        print(f"{name}: hw {p.hw}, {p.W} taps, hops {p.hops}, {p.T} frames per clip; {in_bytes / 1e6:.1f} MB in, "
              f"{out_bytes / 1e6:.1f} MB out", flush=True)
        d_w = torch.from_numpy(np.array(p.window)).to(dev)
        sw = d_w.sum()
        ar = torch.arange(-p.hw, p.hw + 1, device=dev)
        Tc = p.T if comp_frames is None else min(p.T, comp_frames)
        d_c = torch.from_numpy(p.centres[:Tc].astype(np.int64)).to(dev)
        per = max(1, (1 << 27) // p.W)                       # frames of a chunk: about 1 GiB of float64

        def composition():
            out = torch.empty((rows, Tc), dtype=torch.float64, device=dev)
            for b in range(rows):
                xb = d[b].double()
                for k0 in range(0, Tc, per):
                    k1 = min(k0 + per, Tc)
                    v = xb[(d_c[k0:k1, None] + ar[None, :]).clamp_(0, n - 1)]
                    dd = v - v.mean(dim=1, keepdim=True)
                    out[b, k0:k1] = (dd * dd * d_w).sum(dim=1) / sw
            return out
        want = composition()
        # (the two references do not clip a window at the sound's ends -- the framing reaches that only where its rounding
        # falls on a tie, in the first or last frame --: such frames are timed, not compared)
        whole = torch.from_numpy((p.centres >= p.hw) & (p.centres.astype(np.int64) + p.hw < n)).to(dev)
        print(f"  {int((~whole).sum())} of {p.T} frames have a clipped window", flush=True)
        err = float(((got[:, :Tc] - want).abs() / want)[:, whole[:Tc]].max())
        print(f"  largest per-frame difference kernel / torch composition ({Tc} of {p.T} frames): {err:.1e}", flush=True)
        assert err <= 1e-10, err
        del want
        host = None
        if with_host:
            hr, hf = min(rows, host_rows), p.T if host_frames is None else min(p.T, host_frames)
            host = lambda: torch.from_numpy(host_restatement(d[:hr].cpu().numpy(), p, 0, hf)).to(dev)
            errh = float(((got[:hr, :hf] - host()).abs() / got[:hr, :hf])[:, whole[:hf]].max())
            print(f"  largest per-frame difference kernel / host restatement: {errh:.1e}", flush=True)
            assert errh <= 1e-10, errh
        del got
        src = torch.empty((in_bytes + out_bytes + 15) // 16 * 4, dtype=torch.float32, device=dev).normal_()
        dst = torch.empty_like(src)
        stream = lambda: torch.cuda.current_stream().cuda_stream
        parts = {KERNEL: call, "torch composition": composition,
                 FLOOR: lambda: _lib.check(
                     lib.mm_devcopy_f32(src.data_ptr(), dst.data_ptr(), src.numel(), stream()), "mm_devcopy_f32")}
        for fn in parts.values():                                   # warm-up: code objects, allocator
            for _ in range(2):
                fn()
        torch.cuda.synchronize()
        t = {k: [] for k in parts}
        for _ in range(3):                                          # alternating, 3 calls each a round
            for k, fn in parts.items():
                t[k] += [one_ms(fn) for _ in range(3)]
        for k in parts:
            note = f" [{Tc} of {p.T} frames: x {p.T / Tc:.1f} for all]" if k == "torch composition" and Tc != p.T else ""
            print(f"    {k}: {stats(t[k])}{note}", flush=True)
        med = {k: sorted(v)[len(v) // 2] for k, v in t.items()}
        k_ms = med[KERNEL]
        print(f"    the copy is {med[FLOOR] / k_ms:.3f} of the kernel's time; the torch composition, scaled to all frames, takes "
              f"{med['torch composition'] * p.T / Tc / k_ms:.2f} x the kernel; {rows * n / sr / (k_ms / 1e3):.0f} s of sound per second",
              flush=True)
        ops = 4.0 * rows * p.T * p.W / (k_ms / 1e3)
        print(f"    {ops / 1e12:.2f} T float64 operations per second (4 per tap and frame): {100 * ops / PEAK_F64_OPS:.1f} % of the "
              f"vector peak of {PEAK_F64_OPS / 1e12:.1f} T", flush=True)
        if host is not None:
            th = [one_ms(host) for _ in range(1)]
            scale = rows / hr * p.T / hf
            print(f"    host round trip of {hr} of {rows} clips, {hf} of {p.T} frames: {stats(th)}  ->  scaled to the whole "
                  f"{sorted(th)[len(th) // 2] * scale / k_ms:.0f} x the kernel", flush=True)
        del src, dst, d
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
