"""Praat-style spectrogram timing (GPU box): praat_spectrogram_batch (mm_pspec_f32) against
  (a) a torch composition on the device: gather the frames by the same table, window, torch.fft.rfft(n=nfft), square,
      band sum, scale;
  (b) the route through the host: the sound copied to the host, the numpy restatement (scipy.fft.rfft), the image copied back;
  (c) a float4 device-to-device copy of the input's plus the output's bytes (mm_devcopy_f32): the floor of any kernel that
      reads the sound and writes the image once,
on one five-minute 44.1 kHz recording at the defaults, the same at window 0.03 / frequency step 100, and 1024 clips of 10 s
at 16 kHz.  Every call is timed whole with device events, warmed, repeated, the median printed with the extremes; the
routes alternate in one process; the results are compared before anything is timed.  The tables of a geometry are uploaded
by the first call (the warm-up), as for every later call of a user.
    python tools/pspec_time.py [--no-host]"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import scipy.fft


def host_restatement(x, p):
    """numpy float32, frame by frame in blocks (the frames of a long recording do not fit at once)."""
    out = np.empty((x.shape[0], p.n_freqs, p.n_frames), dtype=x.dtype)
    w = p.window.astype(x.dtype)
    nb = p.n_freqs * p.bw
    for b in range(x.shape[0]):
        for k0 in range(0, p.n_frames, 4096):
            s = p.starts[k0:k0 + 4096].astype(np.int64)
            X = scipy.fft.rfft(x[b][s[:, None] + np.arange(p.nw)[None, :]] * w, n=p.nfft, axis=-1)[:, :nb]
            P = (X.real * X.real + X.imag * X.imag).reshape(len(s), p.n_freqs, p.bw).sum(axis=2)
            out[b, :, k0:k0 + len(s)] = (x.dtype.type(p.scale) * P).T
    return out


def main():
    import torch
    from modulation_mfcc_amd import _lib, praat_spectrogram_batch, praat_spectrogram_params
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
    cases = (("5 min at 44.1 kHz, defaults", 1, 300 * 44100, 44100, {}, 1),
             ("5 min at 44.1 kHz, window 0.03 / step 100", 1, 300 * 44100, 44100, dict(window_length=0.03, frequency_step=100.0), 1),
             ("1024 clips x 10 s at 16 kHz, defaults", 1024, 160000, 16000, {}, 1))
    HOST_ROWS = 64          # the host route is timed on this many clips of a batch and scaled to the batch
    FLOOR = "float4 copy of the input's and output's bytes (the floor)"
    for name, rows, n, sr, kw, host_reps in cases:
        p = praat_spectrogram_params(n, sr, **kw)
        x = (0.1 * r.standard_normal((rows, n))).astype(np.float32)
        d = torch.from_numpy(x).to(dev)
        call = lambda: praat_spectrogram_batch(d, sr, **kw)[2]
        got = call()
        in_bytes, out_bytes = d.numel() * 4, got.numel() * 4
        print(f"{name}: nw {p.nw}, nfft {p.nfft}, bw {p.bw}, {p.n_freqs} x {p.n_frames} per clip; {in_bytes / 1e6:.1f} MB in, "
              f"{out_bytes / 1e6:.1f} MB out", flush=True)
        d_w = torch.from_numpy(p.window.astype(np.float32)).to(dev)
        d_s = torch.from_numpy(p.starts.astype(np.int64)).to(dev)
        ar = torch.arange(p.nw, device=dev)
        chunk = max(1, (1 << 28) // (p.n_frames * p.nfft * 4))              # rows of a gather: about 1 GiB of frames at a time

        def composition():
            out = torch.empty((rows, p.n_freqs, p.n_frames), dtype=torch.float32, device=dev)
            for r0 in range(0, rows, chunk):
                fr = d[r0:r0 + chunk][:, d_s[:, None] + ar[None, :]] * d_w
                X = torch.fft.rfft(fr, n=p.nfft, dim=-1)[..., :p.n_freqs * p.bw]
                P = (X.real * X.real + X.imag * X.imag).reshape(fr.shape[0], p.n_frames, p.n_freqs, p.bw).sum(dim=3)
                out[r0:r0 + chunk] = (P * p.scale).transpose(1, 2)
            return out
        want = composition()
        err = float((got.double() - want.double()).abs().max() / want.double().abs().max())
        print(f"  largest difference kernel / torch composition, relative to the maximum: {err:.1e}", flush=True)
        assert err <= 4e-6, err
        del want
        host = None
        if with_host and host_reps:
            hr = min(rows, HOST_ROWS)
            host = lambda: torch.from_numpy(host_restatement(d[:hr].cpu().numpy(), p)).to(dev)
            errh = float((got[:hr].double() - host().double()).abs().max() / got[:hr].double().abs().max())
            print(f"  largest difference kernel / host restatement: {errh:.1e}", flush=True)
            assert errh <= 4e-6, errh
        del got
        src = torch.empty((in_bytes + out_bytes + 15) // 16 * 4, dtype=torch.float32, device=dev).normal_()
        dst = torch.empty_like(src)
        stream = lambda: torch.cuda.current_stream().cuda_stream
        parts = {"kernel (praat_spectrogram_batch)": call, "torch composition": composition,
                 FLOOR: lambda: _lib.check(
                     lib.mm_devcopy_f32(src.data_ptr(), dst.data_ptr(), src.numel(), stream()), "mm_devcopy_f32")}
        for fn in parts.values():                                   # warm-up: code objects, allocator, rocFFT plans
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        t = {k: [] for k in parts}
        for _ in range(4):                                          # alternating, 5 calls each a round
            for k, fn in parts.items():
                t[k] += [one_ms(fn) for _ in range(5)]
        for k in parts:
            print(f"    {k}: {stats(t[k])}", flush=True)
        med = {k: sorted(v)[len(v) // 2] for k, v in t.items()}
        k_ms = med["kernel (praat_spectrogram_batch)"]
        print(f"    the copy is {med[FLOOR] / k_ms:.2f} "
              f"of the kernel's time; the torch composition takes {med['torch composition'] / k_ms:.2f} x the kernel; "
              f"{rows * n / sr / (k_ms / 1e3):.0f} s of sound per second", flush=True)
        if host is not None:
            th = [one_ms(host) for _ in range(host_reps)]
            print(f"    host round trip of {hr} of {rows} clips: {stats(th)}  ->  scaled to the batch "
                  f"{sorted(th)[len(th) // 2] * rows / hr / k_ms:.0f} x the kernel", flush=True)
        del src, dst, d
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
