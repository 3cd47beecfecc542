"""B-spline zoom timing (GPU box): zoom_batch / zoom_ragged_batch (mm_zoom2d_*) against
  (a) the route through the host: the images copied to the host, scipy.ndimage.zoom image by image, the result copied back;
  (b) a float4 device-to-device copy of the output's bytes (mm_devcopy_f32): the ceiling of a kernel bound by its stores,
on 129 x 2000 float64 at zoom 6, order 4 (the reference's example size), 257 x 30001 float32 at zoom 6, order 4 (a
five-minute recording: 1.1 GB out), 1024 x 40 x 1001 float32 at zoom (1, 0.5), order 3 (log-mel images brought to half the
frames) and the last ragged at 200 .. 1001 frames.  The prefilter alone (spline_filter_batch: the first two launches) and
the zoom without it (prefilter=False: the conversion and the evaluation) are timed beside the whole call to show which
launch holds the time.  Every call is timed whole with device events, warmed, repeated, the median printed with the
extremes; device and host calls alternate in one process; the results are compared before anything is timed.
    python tools/zoom_time.py [--no-host]"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import scipy.ndimage


def host_round_trip(X, zoom, order, widths=None, w_out=None):
    import torch
    imgs = X.cpu().numpy()
    if imgs.ndim == 2:
        out = scipy.ndimage.zoom(imgs, zoom, order=order)
    elif widths is None:
        out = np.stack([scipy.ndimage.zoom(a, zoom, order=order) for a in imgs])
    else:
        rows = [scipy.ndimage.zoom(a[:, :w], zoom, order=order) for a, w in zip(imgs, widths)]
        out = np.zeros((len(rows), rows[0].shape[0], w_out), dtype=imgs.dtype)
        for b, r in enumerate(rows):
            out[b, :, :r.shape[1]] = r
    return torch.from_numpy(np.ascontiguousarray(out)).to(X.device)


def main():
    import torch
    from modulation_mfcc_amd import _lib, spline_filter_batch, zoom_batch, zoom_ragged_batch
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
    cases = (("129 x 2000 float64, zoom 6, order 4", (129, 2000), np.float64, 6, 4, False, 3),
             ("257 x 30001 float32, zoom 6, order 4", (257, 30001), np.float32, 6, 4, False, 1),
             ("1024 x 40 x 1001 float32, zoom (1, 0.5), order 3", (1024, 40, 1001), np.float32, (1, 0.5), 3, False, 1),
             ("1024 x 40 x 1001 float32 ragged at 200 .. 1001, zoom (1, 0.5), order 3", (1024, 40, 1001), np.float32, (1, 0.5), 3,
              True, 1))
    for name, shape, dtype, zoom, order, is_ragged, host_reps in cases:
        x = (-40.0 + 15.0 * r.standard_normal(shape)).astype(dtype)
        d = torch.from_numpy(x).to(dev)
        widths = np.linspace(200, shape[-1], shape[0]).astype(np.int64) if is_ragged else None
        wd = None if widths is None else torch.from_numpy(widths).to(dev)
        if is_ragged:
            call = lambda: zoom_ragged_batch(d, wd, zoom, order=order)[0]
        else:
            call = lambda: zoom_batch(d, zoom, order=order)
        got = call()
        n_bytes = got.numel() * got.element_size()
        print(f"{name}: {tuple(got.shape)} out, {n_bytes / 1e6:.1f} MB", flush=True)
        w_out = got.shape[-1]
        host = (lambda: host_round_trip(d, zoom, order, widths, w_out)) if with_host else None
        if host is not None:
            want = host()
            err = float((got.double() - want.double()).abs().max() / want.double().abs().max())
            print(f"  largest difference device / host, relative to the maximum: {err:.1e}", flush=True)
            assert err <= (1e-6 if dtype == np.float32 else 1e-11), err
            del want
        parts = {"whole call": call,
                 "prefilter alone (launches 1 + 2)": lambda: spline_filter_batch(d, order),
                 "without prefilter (conversion + evaluation)":
                     (lambda: zoom_ragged_batch(d, wd, zoom, order=order, prefilter=False)) if is_ragged else
                     (lambda: zoom_batch(d, zoom, order=order, prefilter=False))}
        src = torch.empty((n_bytes + 15) // 16 * 4, dtype=torch.float32, device=dev).normal_()
        dst = torch.empty_like(src)
        stream = lambda: torch.cuda.current_stream().cuda_stream
        parts["float4 copy of the output's bytes (the ceiling)"] = lambda: _lib.check(
            lib.mm_devcopy_f32(src.data_ptr(), dst.data_ptr(), src.numel(), stream()), "mm_devcopy_f32")
        del got
        for fn in parts.values():                                   # warm-up: code objects, allocator
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        t = {k: [] for k in parts}
        for _ in range(4):                                          # alternating, 10 calls each a round
            for k, fn in parts.items():
                t[k] += [one_ms(fn) for _ in range(10)]
        for k in parts:
            print(f"    {k}: {stats(t[k])}", flush=True)
        med = {k: sorted(v)[len(v) // 2] for k, v in t.items()}
        ceil = med["float4 copy of the output's bytes (the ceiling)"]
        print(f"    whole call reaches {ceil / med['whole call']:.2f} of the copy; {n_bytes / med['whole call'] / 1e6:.0f} GB/s "
              f"of output", flush=True)
        if host is not None:
            th = [one_ms(host) for _ in range(host_reps)]
            print(f"    host round trip: {stats(th)}  ->  {sorted(th)[len(th) // 2] / med['whole call']:.0f} x the device call",
                  flush=True)
        del src, dst, d
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
