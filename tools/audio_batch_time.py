"""Batched loader timing (GPU box): 1024 clips of 2 .. 10 s at 44.1 kHz, all lengths distinct, converted to 16 kHz.
    resample   resample_ragged_batch (device lengths and host lengths: one launch)  vs  the only correct route before it,
               one resample_batch per row, and -- for context: it computes and stores the padding and needs real zeros
               behind every clip -- resample_batch on all rows zero-filled to n_max (with and without the fill)
    files      load_audio_batch on generated 16-bit mono files (one read of every data chunk into a pinned buffer, one
               copy, one decode launch, one resample launch)  vs  the loop over load_audio; wall time including the file
               reads, and the device events around the same calls
    uniform    resample_batch on 256 x 441 000 samples (the README's single-length figure); with --lib, through another
               build of the library (ctypes only, so a build without the ragged entries can be timed in the same session)
Device events around each call after a warm-up; the ragged results are compared with the looped rows before anything is
timed.
    python tools/audio_batch_time.py [--root TREE] [--batch B] [--reps N] [--only resample|files|uniform] [--lib SO]"""
import argparse
import ctypes as C
import os
import shutil
import struct
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SR_IN, SR_OUT = 44100, 16000


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=ROOT)
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", choices=["resample", "files", "uniform"], default=None)
    ap.add_argument("--lib", default=None, help="uniform: another libmodmfcc.so to time mm_resample_banded_f32 of")
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))
    import torch
    import modulation_mfcc_amd
    from modulation_mfcc_amd import audio_io, load_audio, load_audio_batch, resample_batch, resample_ragged_batch
    print(f"package: {os.path.dirname(modulation_mfcc_amd.__file__)}", flush=True)
    dev = torch.device("cuda", 0)
    B = args.batch
    rng = np.random.default_rng(1)
    lens = rng.choice(np.arange(2 * SR_IN, 10 * SR_IN + 1), B, replace=False).astype(np.int64)
    n_max = int(lens.max())
    print(f"device: {torch.cuda.get_device_name(0)}; {B} clips, {lens.min()} .. {n_max} samples, {len(set(lens.tolist()))} distinct "
          f"lengths, {int(lens.sum())} valid samples of {B * n_max}", flush=True)

    def event_ms(fn, iters=1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / iters

    def wall_ms(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    def stats(ts):
        ts = sorted(ts)
        return f"{ts[len(ts) // 2]:.3f} ms (min {ts[0]:.3f}, max {ts[-1]:.3f}; {len(ts)} repeats)"

    def timed(fn, iters=1, warm=2, clock=event_ms):
        for _ in range(warm):
            fn()
        torch.cuda.synchronize()
        return stats([clock(fn, iters) if clock is event_ms else clock(fn) for _ in range(args.reps)])

    if args.only in (None, "uniform"):
        rows, n = 256, 441000
        x = torch.randn((rows, n), device=dev)
        if args.lib:
            lib = C.CDLL(os.path.abspath(args.lib))
            vp, i64, i32 = C.c_void_p, C.c_int64, C.c_int32
            lib.mm_resample_banded_f32.argtypes = [vp, i64, i64, i64, vp, vp] + [i32] * 6 + [vp, i64, vp]
            L, M = audio_io.resample_ratio(SR_IN, SR_OUT)
            tb = audio_io._device_banded(L, M, dev)
            y = torch.empty((rows, -(-n * L // M)), device=dev)
            st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

            def uniform():
                rc = lib.mm_resample_banded_f32(x.data_ptr(), rows, n, n, tb["d_atab"].data_ptr(), tb["d_lo_off"].data_ptr(), tb["F"],
                                                tb["S"], tb["NB"], tb["ksteps"], tb["lo_min"], tb["win"], y.data_ptr(), y.shape[1], st)
                assert rc == 0, rc
        else:
            def uniform():
                return resample_batch(x, SR_IN, SR_OUT)
        print(f"uniform: resample_batch {rows} x {n}, {args.lib or 'this build'}: {timed(uniform, iters=100, warm=10)}", flush=True)
        del x

    if args.only in (None, "resample"):
        x = torch.randn((B, n_max), device=dev)
        d_lens = torch.from_numpy(lens).to(dev)
        rows = [x[b, :int(lens[b])] for b in range(B)]
        xz = torch.empty_like(x)
        behind = torch.arange(n_max, device=dev)[None, :] >= d_lens[:, None]

        def loop():
            return [resample_batch(r, SR_IN, SR_OUT) for r in rows]

        def padded():
            xz.copy_(x)
            xz.masked_fill_(behind, 0.0)
            return resample_batch(xz, SR_IN, SR_OUT)
        y, ol = resample_ragged_batch(x, d_lens, SR_IN, SR_OUT)
        yh = resample_ragged_batch(x, lens, SR_IN, SR_OUT)[0]
        one = loop()
        assert torch.equal(y, yh) and ol.cpu().tolist() == [r.shape[0] for r in one]
        assert all(torch.equal(y[b, :one[b].shape[0]], one[b]) and not y[b, one[b].shape[0]:].any() for b in range(B))
        del y, yh, one
        print("resample: every ragged row equals resample_batch of the row alone bit for bit, zeros behind", flush=True)
        print(f"    resample_ragged_batch, device lengths: {timed(lambda: resample_ragged_batch(x, d_lens, SR_IN, SR_OUT), iters=5)}", flush=True)
        print(f"    resample_ragged_batch, host lengths:   {timed(lambda: resample_ragged_batch(x, lens, SR_IN, SR_OUT), iters=5)}", flush=True)
        print(f"    one resample_batch per row, events:    {timed(loop)}", flush=True)
        print(f"    one resample_batch per row, host wall: {timed(loop, clock=wall_ms)}", flush=True)
        print(f"    zero fill + resample_batch at n_max:   {timed(padded, iters=3)}", flush=True)
        print(f"    resample_batch at n_max alone:         {timed(lambda: resample_batch(xz, SR_IN, SR_OUT), iters=3)}", flush=True)
        del x, xz, rows, behind
        torch.cuda.empty_cache()

    if args.only in (None, "files"):
        d = tempfile.mkdtemp(prefix="audio_batch_time_")
        try:
            paths = []
            for i, n in enumerate(lens):
                data = rng.integers(-20000, 20000, int(n), dtype=np.int16).tobytes()
                body = b"WAVEfmt " + struct.pack("<IHHIIHH", 16, 1, 1, SR_IN, 2 * SR_IN, 2, 16) + b"data" + struct.pack("<I", len(data)) + data
                paths.append(os.path.join(d, f"{i:04d}.wav"))
                with open(paths[-1], "wb") as f:
                    f.write(b"RIFF" + struct.pack("<I", len(body)) + body)
            print(f"files: {B} 16-bit mono files, {sum(os.path.getsize(p) for p in paths) / 1e6:.0f} MB", flush=True)

            def batch():
                return load_audio_batch(paths, SR_OUT)

            def loop():
                return [load_audio(p, SR_OUT) for p in paths]
            xb, lb = batch()
            one = loop()
            assert all(torch.equal(xb[b, :int(lb[b])], one[b][0]) for b in range(B))
            del xb, one
            print("    every row of load_audio_batch equals load_audio of its file bit for bit", flush=True)
            print(f"    load_audio_batch, wall:          {timed(batch, clock=wall_ms)}", flush=True)
            print(f"    load_audio_batch, events:        {timed(batch)}", flush=True)
            print(f"    loop over load_audio, wall:      {timed(loop, warm=1, clock=wall_ms)}", flush=True)
            print(f"    loop over load_audio, events:    {timed(loop, warm=1)}", flush=True)
            # the device work of the batch route alone: the raw bytes are on the device already
            pl = audio_io.plan_wav_batch([audio_io.read_wav_header(p) for p in paths])
            raw = np.zeros(pl["total_bytes"], dtype=np.uint8)
            for p, o, nb in zip(paths, pl["offsets"], pl["nbytes"]):
                raw[o:o + nb] = np.fromfile(p, dtype=np.uint8, count=int(nb), offset=44)
            host = torch.from_numpy(raw).pin_memory()
            d_raw, d_tab = host.to(dev), torch.from_numpy(pl["table"].view(np.uint8)).to(dev)
            x, lengths = audio_io.decode_wav_batch(d_raw, d_tab, pl), pl["frames"]
            assert torch.equal(x, audio_io.load_wav_batch(paths, dev)[0])
            print(f"    host-to-device copy of the pinned buffer ({pl['total_bytes'] / 1e6:.0f} MB): {timed(lambda: host.to(dev, non_blocking=True))}", flush=True)
            print(f"    decode launch (mm_pcm_decode_ragged_f32):   {timed(lambda: audio_io.decode_wav_batch(d_raw, d_tab, pl), iters=5)}", flush=True)
            print(f"    resample_ragged_batch of the decoded batch: {timed(lambda: resample_ragged_batch(x, lengths, SR_IN, SR_OUT), iters=5)}",
                  flush=True)
            one = [np.fromfile(p, dtype=np.uint8, offset=44) for p in paths[:64]]
            d_one = [torch.from_numpy(r).to(dev) for r in one]
            lib = modulation_mfcc_amd._lib.load()
            outs = [torch.empty((1, r.shape[0] // 2), dtype=torch.float32, device=dev) for r in one]
            st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

            def dec64():
                for r, o in zip(d_one, outs):
                    lib.mm_pcm_decode_f32(r.data_ptr(), 2, 1, o.shape[1], o.data_ptr(), o.shape[1], st)
            print(f"    64 single-file decodes (mm_pcm_decode_f32), for scale: {timed(dec64)}", flush=True)
        finally:
            shutil.rmtree(d)


if __name__ == "__main__":
    main()
