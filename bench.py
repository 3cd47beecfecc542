#!/usr/bin/env python3
"""bench.py -- MFCC + modulation-spectrum frames/s on MI355X (BASELINE.json metric).

    python bench.py [--gpus N] [--steps K] [--warmup W] [--dump-outputs DIR] [--full]

One "step" = one pass of the hot path (MFCC, then the trajectory rFFT) over one batch of synthetic
clips that is already resident in HBM.  Per-GPU workload = BASELINE.json configs[2]: 1024 clips x
10 s x 16 kHz, win 400 / hop 160 / n_fft 512 / 40 mel / 13 MFCC + modulation spectrum; with N GPUs
every rank processes its own 1024 clips (weak scaling; N = 8 is configs[4], 8192 clips) and ONE RCCL
gather moves every rank's output slab to rank 0 inside the timed region.

A plain run does only what the headline needs: set up the batch (rows 0, R/2 and R-1 carry three
oracle clips unless --no-check, so that the inputs are those of a --full run), run the step untimed
for --settle-ms (the GPU's clocks leave their idle state), run W warm-up steps, time K steps, write
the last timed step's outputs when --dump-outputs DIR is given, and print one JSON line (rank 0)
with `value` = whole-job frames/s and `ms_per_step` = wall milliseconds of one timed step.

--dump-outputs DIR writes DIR/mfcc.npy (float32 [rows, n_mfcc, T]) and, for the workloads with the
modulation spectrum, DIR/modspec.npy (float32 [rows, n_mfcc, n_mod/2+1, 2]: real, imaginary) of the
last timed step on rank 0: every row of the batch when that fits DUMP_BYTES_MAX, otherwise a fixed
sample of rows drawn with DUMP_ROW_SEED (the result line names them under `dump`).

--full adds everything else, as sections of the same run (--no-cpu / --no-check / --no-extra drop
single ones of them):
  roofline     -- the dominant kernel of the timed region (fused frame+window+rFFT+power+mel+log),
                  algorithmic bytes / average launch duration from HIP events on the launch stream;
  rfft_stage   -- the stage-isolated batched rFFT kernel (the "% HBM roofline (rFFT)" figure),
                  measured in the same process right after the timed region, beside a float4
                  grid-stride device copy (mm_devcopy_f32) as the practical HBM ceiling;
  c2, c4       -- BASELINE configs[1] (MFCC only) and configs[3] (48 kHz stereo, n_fft 2048, 80 mel,
                  40 MFCC, batch 512) timed in the same process after the headline region (N = 1);
  value_literal, value_mfcc_only, gather_variants -- N > 1: both gather variants timed with the same steps: the literal
                  north star (every rank computes MFCC + modulation spectrum in its one fused launch, both arrays
                  travel in the one gather; the default, `value`) and MFCC-only on the wire (root transforms the
                  gathered trajectories), each with the root's and the other ranks' compute / gather times;
  cpu_baseline -- the NumPy oracle (a port of the reference's librosa path) on the host cores,
                  bounded sample, rank 0 at N = 1 only.  It runs FIRST, before anything touches the
                  GPU (its worker pool is forked from a process that has not initialised HIP);
  check, parity_ok -- the three oracle rows of every section's last timed step against the oracle
                  (a failed check makes the run exit 3 after the line);
  refdefault_call, next_rows -- see time_reference_call() and time_next_rows().
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0          # MI355X HBM3E spec (MI355X_MICROARCH.md); ~6300 GB/s achievable

C16K = dict(sr=16000, n_fft=512, win_length=400, hop_length=160, n_mels=40, n_mfcc=13, fmin=100.0, fmax=8000.0)
C48K = dict(sr=48000, n_fft=2048, win_length=1200, hop_length=480, n_mels=80, n_mfcc=40, fmin=100.0, fmax=10000.0)
# the reference's OWN default call (script/main.py:732-748 -> script/mfcc.py:382-387): sr 10 kHz, tStep 5 ms -> hop 50,
# winLen 25 ms -> win 250, n_fft 512, librosa's default 128 mel, maxFreq 10000 (above Nyquist: 26 empty filters)
REFD = dict(sr=10000, n_fft=512, win_length=250, hop_length=50, n_mels=128, n_mfcc=13, fmin=100.0, fmax=10000.0)
WORKLOADS = {
    # name: (BASELINE configs index, rows per GPU, channels, seconds, cfg kwargs, with_modspec)
    "c3": (2, 1024, 1, 10.0, C16K, True),
    "c2": (1, 1024, 1, 10.0, C16K, False),
    "c4": (3, 512, 2, 10.0, C48K, False),
    "refdefault": (None, 1024, 1, 10.0, REFD, False),
}
UI_CALL = dict(channelN=0, tStep=0.005, winLen=0.025, n_mfcc=13, n_fft=512, minFreq=100, maxFreq=10000, removeFirst=1,
               filtCutoff=12, filtOrd=6, diffMethod="grad", outFilter="iir", outFiltType="low", outFiltCutOff=[12],
               outFiltLen=6, outFiltPolyOrd=3)          # script/main.py:732-769, argument for argument


def workload_label(name, B, T, cfg, n_mod):
    idx, _, ch, secs, _, with_mod = WORKLOADS[name]
    what = f"{B} clips" if ch == 1 else f"{B} stereo clips (both channels transformed = {B * ch} channel-rows [B, 2, n], row stride n)"
    head = f"BASELINE configs[{idx}] per GPU" if idx is not None else "the reference's own default call (script/main.py:732-748) as a batch"
    return (f"{head}: {what} x {secs:g} s x {cfg.sr:g} Hz, win {cfg.win_length} "
            f"hop {cfg.hop_length} n_fft {cfg.n_fft}, {cfg.n_mels} mel (fmax {cfg.fmax:g}), {cfg.n_mfcc} MFCC"
            + (f" + modulation spectrum (rFFT {n_mod} over trajectories)" if with_mod else ""))


def csrc_sha16():
    """Content hash of the kernel sources (csrc/* and the C header), 16 hex digits: what ties a committed counter
    summary to the code it was taken on (tools/summarize_prof.py writes the same value into profiles/*_pmc.csv)."""
    import hashlib
    h = hashlib.sha256()
    d = os.path.join(ROOT, "modulation_mfcc_amd", "csrc")
    files = sorted(os.path.join(d, f) for f in os.listdir(d) if f.endswith((".hip", ".inc", ".h", ".cpp")) or f == "Makefile")
    files.append(os.path.join(ROOT, "include", "modmfcc.h"))
    for f in files:
        h.update(os.path.basename(f).encode() + b"\0")
        h.update(open(f, "rb").read())
    return h.hexdigest()[:16]


def s16_kernel_key(cfg, mode):
    """Name prefix of the staged-sample kernel instantiation a configuration runs on: logmel512s_kernel<MODE, NR, ...> with NR
    the staging groups of its hop (1 / 2 / 3 / 4 for hop <= 56 / 121 / 186 / 252; pre-emphasis: at least 3) --
    configs[1] (NR 3) and the reference default (NR 1) are different kernels with different traffic."""
    hop = cfg.hop_length
    nr = 1 if hop <= 56 else 2 if hop <= 121 else 3 if hop <= 186 else 4
    if getattr(cfg, "preemph", 0.0):
        nr = max(nr, 3)
    return f"logmel512s_kernel<{mode}, {nr},"


def pmc_traffic(kernel_key):
    """HBM bytes per launch of a kernel from the newest committed rocprofv3 PMC summary that lists it
    (profiles/*_pmc.csv, written by tools/summarize_prof.py from separate FETCH_SIZE / WRITE_SIZE passes of
    this same command; FETCH_SIZE x2 as MI355X_MICROARCH.md prescribes) -- but ONLY a summary taken on the kernel
    sources of this run (its csrc_sha16 column equals csrc_sha16()): otherwise None, with the reason."""
    import csv
    import glob
    want = csrc_sha16()
    stale = None
    for f in sorted(glob.glob(os.path.join(ROOT, "profiles", "*_pmc.csv")), reverse=True):
        for r in csv.DictReader(open(f)):
            if kernel_key in r["Kernel"]:
                if r.get("csrc_sha16") == want:
                    return int(r["hbm_bytes_per_launch"]), os.path.relpath(f, ROOT)
                stale = stale or os.path.relpath(f, ROOT)
    return None, (f"no counter summary for csrc {want} (newest listing this kernel: {stale}, other sources)" if stale else None)


def synth_batch(torch, device, batch, n, sr, seed0):
    """0.3 sin(2 pi 220 t)(1 + 0.5 sin(2 pi 4 t)) + 0.05 N(0,1), generated on device."""
    import math
    g = torch.Generator(device=device).manual_seed(seed0)
    t = torch.arange(n, device=device, dtype=torch.float64) / sr
    base = (0.3 * torch.sin(2 * math.pi * 220 * t) * (1 + 0.5 * torch.sin(2 * math.pi * 4 * t))).float()
    x = torch.randn((batch, n), generator=g, device=device, dtype=torch.float32)
    x.mul_(0.05).add_(base[None, :])
    return x


# ---- CPU baseline (oracle) ------------------------------------------------------------------
def _cpu_init():
    # one thread per worker process: the BLAS / OpenMP pools must be limited BEFORE numpy is first imported
    # in the worker (the parent has not imported it when it forks)
    for v in ("OMP_NUM_THREADS", "OPENBLAS_NUM_THREADS", "MKL_NUM_THREADS", "NUMEXPR_NUM_THREADS"):
        os.environ[v] = "1"
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import mfcc_oracle  # noqa: F401  (numpy / scipy load here, once per worker)
    try:
        from threadpoolctl import threadpool_limits
        threadpool_limits(1)
    except Exception:
        pass


_CLIPS = {}


def _cpu_one(args):
    seed, n, kw, with_mod = args
    import mfcc_oracle as O
    key = (seed % 4, n, kw["sr"])                       # four clips per worker, generated once (not in the timed work)
    if key not in _CLIPS:
        _CLIPS[key] = O.synth_clip(seed % 4, n, kw["sr"], "am")   # the GPU batch's signal model
    clip = _CLIPS[key]
    t0 = time.perf_counter()
    m = O.mfcc(clip, O.OracleConfig(**kw))
    if with_mod:
        O.modspec(m)
    return m.shape[1], time.perf_counter() - t0


def cpu_baseline(kw, n, with_mod, budget_s=12.0):
    """Runs before the first GPU call: fork()ing workers from a HIP-initialised parent is not safe."""
    import multiprocessing as mp
    try:
        cores = len(os.sched_getaffinity(0))
    except AttributeError:
        cores = os.cpu_count() or 1
    cores = max(1, min(cores, 16))   # a 1-GPU box's CPU share is 16 cores (the node shows 256)
    ctx = mp.get_context("fork")
    with ctx.Pool(cores, initializer=_cpu_init) as pool:
        pool.map(_cpu_one, [(i, n, kw, with_mod) for i in range(4 * cores)], chunksize=4)   # warm-up: clips generated, pages in
        t0 = time.perf_counter()
        pool.map(_cpu_one, [(100 + i, n, kw, with_mod) for i in range(cores)])
        dt1 = time.perf_counter() - t0
        rounds = max(1, min(2000, int(budget_s / max(dt1, 1e-3))))
        n_clips = cores * rounds
        t0 = time.perf_counter()
        res = pool.map(_cpu_one, [(1000 + i, n, kw, with_mod) for i in range(n_clips)], chunksize=1)
        dt = time.perf_counter() - t0
    frames = sum(r[0] for r in res)
    busy = sum(r[1] for r in res)
    return {"value": frames / dt, "unit": "frames/s", "cores": cores, "kind": "port",
            "sample": f"{n_clips} clips x {frames // n_clips} frames (the GPU run's signal model, four clips per worker generated "
                      f"beforehand), NumPy oracle of the librosa path, {cores} worker processes x "
                      f"1 thread, {dt:.1f} s wall, {busy:.0f} core-seconds in the path"}


def _check_one(args):
    seed, n, kw, with_mod = args
    import mfcc_oracle as O
    clip = O.synth_clip(seed, n, kw["sr"], "am")
    m = O.mfcc(clip, O.OracleConfig(**kw))
    return clip, m, (O.modspec(m) if with_mod else None)


CHECK_SEEDS = (90001, 90002, 90003)


def oracle_check_vectors(jobs, seeds=CHECK_SEEDS):
    """jobs: {name: (cfg kwargs, n_samples, with_modspec)} -> {name: [(clip, oracle MFCC, oracle spectrum or None) x 3]}.
    Three clips of the run's signal model per workload with their oracle answers, computed in forked workers BEFORE
    this process touches HIP -- the oracle as the checker of the timed output, never on its path.  The bench writes the
    clips into rows 0, R/2 and R-1 of each device batch and compares those output rows after the timed region."""
    import multiprocessing as mp
    ctx = mp.get_context("fork")
    names = list(jobs)
    args = [(sd, jobs[nm][1], jobs[nm][0], jobs[nm][2]) for nm in names for sd in seeds]
    with ctx.Pool(min(len(args), 12), initializer=_cpu_init) as pool:
        res = pool.map(_check_one, args, chunksize=1)
    return {nm: res[i * len(seeds):(i + 1) * len(seeds)] for i, nm in enumerate(names)}


def compare_rows(np, out_mfcc, out_mod, rows, vec):
    """Oracle spot-check of the rows that carry the oracle's clips: worst |got - want| / max|want| (north-star bound 1e-4)."""
    worst, worst_ms = 0.0, 0.0
    for r_, (_, want, want_ms) in zip(rows, vec):
        got = out_mfcc[r_].cpu().numpy()
        worst = max(worst, float(np.abs(got - want).max() / np.abs(want).max()))
        if want_ms is not None and out_mod is not None:
            gm = out_mod[r_].cpu().numpy()
            worst_ms = max(worst_ms, float(np.abs(gm - want_ms).max() / np.abs(want_ms).max()))
    has_ms = out_mod is not None and vec[0][2] is not None
    return {"rows": list(rows), "max_rel": worst, "max_rel_modspec": (worst_ms if has_ms else None),
            "tolerance": 1e-4, "ok": bool(worst <= 1e-4 and worst_ms <= 1e-4),
            "against": "NumPy oracle (oracle/mfcc_oracle.py) on the same three clips, computed before HIP init; "
                       "output rows of the last timed step"}


EVENT_EVERY = 4      # dominant-kernel HIP events on every 4th timed step


def settle(torch, fn, seconds, chunk=8):
    """Untimed calls of fn, `chunk` at a time with a synchronize after each chunk (the host must not queue far more GPU work
    than the wall-clock budget), until `seconds` have passed.  Returns the number of calls."""
    calls = 0
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < seconds:
        for _ in range(chunk):
            fn()
        torch.cuda.synchronize()
        calls += chunk
    return calls


def time_steps(torch, plan, fn, steps, warmup, stages, sync=None, events=True):
    """warmup untimed + `steps` timed calls of fn; HIP events around `stages` only inside the timed region --
    and only on every EVENT_EVERY-th step there (an event pair costs the stream two barrier packets, ~6 us each:
    rocprofv3 shows them as gaps on both sides of the kernel) -- the other stages from a short pass afterwards.
    events=False: no events and no pass afterwards (a plain run: the timed steps alone).
    Returns (seconds, {stage: (ms_sum, launches)})."""
    for _ in range(warmup):
        fn()
    if sync:
        sync()
    torch.cuda.synchronize()
    if not events:
        t0 = time.perf_counter()
        for _ in range(steps):
            fn()
        if sync:
            sync()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, {}
    every = max(1, min(EVENT_EVERY, steps // 5))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(steps):
        if i % every == 0:
            plan.timing_enable(True, stages=stages)
        elif i % every == 1 or every == 1:
            plan.timing_enable(False)
        fn()
    if sync:
        sync()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    plan.timing_enable(False)
    stage = plan.timing_read()
    plan.timing_enable(True)
    for _ in range(min(steps, 5)):
        fn()
    if sync:
        sync()
    torch.cuda.synchronize()
    plan.timing_enable(False)
    for k, v in plan.timing_read().items():
        if k not in stages:
            stage[k] = v
    return dt, stage


FP32_VEC_TF = 157.3           # MI355X_MICROARCH.md: peak FP32 vector = peak f32-input MFMA
FP64_VEC_TF = 78.6            # FP64 vector (half the FP32 vector rate)


def time_next_rows(torch, dev):
    """The rows around the hot path at BASELINE-like sizes: device time per call (wall clock over
    5 calls after 2 warm-up calls) WITH what bounds each -- algorithmic bytes (what the row must read + write) against
    the 8 TB/s HBM peak, or algorithmic flops against the matching arithmetic peak -- so that every entry carries a
    fraction of a roofline, not a bare time."""
    import ctypes as C
    from modulation_mfcc_amd import MfccConfig, MfccPlan, tail, calc, audio_io, _lib
    from modulation_mfcc_amd.batch import rms_batch

    def t(fn, k=5):
        for _ in range(2):
            fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(k):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / k * 1e3

    def hbm(ms, nbytes, what):
        gbs = nbytes / (ms * 1e-3) / 1e9
        return {"ms": round(ms, 4), "bound": "hbm", "algorithmic_bytes": int(nbytes), "achieved": round(gbs, 1),
                "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": round(gbs / HBM_PEAK_GBS, 4), "bytes_are": what}

    def flops(ms, nflop, peak, which, what):
        tf = nflop / (ms * 1e-3) / 1e12
        return {"ms": round(ms, 4), "bound": which, "algorithmic_flops": int(nflop), "achieved": round(tf, 2),
                "peak": peak, "unit": "TFLOP/s", "frac": round(tf / peak, 4), "flops_are": what}

    out = {}
    plan = MfccPlan(MfccConfig(**WORKLOADS["c3"][4]))
    B, K, T = 1024, 13, 1001
    m = torch.randn((B, K, T), device=dev)
    sos1 = tail.design_lowpass(6, 12, 0.01)
    ms = t(lambda: plan.mfcc_change(m, sos1, sos1))
    out["N1_change_tail_1024x13x1001"] = hbm(ms, B * K * T * 4 + B * T * 8, "MFCC rows in (f32) + change curve out (f64); the "
                                             "float64 recursion is latency-bound, DESIGN.md section 7")
    # the recursion itself: 3 sections x (4 fma + 1 mul) = 27 flops per sample and direction, 12 rows + 1 curve per clip
    n_ext = T + 2 * 21
    out["N1_change_tail_1024x13x1001"]["fp64"] = flops(ms, 27.0 * 2 * (K - 1 + 1) * n_ext * B, FP64_VEC_TF, "fp64-vector",
                                                       "sequential sosfiltfilt recursion only (what scipy executes), "
                                                       "not the time-parallel form's extra passes")
    # the reference's own call shape: ONE recording (five minutes, tStep 1 ms -> 300 001 frames), the segmented-rows form
    m1 = torch.randn((1, K, 300001), device=dev)
    ms = t(lambda: plan.mfcc_change(m1, sos1, sos1))
    out["N1_change_tail_one_recording_1x13x300001"] = hbm(ms, K * 300001 * 4 + 300001 * 8, "MFCC rows in (f32) + change curve out (f64)")
    del m1
    # row A8 beyond 8192 frames per clip (mm_hilbert_rfft_f32): the trajectories of ONE recording at the reference's
    # default 1 ms step -- ten seconds (10 001 frames -> 16 384 points) and five minutes (300 001 -> 524 288)
    for T_, nm_ in ((10001, 16384), (300001, 524288)):
        tr_ = torch.randn((K, T_), device=dev)
        o_ = torch.empty((K, nm_ // 2 + 1), dtype=torch.complex64, device=dev)
        ms = t(lambda: calc.rfft_rows_long(tr_, nm_, out=o_))
        out[f"A8_long_trajectories_13x{T_}"] = hbm(ms, K * (4 * T_ + 8 * (nm_ // 2 + 1)), "trajectories in + half spectra out "
                                                   f"(n_mod {nm_}: a complex transform of the zero-padded real rows in global memory)")
        del tr_, o_
    x = torch.randn((256, 160000), device=dev)
    ms = t(lambda: rms_batch(x, 400, 160, True))
    out["N3_rms_256x160000"] = hbm(ms, 256 * 160000 * 4 + 256 * 1001 * 4, "samples in + envelope out")
    ms = t(lambda: calc.hilbert_envelope_batch(x))
    out["N3_hilbert_256x160000"] = hbm(ms, 256 * 160000 * 8, "samples in + envelope out (the implementation: two clips per "
                                       "complex transform; forward radix-256 pass | forward radix-625 pass + mask + inverse "
                                       "radix-625 pass in ONE launch | inverse radix-256 pass + envelope: three round trips "
                                       "of 128 complex rows minus the ends, the clips read three times (maxima, pairing, envelope), the envelope "
                                       "written: 8 x 164 MB = 1.31 GB)")
    out["N3_hilbert_256x160000"]["implementation_bytes"] = 128 * 160000 * 8 * 4 + 256 * 160000 * 4 * 4
    from modulation_mfcc_amd import applyFilter
    env = calc.hilbert_envelope_batch(x)                 # float32, as the reference filters it (odd extension in float32)
    ms = t(lambda: applyFilter(env, 16000.0, filt="iir", cutOff=[12.0], filtLen=6))
    out["N3_envelope_iir_filter_256x160000"] = hbm(ms, 256 * 160000 * 12, "float32 envelope in + float64 filtered envelope out "
                                                   "(sosfiltfilt order 6; a workgroup per row: one read + one write per sample "
                                                   "and direction through a float64 workspace)")
    out["N3_envelope_iir_filter_256x160000"]["implementation_bytes"] = 256 * 160000 * (4 + 8 + 8 + 8)
    del env
    # a typed n_fft (the reference's dialog passes what the user types: script/config_dialog.py:141,610): BASELINE
    # configs[1]'s batch with 400- and 800-sample frames on the two-stage register kernel (mm_reg2.hip)
    x16 = 0.1 * torch.randn((1024, 160000), device=dev)
    for nf_ in (400, 800):
        pl_ = MfccPlan(MfccConfig(**dict(C16K, n_fft=nf_)))
        o_ = torch.empty((1024, 13, 1001), device=dev)
        ms = t(lambda: pl_.mfcc(x16, out=o_))
        out[f"typed_n_fft_{nf_}_1024x160000"] = hbm(ms, 1024 * 1001 * (4 * 160 + 4 * 13), "unique audio in + MFCC out (SURVEY 8(d)); "
                                                    "compute-bound like the n_fft 512 kernel (c2 in this record)")
        del pl_, o_
    del x16
    x44 = torch.randn((256, 441000), device=dev)
    ms = t(lambda: audio_io.resample_batch(x44, 44100, 16000))
    L, M = audio_io.resample_ratio(44100, 16000)
    h, _ = audio_io.design_taps(L, M)
    tpo = -(-len(h) // L)                               # taps per output sample
    n_out = -(-441000 * L // M)
    out["N4_resample_44100_to_16000_256x441000"] = flops(
        ms, 2.0 * tpo * n_out * 256, FP32_VEC_TF, "fp32-matrix",
        f"2 x {tpo} taps per output x {n_out} outputs x 256 clips (polyphase FIR {L}/{M}, {len(h)} taps)")
    out["N4_resample_44100_to_16000_256x441000"]["hbm"] = hbm(ms, 256 * (441000 + n_out) * 4, "samples in + samples out")
    raw = torch.randint(0, 255, (256 * 441000 * 2 * 2,), dtype=torch.uint8, device=dev)
    pcm = torch.empty((2, 256 * 441000), dtype=torch.float32, device=dev)
    lib = _lib.load()
    st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    ms = t(lambda: lib.mm_pcm_decode_f32(raw.data_ptr(), 2, 2, 256 * 441000, pcm.data_ptr(), 256 * 441000, st))
    out["N4_pcm_decode_s16_stereo_256x441000"] = hbm(ms, 256 * 441000 * 2 * (2 + 4), "interleaved s16 in + planar f32 out")
    return out


def time_reference_call(torch, dev):
    """get_MFCCS_change(path_to_a_44.1_kHz_wav, 10000, ...) EXACTLY as the reference's UI calls it (script/main.py:750-769,
    UI_CALL above; the second variant is the function's own default tStep = 0.001, script/mfcc.py:296): wall ms per call
    with everything the drop-in does inside it -- RIFF parse, file read, H2D, PCM decode, 44.1 -> 10 kHz resampling, MFCC,
    change tail, D2H, Python -- beside the oracle's time for the same call on ONE host core (from the array already at
    10 kHz: the oracle has no decoder / resampler, row N4), and the change curve checked against that oracle call."""
    import tempfile
    import wave
    import numpy as np
    from modulation_mfcc_amd import get_MFCCS_change
    from modulation_mfcc_amd.audio_io import load_audio
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import mfcc_oracle as O
    try:
        from threadpoolctl import threadpool_limits
    except Exception:
        threadpool_limits = None
    sr_file, secs = 44100, 10.0
    y = O.synth_clip(424242, int(sr_file * secs), sr_file, "am")
    pcm = np.clip(np.round(y * 32767.0), -32768, 32767).astype("<i2")
    out = {"call": "get_MFCCS_change(path, 10000, channelN=0, tStep=0.005, winLen=0.025, n_mfcc=13, n_fft=512, minFreq=100, "
                   "maxFreq=10000, removeFirst=1, filtCutoff=12, filtOrd=6, diffMethod='grad', outFilter='iir', "
                   "outFiltType='low', outFiltCutOff=[12], outFiltLen=6, outFiltPolyOrd=3) -- script/main.py:750-769",
           "file": f"{secs:g} s mono 16-bit PCM WAVE at {sr_file} Hz"}
    with tempfile.TemporaryDirectory() as td:
        path = os.path.join(td, "clip.wav")
        with wave.open(path, "wb") as w:
            w.setnchannels(1); w.setsampwidth(2); w.setframerate(sr_file); w.writeframes(pcm.tobytes())
        y10 = load_audio(path, 10000)[0].cpu().numpy()           # what the device hands to the MFCC stage
        for tag, kw in (("ui_default_tStep_5ms", UI_CALL), ("function_default_tStep_1ms", dict(UI_CALL, tStep=0.001))):
            for _ in range(3):
                got, T = get_MFCCS_change(path, 10000, **kw)
            torch.cuda.synchronize()
            k = 20
            t0 = time.perf_counter()
            for _ in range(k):
                got, T = get_MFCCS_change(path, 10000, **kw)
            ms = (time.perf_counter() - t0) / k * 1e3
            # the oracle on one core (BLAS pinned to one thread), same call on the resampled array
            okw = dict(kw, outFiltCutOff=tuple(kw["outFiltCutOff"]))
            lim = threadpool_limits(1) if threadpool_limits else None
            O.get_MFCCS_change(y10, 10000, **okw)
            t0 = time.perf_counter()
            for _ in range(3):
                want, Tw = O.get_MFCCS_change(y10, 10000, **okw)
            cpu_ms = (time.perf_counter() - t0) / 3 * 1e3
            if lim is not None:
                lim.unregister() if hasattr(lim, "unregister") else None
            err = float(np.abs(got - want).max() / np.abs(want).max())
            out[tag] = {"frames": int(len(T)), "wall_ms_per_call": round(ms, 3), "oracle_one_core_ms_per_call": round(cpu_ms, 2),
                        "oracle_excludes": "WAVE decode and the 44.1 -> 10 kHz resampling (soxr in the reference; row N4)",
                        "check": {"max_rel_change_curve": err, "T_equal": bool(np.array_equal(T, Tw)), "tolerance": 1e-4,
                                  "ok": bool(err <= 1e-4 and np.array_equal(T, Tw)),
                                  "against": "oracle.get_MFCCS_change on the device-resampled array (the suite's bound for the curve: 1e-4 of its maximum)"}}
    return out


def roofline_of(cfg, B, T, n_mod, with_mod, per_stage, fused_dct, traffic_key=None, fused_tail=False):
    spec_rows = 8 * (n_mod // 2 + 1) * cfg.n_mfcc / T if fused_tail else 0
    # ALGORITHMIC bytes of what the launch computes -- a kernel that goes from samples to MFCCs (the
    # fused DCT) counts unique audio in + MFCC out (+ the modulation-spectrum rows where the whole tail runs in the
    # launch): 4 hop + 4 n_mfcc (+ spectrum) = 692 (745) B/frame at configs[1] ([2]); a kernel that stops at the
    # log-mel rows counts audio in + log-mel out.  What the IMPLEMENTATION moves on top (the log-mel rows the fused
    # kernel still stores for the rare clamp fix-up) is reported beside it, never in `frac`.
    alg = {
        "logmel": 4 * cfg.hop_length + (4 * cfg.n_mfcc if fused_dct else 4 * cfg.n_mels) + spec_rows,
        "dct": 4 * cfg.n_mels + 4 * cfg.n_mfcc,            # log-mel in + MFCC out
        "modspec": (4 * T + 8 * (n_mod // 2 + 1)) * cfg.n_mfcc / T if with_mod else 0,
    }
    impl = dict(alg)
    impl["logmel"] = 4 * cfg.hop_length + 4 * cfg.n_mels + (4 * cfg.n_mfcc if fused_dct else 0) + spec_rows \
        + (4 * cfg.n_mfcc if fused_tail else 0)            # + the MFCC rows read back by the in-launch trajectory rFFT
    dom = max(per_stage, key=lambda k: per_stage[k]["avg_ms"])
    if dom not in alg:
        return None
    bytes_launch = alg[dom] * B * T
    ach = bytes_launch / (per_stage[dom]["avg_ms"] * 1e-3) / 1e9
    traffic, src = pmc_traffic(traffic_key) if traffic_key else (None, None)
    out = {"kernel": dom, "bound": "hbm", "achieved": ach, "peak": HBM_PEAK_GBS, "unit": "GB/s",
           "frac": ach / HBM_PEAK_GBS, "traffic": traffic, "traffic_source": src,
           "algorithmic_bytes_per_launch": bytes_launch, "algorithmic_bytes_per_frame": alg[dom],
           "implementation_bytes_per_frame": impl[dom],
           "avg_launch_ms": per_stage[dom]["avg_ms"], "launches_timed": per_stage[dom]["launches"]}
    if dom == "logmel":
        # for information: the fused kernel is issue / LDS bound, not HBM bound -- its
        # algorithmic flops (rFFT 2.5 N log2 N + power + sparse mel + log + DCT) against the FP32 vector peak
        n = cfg.n_fft
        import math
        flops = 2.5 * n * math.log2(n) + 3 * (n // 2 + 1) + 4 * (n // 2 + 1) + cfg.n_mels + (2 * cfg.n_mels * cfg.n_mfcc if fused_dct else 0)
        tf = flops * B * T / (per_stage[dom]["avg_ms"] * 1e-3) / 1e12
        out["fp32_vector"] = {"algorithmic_flops_per_frame": flops, "achieved": tf, "peak": 157.3, "unit": "TFLOP/s",
                              "frac": tf / 157.3}
    return out


DUMP_BYTES_MAX = 48 << 20       # --dump-outputs: bytes of all arrays together, at most
DUMP_ROW_SEED = 1234


def dump_outputs(torch, outdir, arrays, R):
    """arrays: {name: device tensor [R, ...], float32 or complex64} -> outdir/<name>.npy, float32 (complex: a trailing axis
    of 2, real and imaginary part).  Every row when all arrays fit DUMP_BYTES_MAX together, otherwise the same fixed sample
    of rows of each: the first k of numpy.random.RandomState(DUMP_ROW_SEED).permutation(R), in ascending order."""
    import numpy as np
    per_row = sum(t[0].numel() * t.element_size() for t in arrays.values())
    idx = None
    if R * per_row > DUMP_BYTES_MAX:
        k = max(1, DUMP_BYTES_MAX // per_row)
        idx = np.sort(np.random.RandomState(DUMP_ROW_SEED).permutation(R)[:k])
    os.makedirs(outdir, exist_ok=True)
    files = {}
    for name, t in arrays.items():
        if idx is not None:
            t = t.index_select(0, torch.from_numpy(idx).to(t.device))
        if t.is_complex():
            t = torch.view_as_real(t)
        x = t.to(torch.float32).cpu().numpy()
        np.save(os.path.join(outdir, name + ".npy"), x)
        files[name + ".npy"] = list(x.shape)
    rows = "all" if idx is None else {"count": int(len(idx)), "of": R, "seed": DUMP_ROW_SEED,
                                      "rule": "first count of numpy.random.RandomState(seed).permutation(of), sorted"}
    return {"rows": rows, "files": files}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--workload", default="c3", choices=sorted(WORKLOADS))
    ap.add_argument("--clips", type=int, default=0, help="override clips per GPU (debug)")
    ap.add_argument("--full", action="store_true",
                    help="also the CPU baseline, the oracle checks, the per-kernel / roofline figures, the other sections "
                         "(c2 / c4 / refdefault / rFFT stage / rows around the hot path) and, N > 1, the other gather variant")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the last timed step's outputs (rank 0) as DIR/<name>.npy, float32")
    ap.add_argument("--settle-ms", type=float, default=300.0,
                    help="untimed steps for this long before the warm-up steps (clocks out of their idle state)")
    ap.add_argument("--no-cpu", action="store_true", help="--full without the CPU baseline")
    ap.add_argument("--no-check", action="store_true",
                    help="--full without the oracle spot-check of three output clips (and, in any run, without those clips "
                         "in the batch)")
    ap.add_argument("--no-extra", action="store_true", help="--full without the c2 / c4 / rFFT-stage passes (profiling runs)")
    ap.add_argument("--generic", action="store_true", help="force the generic kernels")
    ap.add_argument("--no-fuse-tail", action="store_true", help="separate launches for the clamp fix-up and the trajectory rFFT (development A/B)")
    ap.add_argument("--variant", default=None, help="pin a fused-kernel variant (m12, w16s, w16, w8, wpf): development A/B")
    ap.add_argument("--gather", default="full", choices=["mfcc", "full"],
                    help="N > 1: 'full' (default, the literal north star) -- every rank computes MFCC + modulation spectrum of "
                         "its clips in its one fused launch and both arrays travel in the ONE gather; 'mfcc' -- only the MFCC "
                         "slab travels (half the bytes over xGMI) and the root transforms the gathered trajectories.  `value` is "
                         "the one named here; with --full BOTH are timed with the same number of steps and reported side "
                         "by side (value_literal, value_mfcc_only)")
    a = ap.parse_args()

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if a.gpus != world and world > 1:
        raise SystemExit(f"--gpus {a.gpus} but WORLD_SIZE={world}")
    if a.gpus > 1 and world == 1:
        raise SystemExit("launch N>1 with python -m torch.distributed.run --nproc-per-node N bench.py --gpus N")
    # before anything initialises HIP/HSA: the host driver only supports dmabuf IPC
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    use_dist = world > 1 or bool(os.environ.get("MM_BENCH_FORCE_DIST"))
    if use_dist:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29533")

    # Anything libraries print on stdout (RCCL prints a version banner there at communicator init)
    # goes to stderr: stdout carries exactly ONE line, the JSON result.
    sys.stdout.flush()
    real_stdout = os.dup(1)
    os.dup2(2, 1)

    idx, B, ch, secs, kw, with_mod = WORKLOADS[a.workload]
    if a.clips:
        B = a.clips
    cpu = None
    if a.full and world == 1 and rank == 0 and not a.no_cpu:
        cpu = cpu_baseline(kw, int(secs * kw["sr"]), with_mod)      # no torch / HIP yet in this process
    check_vecs = {}
    if rank == 0 and not a.no_check and not a.full:
        # the oracle's three clips without the oracle's answers: the batch is the one a --full run times
        sys.path.insert(0, os.path.join(ROOT, "oracle"))
        import mfcc_oracle as O
        n_ = int(secs * kw["sr"])
        check_vecs = {a.workload: [(O.synth_clip(sd, n_, kw["sr"], "am"), None, None) for sd in CHECK_SEEDS]}
    elif rank == 0 and not a.no_check:
        jobs = {a.workload: (kw, int(secs * kw["sr"]), with_mod)}
        if world == 1 and not a.no_extra:
            for nm in ("c2", "c4", "refdefault"):
                if nm != a.workload:
                    _, _, _, s_, k_, _ = WORKLOADS[nm]
                    if k_ is kw and int(s_ * k_["sr"]) == int(secs * kw["sr"]):
                        continue                              # same signal and configuration as the headline: shared
                    jobs[nm] = (k_, int(s_ * k_["sr"]), nm == "refdefault")
        check_vecs = oracle_check_vectors(jobs)
        for nm in ("c2", "c4", "refdefault"):
            if nm not in check_vecs and WORKLOADS[nm][4] is kw:
                check_vecs[nm] = check_vecs[a.workload]
    check_vec = check_vecs.get(a.workload)

    import torch
    import torch.distributed as dist
    from modulation_mfcc_amd import MfccConfig, MfccPlan, _lib
    from modulation_mfcc_amd.dist import PipelinedGather, SlabLayout

    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    # MM_BENCH_FORCE_DIST=1: take the N>1 code path (process group, pipelined gather) even with a
    # single rank -- a rehearsal of that path on a 1-GPU box
    if use_dist:
        dist.init_process_group("nccl", device_id=dev, rank=rank, world_size=world)

    def make(name, rows_override=0):
        _, b, c, s, k, wm = WORKLOADS[name]
        if rows_override:
            b = rows_override
        cfg = MfccConfig(**k)
        n = int(s * cfg.sr)
        plan = MfccPlan(cfg)
        if a.generic:
            plan.force_generic(True)
        if a.variant:
            plan.set_variant(a.variant)
        if a.no_fuse_tail:
            plan.set_fuse_tail(False)
        audio = synth_batch(torch, dev, b * c, n, cfg.sr, seed0=1000 * rank)
        if c > 1:                      # [B, ch, n]: the rows the kernels see are the channels, stride n
            audio = audio.view(b, c, n)
        return cfg, plan, audio, n, cfg.num_frames(n)

    cfg, plan, audio, n, T = make(a.workload, a.clips)
    rows = audio.reshape(-1, n)
    R = rows.shape[0]
    check_rows = sorted({0, R // 2, R - 1})
    if check_vec is not None:           # three rows of the timed batch carry clips whose oracle answer is known
        for r_, (clip_, _, _) in zip(check_rows, check_vec):
            rows[r_].copy_(torch.from_numpy(clip_))

    # one flat output slab per rank so that a single gather per step moves everything; with N > 1
    # the slabs are double-buffered and the gather of step k runs on a side stream under the
    # kernels of step k+1 (every step's gather still completes inside the timed region)
    # N > 1, --gather mfcc: the modulation spectrum is a linear map of the MFCC trajectories, so only
    # the MFCC slab travels and the root runs ONE trajectory rFFT over the gathered block on the
    # gather's side stream (modulation_mfcc_amd/dist.py)
    n_mod = cfg.mod_fft_len(T) if with_mod else 0
    plan.workspace(R, n)

    def run_variant(gather_mode, steps, warmup):
        mod_on_root = use_dist and with_mod and gather_mode == "mfcc"
        lay = SlabLayout.make(cfg, R, n, with_mod and not mod_on_root)
        pg = PipelinedGather(lay.numel, dev) if use_dist else None
        if pg and a.full:
            pg.time_every(EVENT_EVERY)
        last = {}
        slab1 = torch.empty(lay.numel, dtype=torch.float32, device=dev) if not use_dist else None
        mod_all = None
        if mod_on_root and rank == 0:
            mod_all = [torch.empty((world * R, cfg.n_mfcc, n_mod // 2 + 1), dtype=torch.complex64, device=dev)
                       for _ in range(pg.depth)]

        def root_modspec(i):        # runs inside the gather's side stream, root only
            got = pg.recv_block[i][:, :lay.mfcc_numel].reshape(world * R, cfg.n_mfcc, T)
            plan.modspec(got, out=mod_all[i])
            last["mod_root"] = mod_all[i][:R]           # rank 0's rows come first in the gathered block

        def compute(slab):
            mfcc_out, mod_out = lay.views(slab)
            if with_mod and not mod_on_root:
                plan.mfcc_modspec(rows, out=mfcc_out, out_mod=mod_out)    # one launch where the plan can (fused tail)
            else:
                plan.mfcc(rows, out=mfcc_out)
            return mfcc_out, mod_out

        def step():
            slab = pg.acquire() if pg else slab1
            last["mfcc"], last["mod"] = compute(slab)
            if pg:
                pg.submit(post=root_modspec if mod_on_root else None)

        def drain():
            if pg:
                pg.finish()
            if use_dist:
                dist.barrier()

        # the kernels of the step without its gather (no collective: the ranks may settle for different numbers of calls),
        # into a slab no gather has used yet
        settle_slab = pg.slabs[0] if pg else slab1
        settled = settle(torch, lambda: compute(settle_slab), a.settle_ms * 1e-3)
        if pg:
            for _ in range(warmup):
                step()
            drain()
            pg.gather_ms()              # discard the warm-up gathers' events (communicator set-up is in the first one)
            dt, stage = time_steps(torch, plan, step, steps, 0, ["logmel"], sync=drain, events=a.full)
        else:
            dt, stage = time_steps(torch, plan, step, steps, warmup, ["logmel"], sync=drain, events=a.full)
        last["settle_calls"] = settled
        per_rank = None
        if use_dist:
            tt = torch.tensor([dt], dtype=torch.float64, device=dev)
            dist.all_reduce(tt, op=dist.ReduceOp.MAX)
            dt = float(tt.item())
        if use_dist and a.full:
            # per rank: device time of the step's kernels (HIP events, every EVENT_EVERY-th step) and of its gather as
            # the side stream saw it -- what separates "compute" from "wire" in the scaling curve
            g_ms, g_n = pg.gather_ms()
            c_ms = sum(v[0] / v[1] for v in stage.values() if v[1])
            mine = torch.tensor([c_ms, g_ms, float(g_n)], dtype=torch.float64, device=dev)
            allr = [torch.zeros_like(mine) for _ in range(world)]
            dist.all_gather(allr, mine)
            per_rank = [{"rank": i, "compute_ms": round(float(v[0]), 4), "gather_ms": round(float(v[1]), 4),
                         "gathers_timed": int(v[2])} for i, v in enumerate(allr)]
        if pg is not None and rank == 0 and os.environ.get("MM_BENCH_FORCE_DIST"):
            # rehearsal check: what arrived at the root is what the last steps produced
            li = (pg.k - 1) % pg.depth
            assert torch.equal(pg.received[li][0], pg.slabs[li]), "gathered slab differs"
        return dt, stage, mod_on_root, last, per_rank, lay

    def run_extras():
        """The bench's other sections -- stage-isolated rFFT, device copy, BASELINE configs[1] and configs[3] -- run
        BEFORE the headline region: they are ~100 ms of GPU work, after which the clocks are at their steady state
        (with the driver's 5 warmup steps = 2.5 ms alone, the 10 ms timed region falls into the clock ramp and reads
        15 % slow: 0.50 vs 0.43 ms per step on the same box)."""
        ex = {}
        # ---- ONE recording through the drop-in call, as the reference's UI makes it: FIRST of the sections -- its host
        # work (file I/O, Python, the oracle's CPU time) leaves the GPU idle, and the headline region must not follow it
        if world == 1:
            try:
                ex["refdefault_call"] = time_reference_call(torch, dev)
            except Exception as e:
                ex["refdefault_call"] = {"error": repr(e)}
        # ---- the rows either side of the hot path, for the record (N = 1 only); FIRST: measured
        # right before the headline region their double-precision kernels left it 10 % slower (0.49 vs 0.44 ms) ----
        if world == 1:
            try:
                ex["next_rows"] = time_next_rows(torch, dev)
            except Exception as e:          # never let a side measurement take the bench down
                ex["next_rows"] = {"error": repr(e)}
            torch.cuda.empty_cache()
        # ---- stage-isolated batched rFFT (frames in -> complex bins out), same process ---------
        nrows = R * T
        frames_buf = torch.randn((nrows, cfg.n_fft), device=dev, dtype=torch.float32)
        spec = torch.empty((nrows, cfg.n_bins), dtype=torch.complex64, device=dev)
        for _ in range(3):
            plan.rfft(frames_buf, cfg.n_fft, out=spec)
        torch.cuda.synchronize()
        plan.timing_enable(True)
        for _ in range(10):
            plan.rfft(frames_buf, cfg.n_fft, out=spec)
        plan.timing_enable(False)
        ms, cnt = plan.timing_read()["rfft"]
        bpf = 4 * cfg.n_fft + 8 * cfg.n_bins
        ach = nrows * bpf / (ms / cnt * 1e-3) / 1e9
        ex["rfft_stage"] = {"kernel": "batched rFFT-%d, %d rows" % (cfg.n_fft, nrows), "bound": "hbm",
                             "achieved": ach, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                             "frac": ach / HBM_PEAK_GBS, "algorithmic_bytes_per_frame": bpf,
                             "frames_per_s": nrows / (ms / cnt * 1e-3), "avg_launch_ms": ms / cnt}
        # practical HBM ceiling of this device: float4 grid-stride copy kernel of the library (bytes
        # read + written), on the same stream, timed with events
        src_c = frames_buf.view(-1)[: (1 << 28)]              # 1 GiB
        dst_c = torch.empty_like(src_c)
        lib = _lib.load()
        st = torch.cuda.current_stream(dev).cuda_stream
        for _ in range(2):
            _lib.check(lib.mm_devcopy_f32(src_c.data_ptr(), dst_c.data_ptr(), src_c.numel(), st), "mm_devcopy_f32")
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(5):
            lib.mm_devcopy_f32(src_c.data_ptr(), dst_c.data_ptr(), src_c.numel(), st)
        e1.record()
        torch.cuda.synchronize()
        copy_gbs = 5 * 2 * src_c.numel() * 4 / (e0.elapsed_time(e1) * 1e-3) / 1e9
        ex["rfft_stage"]["device_copy_GBs"] = copy_gbs
        ex["rfft_stage"]["frac_of_device_copy"] = ach / copy_gbs
        ex["_copy_gbs"] = copy_gbs
        del frames_buf, spec, src_c, dst_c

        # ---- the other single-GPU configurations, same process (N = 1 only) --------------------
        if world == 1:
            import numpy as np
            for name in ("c2", "c4", "refdefault"):
                if name == a.workload:
                    continue
                c2, p2, audio2, n2, T2 = make(name)
                rows2 = audio2.reshape(-1, n2)
                R2 = rows2.shape[0]
                vec2 = check_vecs.get(name)
                crow2 = sorted({0, R2 // 2, R2 - 1})
                if vec2 is not None:
                    for r_, (clip_, _, _) in zip(crow2, vec2):
                        rows2[r_].copy_(torch.from_numpy(clip_))
                out2 = torch.empty((R2, c2.n_mfcc, T2), dtype=torch.float32, device=dev)
                p2.workspace(R2, n2)
                # (enough steps behind enough warm-up for steady clocks: with 10 steps behind 2 the 2 ms configs[3] step read 10 %
                # slower than in a 200-step run of the same kernels on the same box)
                k = max(30, a.steps)
                dt2, st2 = time_steps(torch, p2, lambda: p2.mfcc(rows2, out=out2), k, 10, ["logmel"])
                ps = {kk: {"avg_ms": v[0] / v[1], "launches": v[1]} for kk, v in st2.items()}
                key2 = {"radix16-w16s": s16_kernel_key(c2, 1), "radix16-m12": "logmel12m", "radix16-wpf": "logmel_wpf"}.get(p2.kernel_path)
                ex[name] = {"workload": workload_label(name, WORKLOADS[name][1], T2, c2, 0),
                             "metric": "MFCC frames/sec", "value": R2 * T2 * k / dt2, "unit": "frames/s",
                             "ms_per_step": 1e3 * dt2 / k, "steps": k, "kernel_path": p2.kernel_path,
                             "fused_dct": bool(p2.fused_dct), "launches_per_step": len(ps),
                             "ns_per_frame_mel": 1e9 * dt2 / k / (R2 * T2 * c2.n_mels),
                             "kernels_ms": {kk: round(v["avg_ms"], 4) for kk, v in ps.items()},
                             "roofline": roofline_of(c2, R2, T2, 0, False, ps, p2.fused_dct, key2)}
                if vec2 is not None:
                    ex[name]["check"] = compare_rows(np, out2, None, crow2, vec2)
                if name == "refdefault":
                    # the same batch through the headline entry point (MFCC + modulation spectrum of the trajectories)
                    nm2 = c2.mod_fft_len(T2)
                    mod2 = torch.empty((R2, c2.n_mfcc, nm2 // 2 + 1), dtype=torch.complex64, device=dev)
                    dt3, st3 = time_steps(torch, p2, lambda: p2.mfcc_modspec(rows2, out=out2, out_mod=mod2), k, 5, ["logmel"])
                    ps3 = {kk: {"avg_ms": v[0] / v[1], "launches": v[1]} for kk, v in st3.items()}
                    ft3 = bool(p2.fused_tail(R2, n2))
                    ex[name]["with_modspec"] = {
                        "metric": "MFCC+mod-spectrum frames/sec", "value": R2 * T2 * k / dt3, "unit": "frames/s",
                        "ms_per_step": 1e3 * dt3 / k, "steps": k, "n_mod": nm2, "fused_tail": ft3,
                        "launches_per_step": 1 if ft3 else len(ps3),
                        "kernels_ms": {kk: round(v["avg_ms"], 4) for kk, v in ps3.items()},
                        "roofline": roofline_of(c2, R2, T2, nm2, True, ps3, p2.fused_dct,
                                                s16_kernel_key(c2, 2) if ft3 else key2, fused_tail=ft3)}
                    if vec2 is not None:
                        ex[name]["with_modspec"]["check"] = compare_rows(np, out2, mod2, crow2, vec2)
                    del mod2
                del out2, audio2, rows2
                torch.cuda.empty_cache()
            if "c2" in ex and "refdefault" in ex:
                ex["refdefault"]["vs_c2_per_frame_mel"] = ex["refdefault"]["ns_per_frame_mel"] / ex["c2"]["ns_per_frame_mel"]
        return ex

    extras = run_extras() if a.full and not a.no_extra else {}
    dt, stage, mod_on_root, last, per_rank, lay = run_variant(a.gather, a.steps, a.warmup)
    dumped = None
    if a.dump_outputs and rank == 0:
        outs = {"mfcc": last["mfcc"]}
        mod_ = last["mod"] if last["mod"] is not None else last.get("mod_root")
        if mod_ is not None:
            outs["modspec"] = mod_
        dumped = dump_outputs(torch, a.dump_outputs, outs, R)
    # ---- spot-check of the TIMED output against the oracle, outside the timed region: the three rows that carry the
    # oracle's clips, MFCC (north-star bound: 1e-4 of max|MFCC|) and modulation spectrum ----
    check = None
    if a.full and check_vec is not None and rank == 0:
        import numpy as np
        check = compare_rows(np, last["mfcc"], last["mod"], check_rows, check_vec)
    frames_total = world * R * T * a.steps
    res = {
        "metric": "MFCC+mod-spectrum frames/sec" if with_mod else "MFCC frames/sec",
        "value": frames_total / dt, "unit": "frames/s", "n_gpus": world, "steps": a.steps,
        "warmup": a.warmup, "ms_per_step": 1e3 * dt / a.steps, "higher_is_better": True,
        "scaling": "weak", "vs_baseline": None, "dtype": "f32", "data": "synthetic",
        "config": {"workload": workload_label(a.workload, B, T, cfg, n_mod),
                   "frames_per_clip": T, "clips_total": world * B, "kernel_path": plan.kernel_path,
                   "parallelism": f"clips sharded x{world}" + (", one RCCL gather per step (overlapped with the next step's kernels)" if world > 1 else "")
                                  + ("; MFCC slab gathered, modulation spectrum of the gathered trajectories computed on the root" if mod_on_root else ""),
                   "gather": (a.gather if use_dist else None),
                   "rccl_ranks": (dist.get_world_size() if use_dist else None),
                   "gather_bytes_per_rank": (lay.numel * 4 if use_dist else None),
                   "csrc_sha16": csrc_sha16(),
                   "hsa_ipc_mode_legacy": os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY"),
                   "settle_ms": a.settle_ms, "settle_calls": last["settle_calls"], "full": a.full},
    }
    if dumped is not None:
        res["dump"] = dumped
    if a.full and use_dist and with_mod:
        # the other gather variant, SAME steps and warm-up, reported as a top-level peer of `value`
        other = "full" if a.gather == "mfcc" else "mfcc"
        dt2, _, _, _, per_rank2, lay2 = run_variant(other, a.steps, a.warmup)
        if rank == 0:
            def variant(mode, dt_, per_rank_, lay_):
                root = [r for r in per_rank_ if r["rank"] == 0][0]
                rest = [r for r in per_rank_ if r["rank"] != 0]
                return {"gather": mode, "value": world * R * T * a.steps / dt_, "unit": "frames/s", "ms_per_step": 1e3 * dt_ / a.steps,
                        "steps": a.steps, "gather_bytes_per_rank": lay_.numel * 4,
                        "root_compute_ms": root["compute_ms"], "root_gather_ms": root["gather_ms"],
                        "other_ranks_compute_ms_max": (max(r["compute_ms"] for r in rest) if rest else None),
                        "other_ranks_compute_ms_mean": (sum(r["compute_ms"] for r in rest) / len(rest) if rest else None),
                        "per_rank": per_rank_,
                        "what": ("literal north star: every rank computes MFCC + modulation spectrum (one fused launch), both "
                                 "arrays in the one gather" if mode == "full" else
                                 "MFCC slab gathered; the root computes the modulation spectrum of ALL gathered trajectories on "
                                 "the gather's side stream (the root's compute_ms includes that rFFT: the plan's event timer "
                                 "records it as a stage)")}
            mine, theirs = variant(a.gather, dt, per_rank, lay), variant(other, dt2, per_rank2, lay2)
            res["value_literal"] = (mine if a.gather == "full" else theirs)["value"]
            res["value_mfcc_only"] = (mine if a.gather == "mfcc" else theirs)["value"]
            res["gather_variants"] = {a.gather: mine, other: theirs}

    parity_failed, all_checks = False, {}
    if rank == 0:
        ftail = bool(with_mod and not mod_on_root and plan.fused_tail(R, n))
        res["config"]["fused_tail"] = ftail
        if ftail:
            res["config"]["launches_per_step"] = 1
    if rank == 0 and a.full:
        # ---- roofline of the dominant kernel, from HIP events recorded around every launch -----
        # the n_fft 512 tile kernels also apply the (unclamped) DCT: their launch stores the MFCC rows too
        fused = plan.fused_dct
        per_stage = {k: {"avg_ms": v[0] / v[1], "launches": v[1]} for k, v in stage.items()}
        res["kernels_ms"] = {k: round(v["avg_ms"], 4) for k, v in per_stage.items()}
        key = {"radix16-w16s": s16_kernel_key(cfg, 1), "radix16-m12": "logmel12m", "radix16-wpf": "logmel_wpf"}.get(plan.kernel_path)
        if ftail:
            key = s16_kernel_key(cfg, 2)        # the clip-mode instantiation
        res["config"]["launches_per_step"] = 1 if ftail else (len(per_stage) if per_stage else None)
        rl = roofline_of(cfg, R, T, n_mod, with_mod, per_stage, fused, key, fused_tail=ftail)
        if rl:
            res["roofline"] = rl

        res["config"]["sections_before_headline"] = sorted(k_ for k_ in extras if not k_.startswith("_"))
        for k_, v_ in extras.items():
            if k_ != "_copy_gbs":
                res[k_] = v_
        if "_copy_gbs" in extras and "roofline" in res:
            res["roofline"]["device_copy_GBs"] = extras["_copy_gbs"]

        if per_rank is not None:
            res["per_rank"] = per_rank
        if check is not None:
            res["check"] = check
        # every oracle check of this run in one verdict; a failed check makes the run FAIL (exit code 3 after the line)
        def _checks(d, path=""):
            if isinstance(d, dict):
                for k_, v_ in d.items():
                    if k_ == "check" and isinstance(v_, dict) and "ok" in v_:
                        yield path + "check", v_["ok"]
                    else:
                        yield from _checks(v_, path + k_ + ".")
        all_checks = dict(_checks(res))
        res["parity_ok"] = bool(all(all_checks.values())) if all_checks else None
        res["parity_checks"] = all_checks
        parity_failed = res["parity_ok"] is False
        if cpu is not None:
            res["cpu_baseline"] = cpu
    if rank == 0:
        sys.stdout.flush()
        os.dup2(real_stdout, 1)
        print(json.dumps(res), flush=True)
        os.dup2(2, 1)

    if use_dist:
        dist.barrier()
        dist.destroy_process_group()
    if rank == 0 and parity_failed:
        print("bench.py: an oracle check of the timed output FAILED: " + json.dumps({k: v for k, v in all_checks.items() if not v}),
              file=sys.stderr, flush=True)
        sys.exit(3)


if __name__ == "__main__":
    main()
