"""The registry behind tests/test_stream_host.py and tests/test_gpu_streams.py: every compute entry of include/modmfcc.h
(every prototype whose last parameter is ``void* stream``) in every form, i.e. every distinct launch sequence, as a case
that can be called again and again on the same buffers.

A case has a ``name``, the C symbol it reaches (``entry``), its ``family`` and

  data()          the two data sets as HOST arrays, {buffer: (set 0, set 1)} -- numpy only, no GPU, no library; a ragged
                  case's lengths tensor is one of the buffers (set 1: a row at n_max, a row at the smallest length the
                  entry admits, rows in between);
  prepare(gpu)    -> Prepared: the plan or handle, the input buffers, both data sets staged on the device, the outputs the
                  case owns and the workspace, made once;
  Prepared.fill(k)   data set k into the input buffers, device to device (copy_), nothing on the host;
  Prepared.call()    the call on torch.cuda.current_stream() AS READ AT CALL TIME -> the tuple of output tensors.

call() goes through the lowest function of the package that reaches the entry (MfccPlan.mfcc, filters.sosfiltfilt_batch,
calc.find_peaks_batch ...), so that the wrapper's share of the contract is held too, and through ctypes where that function
works on host data by design: a path (mm_pcm_decode_f32), host-side validation that reads the data back (interp_nan_batch),
or a workspace the MfccPlan object owns (the thread cases of mm_mfcc_f32 and its kin need one per thread).  Host-side
arguments -- SOS sections, mm_pyin_params, peak conditions -- are the same in both sets: a captured graph bakes them in.

Shapes are the smallest that still take the form; every prepare() asserts the form where the library can tell
(kernel_path, fused_tail, mm_hilbert_fft_size).
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

CASES = []
_NAMES = set()


class Case:
    def __init__(self, name, entry, family, data, setup, ragged=False, threads=False, host_sync=None, tol=None):
        assert name not in _NAMES, name
        _NAMES.add(name)
        self.name, self.entry, self.family = name, entry, family
        self.data, self.setup = data, setup
        self.ragged = ragged            # one of the buffers is a lengths tensor the kernels read
        self.threads = threads          # takes an mm_plan* / mm_hilbert* (or is mm_pyin_f32): test C runs it on two threads
        # host_sync: None, or the sentence of the wrapper's documentation that announces a read-back -- such a case must
        # be SEEN to wait in test A (the detector agrees with the documentation) and cannot be captured
        self.host_sync = host_sync
        # tol: None = bit for bit; otherwise (existing test file, rtol of the output's maximum) for an entry SHOWN not to be
        # reproducible run to run.  No registered case has one.
        self.tol = tol

    def prepare(self, gpu, shared=None):
        return Prepared(self, gpu, shared)

    def __repr__(self):
        return self.name


class Prepared:
    def __init__(self, case, gpu, shared=None):
        import torch
        self.case, self.gpu = case, gpu
        self.shared = {} if shared is None else shared      # the plan / handle two thread instances have in common
        host = case.data()
        self.staged = [{k: torch.from_numpy(np.ascontiguousarray(v[i])).to(gpu) for k, v in host.items()} for i in (0, 1)]
        self.buf = {k: torch.empty_like(t) for k, t in self.staged[0].items()}
        self.outs, self.keep = [], []
        with torch.cuda.device(gpu):
            self._call = case.setup(self)
        self.fill(0)

    def out(self, shape, dtype):
        """An output buffer the case owns (poisoned before every checked call)."""
        import torch
        t = torch.empty(tuple(int(s) for s in shape), dtype=dtype, device=self.gpu)
        self.outs.append(t)
        return t

    def work(self, nbytes):
        import torch
        return torch.empty(max(int(nbytes), 16), dtype=torch.uint8, device=self.gpu)

    def plan(self, make):
        """The plan of the case: made once per `shared` dict (two thread instances use the same one)."""
        if "plan" not in self.shared:
            self.shared["plan"] = make()
        return self.shared["plan"]

    def fill(self, k):
        for key, b in self.buf.items():
            b.copy_(self.staged[k][key])

    def poison(self):
        """All bits set in every output the case owns: NaN in floats, -1 in integers."""
        import torch
        for o in self.outs:
            (torch.view_as_real(o) if o.is_complex() else o).view(torch.uint8).fill_(0xFF)

    def call(self):
        import torch
        r = self._call()
        r = (r,) if isinstance(r, torch.Tensor) else tuple(r)
        flat = []
        for t in r:
            if isinstance(t, dict):
                flat.extend(t[k] for k in sorted(t))
            elif t is not None:
                flat.append(t)
        return tuple(flat)


def stream():
    """The current stream, read now, as the C ABI takes it."""
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _lib():
    from modulation_mfcc_amd import _lib as L
    return L, L.load()


def _ok(rc, what):
    L, _ = _lib()
    L.check(rc, what)


def add(*a, **kw):
    CASES.append(Case(*a, **kw))


# ---- host data ----------------------------------------------------------------------------------------------------------
def _seed(name, k):
    # (hash() of a str is salted per process: a fixed digest instead)
    import zlib
    return np.random.default_rng([zlib.crc32(name.encode()), k])


def audio_sets(name, B, n, dtype=np.float32, pitch=None, clamp_row=None):
    """Two sets of B clips: a tone per clip plus noise, other tones and another seed in set 1.  clamp_row: that clip is loud
    in its first half and 1e-6 of it in its second (its log-mel minimum lies more than top_db under its maximum)."""
    out = []
    for k in (0, 1):
        r = _seed(name, k)
        t = np.arange(n) / 16000.0
        f = r.uniform(100, 900, size=(B, 1))
        x = 0.3 * np.sin(2 * np.pi * f * t[None, :]) + 0.05 * r.standard_normal((B, n))
        if clamp_row is not None:
            x[clamp_row] = 0.5 * r.standard_normal(n)
            x[clamp_row, n // 2:] *= 1e-6
        a = np.zeros((B, pitch or n), dtype=dtype)
        a[:, :n] = x
        out.append(a)
    return tuple(out)


def curve_sets(name, rows, n, dtype=np.float64, pitch=None):
    """Two sets of smooth curves with noise (filters, stencils, peaks)."""
    out = []
    for k in (0, 1):
        r = _seed(name, k)
        t = np.arange(n)[None, :]
        x = np.sin(2 * np.pi * t / r.uniform(20, 200, size=(rows, 1))) + 0.2 * r.standard_normal((rows, n))
        a = np.zeros((rows, pitch or n), dtype=dtype)
        a[:, :n] = x
        out.append(a)
    return tuple(out)


def length_sets(rows, n_max, least):
    """(set 0, set 1) int64 [rows]: set 1 has a row at n_max, a row at `least`, rows in between; set 0 differs in every row."""
    assert rows >= 3 and least < n_max
    one = np.empty(rows, dtype=np.int64)
    one[0], one[1] = n_max, least
    one[2:] = np.linspace(least + (n_max - least) // 3, n_max - 1, rows - 2, dtype=np.int64)
    zero = np.clip(n_max + least - one + ((np.arange(rows) % 3) - 1), least, n_max)
    zero = np.where(zero == one, np.clip(one - 1, least, n_max), zero)
    zero = np.where(zero == one, one + 1, zero)
    assert (zero != one).all() and zero.min() >= least and zero.max() <= n_max
    return zero.astype(np.int64), one.astype(np.int64)


# ---- the MFCC front end (mm_plan) -----------------------------------------------------------------------------------------
C1 = dict(sr=16000, n_fft=512, win_length=400, hop_length=160, n_mels=40, n_mfcc=13, fmin=100.0, fmax=8000.0)
C1K = dict(sr=16000, n_fft=1024, win_length=1024, hop_length=256, n_mels=64, n_mfcc=13, fmin=50.0, fmax=8000.0)
C2K = dict(sr=22050, n_fft=2048, win_length=2048, hop_length=512, n_mels=80, n_mfcc=13, fmin=50.0, fmax=11025.0)
REF_DEFAULT = dict(sr=10000, n_fft=512, win_length=250, hop_length=50, n_mels=128, n_mfcc=13, fmin=100.0, fmax=10000.0)
ANY400 = dict(C1, n_fft=400)                                    # 200 = 8 x 25 complex points: the two-register-stage kernel
ANY360 = dict(C1, n_fft=360, win_length=360)                    # 180 = 2^2 3^2 5: no such pair, the Stockham passes in LDS
EMB256 = dict(sr=8000, n_fft=256, win_length=200, hop_length=80, n_mels=40, n_mfcc=13, fmin=50.0, fmax=4000.0)
ANY502 = dict(C1, n_fft=502)                                    # 251 is prime: Bluestein

# name -> (config, set-up of a fresh plan, the kernel path it must report)
PLANS = {
    "p0-generic": (C1, lambda p: p.force_generic(True), "generic"),
    "p1-w8": (C1, lambda p: p.set_variant(1), "radix16-w8"),
    "p2-w16": (C1, lambda p: p.set_variant(2), "radix16-w16"),
    "p3-wpf1024": (C1K, None, "radix16-wpf"),
    "p3-wpf2048": (C2K, None, "radix16-wpf"),
    "p4-w16s": (C1, None, "radix16-w16s"),
    "p5-m12": (C1, lambda p: p.set_variant(5), "radix16-m12"),
    "p6-reg2-400": (ANY400, None, "any-length"),
    "p6-stockham-360": (ANY360, None, "any-length"),
    "p6-bluestein-502": (ANY502, None, "any-length"),
    "p4-dct-apart": (C1, lambda p: p.set_fuse_dct(False), "radix16-w16s"),
    "refdefault": (REF_DEFAULT, None, "radix16-w16s"),
    "refdefault-tail2": (REF_DEFAULT, lambda p: p.set_fuse_tail(2), "radix16-w16s"),
    "p4-tail-apart": (C1, lambda p: p.set_fuse_tail(False), "radix16-w16s"),
    # forms behind the seven paths: the 32-frame direct-load kernel, the one-frame-per-wave and the batched form of an
    # any-length plan (launch_any), n_fft 256 embedded in the 512-point tile kernel
    "p7-h32": (C1, lambda p: p.set_variant("h32"), "radix16-h32"),
    "p6-400-form1": (ANY400, lambda p: p.set_variant(1), "any-length"),
    "p6-400-form2": (ANY400, lambda p: p.set_variant(2), "any-length"),
    "p4-embedded-256": (EMB256, None, "radix16-w16s"),
}


def _make_plan(env, which):
    from modulation_mfcc_amd import MfccConfig, MfccPlan
    cfg, tweak, path = PLANS[which]

    def make():
        p = MfccPlan(MfccConfig(**cfg), device=env.gpu)
        if tweak:
            tweak(p)
        assert p.kernel_path == path, (which, p.kernel_path)
        return p
    return env.plan(make), cfg


def _frames(cfg, n):
    return 1 + (n + 2 * (cfg["n_fft"] // 2) - cfg["n_fft"]) // cfg["hop_length"]


def _mod_len(T):
    return 1 << max(0, (T - 1).bit_length())


def front_case(kind, which, B=4, n=16000, clamp_row=None, suffix="", threads=False, check=None):
    """mm_mfcc_f32 / mm_logmel_f32 / mm_stft_power_f32 / mm_mfcc_modspec_f32 through the MfccPlan method of that name."""
    import torch
    entry = {"mfcc": "mm_mfcc_f32", "logmel": "mm_logmel_f32", "stft_power": "mm_stft_power_f32",
             "mfcc_modspec": "mm_mfcc_modspec_f32"}[kind]
    name = f"{kind}/{which}{suffix}"

    def setup(env):
        plan, cfg = _make_plan(env, which)
        T = _frames(cfg, n)
        if check:
            check(plan, B, n)
        x = env.buf["audio"]
        if kind == "mfcc":
            out = env.out((B, cfg["n_mfcc"], T), torch.float32)
            return lambda: plan.mfcc(x, out=out)
        if kind == "mfcc_modspec":
            out = env.out((B, cfg["n_mfcc"], T), torch.float32)
            mod = env.out((B, cfg["n_mfcc"], _mod_len(T) // 2 + 1), torch.complex64)
            return lambda: plan.mfcc_modspec(x, out=out, out_mod=mod)
        return (lambda: plan.logmel(x)) if kind == "logmel" else (lambda: plan.stft_power(x))
    add(name, entry, "front", lambda: {"audio": audio_sets(name, B, n, clamp_row=clamp_row)}, setup, threads=threads)


for _w in ("p0-generic", "p1-w8", "p2-w16", "p3-wpf1024", "p3-wpf2048", "p4-w16s", "p5-m12", "p6-reg2-400", "p6-stockham-360",
           "p6-bluestein-502", "p4-dct-apart", "refdefault", "refdefault-tail2", "p7-h32", "p6-400-form1", "p6-400-form2",
           "p4-embedded-256"):
    # (the widened clip mode needs a clip per compute unit at the least: s16_clip_mode_ok of csrc/mm_api.hip)
    front_case("mfcc", _w, B=256 if _w == "refdefault-tail2" else 4)
front_case("mfcc", "p4-w16s", clamp_row=1, suffix="+fixup")      # one clip clamps: the fix-up launch has work
for _w in ("p0-generic", "p3-wpf1024", "p4-w16s", "p6-reg2-400"):
    front_case("logmel", _w, threads=_w == "p4-w16s")
    front_case("stft_power", _w, threads=_w == "p4-w16s")


def _is_fused(plan, B, n):
    assert plan.fused_tail(B, n), "mm_plan_fused_tail(): this shape was chosen for the one-launch form"


def _is_apart(plan, B, n):
    assert not plan.fused_tail(B, n)


# one launch: a clip per compute unit at the least (mm_plan_fused_tail), 301 frames -> a 512-point trajectory
front_case("mfcc_modspec", "p4-w16s", B=256, n=48000, suffix="+one-launch", check=_is_fused)
front_case("mfcc_modspec", "p4-tail-apart", B=4, n=48000, suffix="", check=_is_apart)


def front_ctypes_case(kind, which, B=4, n=16000):
    """The three entries whose MfccPlan method uses the workspace the plan OBJECT owns ("one plan = one stream at a time"):
    through ctypes with a workspace per instance, so that two threads can share the mm_plan as the header allows."""
    import torch
    entry = {"mfcc": "mm_mfcc_f32", "mfcc_modspec": "mm_mfcc_modspec_f32", "mfcc_ragged": "mm_mfcc_ragged_f32"}[kind]
    name = f"{kind}/{which}+own-workspace"

    def data():
        d = {"audio": audio_sets(name, B, n)}
        if kind == "mfcc_ragged":
            d["lengths"] = length_sets(B, n, 1)
        return d

    def setup(env):
        L, lib = _lib()
        plan, cfg = _make_plan(env, which)
        T = _frames(cfg, n)
        x = env.buf["audio"]
        out = env.out((B, cfg["n_mfcc"], T), torch.float32)
        mod = env.out((B, cfg["n_mfcc"], _mod_len(T) // 2 + 1), torch.complex64)
        need = lib.mm_ragged_workspace_bytes if kind == "mfcc_ragged" else lib.mm_workspace_bytes
        ws = env.work(need(plan._h, B, n))
        if kind == "mfcc":
            def call():
                _ok(lib.mm_mfcc_f32(plan._h, x.data_ptr(), B, n, x.stride(0), out.data_ptr(), ws.data_ptr(), ws.numel(), stream()),
                    entry)
                return out
        elif kind == "mfcc_modspec":
            def call():
                _ok(lib.mm_mfcc_modspec_f32(plan._h, x.data_ptr(), B, n, x.stride(0), out.data_ptr(), mod.data_ptr(),
                                            ws.data_ptr(), ws.numel(), stream()), entry)
                return out, mod
        else:
            lens = env.buf["lengths"]

            def call():
                _ok(lib.mm_mfcc_ragged_f32(plan._h, x.data_ptr(), B, n, x.stride(0), lens.data_ptr(), out.data_ptr(),
                                           mod.data_ptr(), ws.data_ptr(), ws.numel(), stream()), entry)
                return out, mod
        return call
    add(name, entry, "front", data, setup, ragged=kind == "mfcc_ragged", threads=True)


for _k in ("mfcc", "mfcc_modspec", "mfcc_ragged"):
    front_ctypes_case(_k, "p4-w16s")


def rfft_case(nfft, L, rows=8):
    import torch
    name = f"rfft/{nfft}-L{L}"

    def setup(env):
        plan, _ = _make_plan(env, "p4-w16s")
        out = env.out((rows, nfft // 2 + 1), torch.complex64)
        return lambda: plan.rfft(env.buf["rows"], nfft, out=out)
    add(name, "mm_rfft_f32", "front", lambda: {"rows": audio_sets(name, rows, L)}, setup, threads=nfft == 512)


for _n, _l in ((512, 512), (2048, 2048), (1024, 1001), (64, 40)):
    rfft_case(_n, _l)


def modspec_case(T, what, B=2):
    """512- and 1024-point trajectories: mm_modspec_f32; more than 8192 frames: MfccPlan.modspec hands the rows to the
    global-memory transform, mm_hilbert_rfft_f32."""
    import torch
    nm = _mod_len(T)
    name = f"modspec/{what}"

    def data():
        a, b = audio_sets(name, B * 13, T)
        return {"mfcc": (20 * a.reshape(B, 13, T), 20 * b.reshape(B, 13, T))}

    def setup(env):
        plan, _ = _make_plan(env, "p4-w16s")
        out = env.out((B, 13, nm // 2 + 1), torch.complex64)
        return lambda: plan.modspec(env.buf["mfcc"], out=out)
    add(name, "mm_modspec_f32" if nm <= 8192 else "mm_hilbert_rfft_f32", "front", data, setup, threads=True)


modspec_case(300, "512-point")
modspec_case(700, "1024-point")
modspec_case(1500, "2048-point")
modspec_case(5000, "8192-point")
modspec_case(9000, "long-16384-point")


def ragged_front_case(which, B=5, n=16000):
    """MfccPlan.mfcc_modspec_ragged (and, for the first plan, MfccPlan.mfcc_ragged) with an int64 device lengths tensor."""
    import torch

    for method in (("mfcc_modspec_ragged", "mfcc_ragged") if which == "p4-w16s" else ("mfcc_modspec_ragged",)):
        name = f"{method}/{which}"

        def setup(env, method=method):
            plan, cfg = _make_plan(env, which)
            T = _frames(cfg, n)
            out = env.out((B, cfg["n_mfcc"], T), torch.float32)
            x, lens = env.buf["audio"], env.buf["lengths"]
            if method == "mfcc_ragged":
                return lambda: plan.mfcc_ragged(x, lens, out=out)
            mod = env.out((B, cfg["n_mfcc"], _mod_len(T) // 2 + 1), torch.complex64)
            return lambda: plan.mfcc_modspec_ragged(x, lens, out=out, out_mod=mod)
        add(name, "mm_mfcc_ragged_f32", "front", lambda name=name: {"audio": audio_sets(name, B, n), "lengths": length_sets(B, n, 1)},
            setup, ragged=True)


ragged_front_case("p4-w16s")
ragged_front_case("p3-wpf1024")


# ---- the MFCC-change tail -------------------------------------------------------------------------------------------------
def _butter(order, wn):
    from modulation_mfcc_amd.plan import butter_sos
    return butter_sos(order, wn)


def _padlen(n_sec):
    return 3 * (2 * n_sec + 1)


def change_case(what, which, B, T, order=6, second=True):
    name = f"mfcc_change/{what}" + ("" if second else "+no-second-filter")

    def data():
        a, b = audio_sets(name, B * 13, T)
        return {"mfcc": (20 * a.reshape(B, 13, T), 20 * b.reshape(B, 13, T))}

    def setup(env):
        plan, _ = _make_plan(env, which)
        sos, sos2 = _butter(order, 0.1), _butter(order, 0.2)
        return lambda: plan.mfcc_change(env.buf["mfcc"], sos, sos2=sos2, out_filter=second)
    add(name, "mm_mfcc_change_f64", "change", data, setup, threads=what == "clip-resident" and second)


for _second in (True, False):
    change_case("clip-resident", "p4-w16s", 3, 300, second=_second)
    change_case("segmented-rows", "p4-w16s", 2, 9000, second=_second)
    change_case("time-major", "p4-tail-apart", 3, 300, second=_second)
change_case("time-major-5-sections", "p4-w16s", 3, 300, order=10)


def change_ragged_case(B=5, T=300):
    name = "mfcc_change_ragged/iir"

    def data():
        a, b = audio_sets(name, B * 13, T)
        return {"mfcc": (20 * a.reshape(B, 13, T), 20 * b.reshape(B, 13, T)), "frames": length_sets(B, T, _padlen(3) + 1)}

    def setup(env):
        plan, _ = _make_plan(env, "p4-w16s")
        s1, s2 = _butter(6, 0.1), _butter(6, 0.2)
        return lambda: plan.mfcc_change_ragged(env.buf["mfcc"], env.buf["frames"], s1, sos2=s2, out_filter=True)
    add(name, "mm_mfcc_change_ragged_f64", "change", data, setup, ragged=True, threads=True)


change_ragged_case()


# ---- applyFilter's filters, get_velocity's stencils -----------------------------------------------------------------------
def sos_case(what, rows, n, order, f32=False, ragged=False):
    import torch
    dt = np.float32 if f32 else np.float64
    entry = "mm_sosfiltfilt" + ("_ragged" if ragged else "") + ("_f32_f64" if f32 else "_f64")
    name = f"{entry[3:]}/{what}"
    n_sec = (order + 1) // 2

    def data():
        d = {"x": curve_sets(name, rows, n, dt)}
        if ragged:
            d["lengths"] = length_sets(rows, n, _padlen(n_sec) + 1)
        return d

    def setup(env):
        from modulation_mfcc_amd import filters
        sos = _butter(order, 0.08)
        if ragged:
            return lambda: filters.sosfiltfilt_ragged_batch(env.buf["x"], env.buf["lengths"], sos)
        return lambda: filters.sosfiltfilt_batch(env.buf["x"], sos)
    add(name, entry, "filters", data, setup, ragged=ragged)


for _f32 in (False, True):
    sos_case("wave-per-segment", 4, 1100, 6, _f32)              # 1100 + 2 x 21 extended samples: two segments of 1088
    sos_case("workgroup-per-row", 128, 1100, 6, _f32)
    sos_case("time-major-5-sections", 4, 1100, 10, _f32)
    sos_case("wave-per-segment", 4, 1100, 6, _f32, ragged=True)
    sos_case("workgroup-per-row", 128, 1100, 6, _f32, ragged=True)

_FIR_TAPS = np.hanning(33)[1:-1] / np.hanning(33)[1:-1].sum()     # 31 taps


def long_case(kind, ragged, f32=False, rows=4, n=2500):
    """mm_stencil_f64 (np.gradient), mm_fir_filtfilt_* (31 taps) and mm_savgol_f64 (window 21: interior and edge kernel) on
    rows of an ODD pitch (the unvectorised loads); n = 2500 is a second tile of 2048 outputs."""
    dt = np.float32 if f32 else np.float64
    entry = {"stencil": "mm_stencil", "fir": "mm_fir_filtfilt", "savgol": "mm_savgol"}[kind] + ("_ragged" if ragged else "") + \
        ("_f32_f64" if f32 else "_f64")
    name = f"{entry[3:]}/odd-pitch"
    least = {"stencil": 2, "fir": 3 * len(_FIR_TAPS) + 1, "savgol": 21}[kind]

    def data():
        d = {"x": curve_sets(name, rows, n, dt, pitch=n + 1)}
        if ragged:
            d["lengths"] = length_sets(rows, n, least)
        return d

    def setup(env):
        from modulation_mfcc_amd import calc, filters
        x = env.buf["x"][:, :n]
        assert x.stride(0) == n + 1
        if kind == "stencil":
            st, passes = calc.velocity_stencil(100.0, 1, "gradient")
            assert passes == 1
            if ragged:
                return lambda: calc.apply_stencil_ragged(x, env.buf["lengths"], st)
            return lambda: calc.apply_stencil(x, st, 1)
        if kind == "fir":
            if ragged:
                return lambda: filters.fir_filtfilt_ragged_batch(x, env.buf["lengths"], _FIR_TAPS)
            return lambda: filters.fir_filtfilt_batch(x, _FIR_TAPS)
        if ragged:
            return lambda: filters.savgol_ragged_batch(x, env.buf["lengths"], 21, 3)
        return lambda: filters.savgol_batch(x, 21, 3)
    add(name, entry, "filters", data, setup, ragged=ragged)


for _r in (False, True):
    long_case("stencil", _r)
    long_case("fir", _r)
    long_case("fir", _r, f32=True)
    long_case("savgol", _r)


# ---- envelopes --------------------------------------------------------------------------------------------------------------
def rms_case(what, frame, hop, ragged, B=3, n=40000):
    entry = "mm_rms_ragged_f32" if ragged else "mm_rms_f32"
    name = f"{entry[3:]}/{what}"

    def data():
        d = {"audio": audio_sets(name, B, n)}
        if ragged:
            d["lengths"] = length_sets(B, n, 1)
        return d

    def setup(env):
        from modulation_mfcc_amd import batch
        if ragged:
            return lambda: batch.rms_ragged_batch(env.buf["audio"], env.buf["lengths"], frame, hop)
        return lambda: batch.rms_batch(env.buf["audio"], frame, hop)
    add(name, entry, "envelope", data, setup, ragged=ragged)


for _r in (False, True):
    rms_case("tile-kernel", 1600, 160, _r)
    rms_case("frames-kernel", 16385, 4000, _r)


def hilbert_case(what, n, f64, rows, direct):
    import torch
    name = f"hilbert_envelope/{what}-{'f64' if f64 else 'f32'}-{rows}row" + ("s" if rows > 1 else "")

    def setup(env):
        from modulation_mfcc_amd import calc
        L, lib = _lib()
        h = calc._hilbert_plan(n, 1 if f64 else 0, env.gpu)
        assert (lib.mm_hilbert_fft_size(h.h) == n) == direct
        env.keep.append(h)
        return lambda: calc.hilbert_envelope_batch(env.buf["x"])
    add(name, "mm_hilbert_envelope", "envelope", lambda: {"x": audio_sets(name, rows, n, np.float64 if f64 else np.float32)}, setup,
        threads=what == "direct-1000" and not f64)


hilbert_case("direct-1000", 1000, False, 5, True)                  # 2^3 5^3: single passes
hilbert_case("direct-1000", 1000, True, 1, True)
hilbert_case("fused-pairs-160000", 160000, False, 1, True)         # 2^8 5^4: a radix-256 and a radix-625 pair
hilbert_case("fused-pairs-160000", 160000, True, 5, True)
hilbert_case("bluestein-1009", 1009, False, 1, False)
hilbert_case("bluestein-1009", 1009, True, 5, False)


def hilbert_ragged_case(f64, B=5, n=1500):
    name = f"hilbert_envelope_ragged/{'f64' if f64 else 'f32'}"

    def setup(env):
        from modulation_mfcc_amd import calc
        return lambda: calc.hilbert_envelope_ragged_batch(env.buf["x"], env.buf["lengths"])
    add(name, "mm_hilbert_envelope_ragged", "envelope",
        lambda: {"x": audio_sets(name, B, n, np.float64 if f64 else np.float32), "lengths": length_sets(B, n, 1)}, setup,
        ragged=True, threads=not f64)


hilbert_ragged_case(False)
hilbert_ragged_case(True)


def hilbert_rfft_case(rows=3, T=9000, nfft=16384):
    import torch
    name = "hilbert_rfft/16384"

    def setup(env):
        from modulation_mfcc_amd import calc
        out = env.out((rows, nfft // 2 + 1), torch.complex64)
        return lambda: calc.rfft_rows_long(env.buf["x"], nfft, out=out)
    add(name, "mm_hilbert_rfft_f32", "envelope", lambda: {"x": audio_sets(name, rows, T)}, setup, threads=True)


hilbert_rfft_case()


# ---- the input side -----------------------------------------------------------------------------------------------------------
_BPS = {1: 1, 2: 2, 3: 3, 4: 4, 5: 4, 6: 8}


def _pcm_bytes(name, k, fmt, channels, n):
    r = _seed(name, k)
    if fmt == 5:
        return r.uniform(-1, 1, size=n * channels).astype("<f4").view(np.uint8)
    return r.integers(0, 256, size=n * channels * _BPS[fmt], dtype=np.uint8)


def pcm_case(what, fmt, channels, n=4001):
    """ctypes: the package's caller, audio_io.load_wav, works on a path."""
    import torch
    name = f"pcm_decode/{what}"
    stride = n + 4 - n % 4

    def setup(env):
        L, lib = _lib()
        raw = env.buf["raw"]
        out = env.out((channels, stride), torch.float32)       # (the pad columns keep the poison in every run)

        def call():
            _ok(lib.mm_pcm_decode_f32(raw.data_ptr(), fmt, channels, n, out.data_ptr(), stride, stream()), "mm_pcm_decode_f32")
            return out
        return call
    add(name, "mm_pcm_decode_f32", "input", lambda: {"raw": tuple(_pcm_bytes(name, k, fmt, channels, n) for k in (0, 1))}, setup)


pcm_case("s16-mono", 2, 1)
pcm_case("s16-stereo", 2, 2)
pcm_case("f32-mono", 5, 1)
pcm_case("s24-3-channels", 3, 3)

_WAV_FILES = [(2, 1, 3000), (2, 2, 1), (5, 1, 2047), (3, 3, 1500), (1, 2, 999)]       # (fmt, channels, frames) of set 1


def _wav_plan():
    from modulation_mfcc_amd.audio_io import plan_wav_batch
    return plan_wav_batch([dict(fmt=f, channels=c, n_frames=n) for f, c, n in _WAV_FILES])


def pcm_ragged_case():
    """audio_io.decode_wav_batch: the one launch behind load_wav_batch.  The record table is the lengths tensor of this
    entry: set 0 keeps every file's place in the raw buffer and cuts its frame count."""
    name = "pcm_decode_ragged/five-files"

    def data():
        pl = _wav_plan()
        t1 = pl["table"].copy()
        t0 = t1.copy()
        t0["n_frames"] = np.maximum(1, t1["n_frames"] // 2 + np.arange(len(t1)))
        t0["n_frames"][1] = 1
        t0["n_frames"][0] = 2999
        raws = tuple(_seed(name, k).integers(0, 256, size=pl["total_bytes"], dtype=np.uint8) for k in (0, 1))
        for k in (0, 1):                                          # the float32 file: finite values
            o = int(pl["offsets"][2])
            raws[k][o:o + 4 * 2047] = _seed(name, 7 + k).uniform(-1, 1, 2047).astype("<f4").view(np.uint8)
        return {"raw": raws, "recs": (t0.view(np.uint8).copy(), t1.view(np.uint8).copy())}

    def setup(env):
        from modulation_mfcc_amd import audio_io
        pl = _wav_plan()
        return lambda: audio_io.decode_wav_batch(env.buf["raw"], env.buf["recs"], pl)
    add(name, "mm_pcm_decode_ragged_f32", "input", data, setup, ragged=True)


pcm_ragged_case()

# one rate pair per launch shape mm_resample_banded_shape reports: (periods per tile / 16, pad)
RATE_PAIRS = {(16000, 8000): (8, 1), (10000, 8000): (8, 0), (48000, 44100): (4, 1), (44100, 16000): (2, 0), (16000, 22050): (2, 1)}


def resample_case(sr_in, sr_out, method, ragged, rows=3, n=16000):
    banded = method == "mfma"
    entry = "mm_resample" + ("_banded" if banded else "") + ("_ragged" if ragged else "") + "_f32"
    name = f"{entry[3:]}/{sr_in}-{sr_out}"

    def data():
        d = {"x": audio_sets(name, rows, n)}
        if ragged:
            d["lengths"] = length_sets(rows, n, 1)
        return d

    def setup(env):
        from modulation_mfcc_amd import audio_io
        L, lib = _lib()
        if banded:
            a, b = audio_io.resample_ratio(sr_in, sr_out)
            tb = audio_io._device_banded(a, b, env.gpu)
            qt, pad, lds = C.c_int32(), C.c_int32(), C.c_size_t()
            _ok(lib.mm_resample_banded_shape(tb["F"], tb["S"], tb["NB"], tb["ksteps"], tb["win"], C.byref(qt), C.byref(pad),
                                             C.byref(lds)), "mm_resample_banded_shape")
            assert (qt.value, pad.value) == RATE_PAIRS[(sr_in, sr_out)]
        if ragged:
            return lambda: audio_io.resample_ragged_batch(env.buf["x"], env.buf["lengths"], sr_in, sr_out, method=method)
        return lambda: audio_io.resample_batch(env.buf["x"], sr_in, sr_out, method=method)
    add(name, entry, "input", data, setup, ragged=ragged)


for (_a, _b) in RATE_PAIRS:
    resample_case(_a, _b, "mfma", False)
for _r in (False, True):
    resample_case(44100, 16000, "f64", _r)
    resample_case(16000, 8000, "f64", _r)
resample_case(16000, 8000, "mfma", True)
resample_case(44100, 16000, "mfma", True)


def devcopy_case(n=1 << 16):
    import torch

    def setup(env):
        L, lib = _lib()
        src = env.buf["src"]
        dst = env.out((n,), torch.float32)

        def call():
            _ok(lib.mm_devcopy_f32(src.data_ptr(), dst.data_ptr(), n, stream()), "mm_devcopy_f32")
            return dst
        return call
    add("devcopy/65536", "mm_devcopy_f32", "input", lambda: {"src": tuple(a[0] for a in audio_sets("devcopy", 1, n))}, setup)


devcopy_case()


# ---- pYIN -----------------------------------------------------------------------------------------------------------------------
PYIN_KW = dict(fmin=100, fmax=500, frame_length=512, hop_length=128)
PYIN_SR = 8000


def _voiced_sets(name, B, n, dtype):
    out = []
    for k in (0, 1):
        r = _seed(name, k)
        t = np.arange(n) / PYIN_SR
        f = r.uniform(120, 400, size=(B, 1))
        x = 0.5 * np.sin(2 * np.pi * f * t[None, :]) * (t[None, :] > 0.2 * (k + 1)) + 0.01 * r.standard_normal((B, n))
        out.append(x.astype(dtype))
    return tuple(out)


def pyin_case(f64, ragged, B=3, n=8000):
    entry = "mm_pyin" + ("_ragged" if ragged else "") + ("_f64" if f64 else "_f32")
    name = f"{entry[3:]}/whole-path"

    def data():
        d = {"x": _voiced_sets(name, B, n, np.float64 if f64 else np.float32)}
        if ragged:
            d["lengths"] = length_sets(B, n, 1)
        return d

    def setup(env):
        from modulation_mfcc_amd import pitch
        if ragged:
            return lambda: pitch.pyin_ragged_batch(env.buf["x"], env.buf["lengths"], PYIN_SR, return_states=True, **PYIN_KW)
        return lambda: pitch.pyin_batch(env.buf["x"], PYIN_SR, return_states=True, **PYIN_KW)
    add(name, entry, "pyin", data, setup, ragged=ragged, threads=not f64 and not ragged)


for _f in (False, True):
    for _r in (False, True):
        pyin_case(_f, _r)


def pyin_cmnd_case(f64, B=3, n=8000):
    name = f"pyin_cmnd/{'f64' if f64 else 'f32'}"

    def setup(env):
        from modulation_mfcc_amd import pitch
        return lambda: pitch.pyin_cmnd(env.buf["x"], PYIN_SR, **PYIN_KW)
    add(name, "mm_pyin_cmnd", "pyin", lambda: {"x": _voiced_sets(name, B, n, np.float64 if f64 else np.float32)}, setup)


pyin_cmnd_case(False)
pyin_cmnd_case(True)


def _pyin_p():
    from modulation_mfcc_amd import pitch
    return pitch.pyin_params(PYIN_KW["frame_length"], PYIN_SR, **PYIN_KW)


def pyin_candidates_case(T=70):
    """pitch.pyin_records on CMND rows made on the host: a dip per frame at a wandering lag, on noise."""
    name = "pyin_candidates/records"

    def data():
        P = math.ceil(PYIN_SR / PYIN_KW["fmin"]) - PYIN_SR // PYIN_KW["fmax"] + 1       # max_period - min_period + 1
        out = []
        for k in (0, 1):
            r = _seed(name, k)
            c = 1.0 + 0.3 * r.standard_normal((T, P))
            lag = r.integers(5, P - 5, size=T)
            c[np.arange(T), lag] = r.uniform(0.01, 0.3, size=T)
            out.append(np.abs(c))
        return {"cmnd": tuple(out)}

    def setup(env):
        from modulation_mfcc_amd import pitch
        p, z = _pyin_p()
        assert env.buf["cmnd"].shape[1] == z["max_period"] - z["min_period"] + 1
        return lambda: pitch.pyin_records(env.buf["cmnd"], PYIN_SR, **PYIN_KW)
    add(name, "mm_pyin_candidates", "pyin", data, setup)


pyin_candidates_case()


def pyin_decode_case(B=3, T=40, K=3):
    """ctypes (the package reaches the decode only inside the whole path): random records, as tests/test_gpu_pitch_params.py
    makes them."""
    import torch
    name = "pyin_decode/records"

    def data():
        nb = 12 * 10 * math.log2(PYIN_KW["fmax"] / PYIN_KW["fmin"])
        nb = int(math.floor(nb)) + 1
        R = (math.ceil(PYIN_SR / PYIN_KW["fmin"]) - PYIN_SR // PYIN_KW["fmax"] + 2) // 2 + 1
        sets = {"count": [], "bins": [], "probs": [], "vp": []}
        for k in (0, 1):
            r = _seed(name, k)
            count = r.integers(1, K + 1, size=(B * T,)).astype(np.int32)
            bins = np.zeros((B * T, R), np.int32)
            probs = np.zeros((B * T, R))
            for i in range(B * T):
                c = int(count[i])
                bins[i, :c] = np.sort(r.choice(nb, size=c, replace=False))[::-1]
                probs[i, :c] = r.dirichlet(np.ones(c)) * r.random()
            sets["count"].append(count), sets["bins"].append(bins), sets["probs"].append(probs)
            sets["vp"].append(np.clip(probs.sum(axis=1), 0, 1))
        return {k: tuple(v) for k, v in sets.items()}

    def setup(env):
        from modulation_mfcc_amd import pitch
        L, lib = _lib()
        p, z = _pyin_p()
        tabs = pitch._tables(p, z, 0.01, (2, 18), 2, env.gpu)
        p.band_h = tabs.H
        env.keep.append(tabs)
        assert env.buf["bins"].shape[1] == p.max_troughs and int(env.staged[1]["bins"].max()) < z["n_bins"]
        states, f0 = env.out((B, T), torch.int32), env.out((B, T), torch.float64)
        voiced = env.out((B, T), torch.uint8)
        ws = env.work(lib.mm_pyin_decode_workspace_bytes(C.byref(p), B, T))
        b = env.buf

        def call():
            _ok(lib.mm_pyin_decode(C.byref(p), C.byref(tabs.c), b["count"].data_ptr(), b["bins"].data_ptr(), b["probs"].data_ptr(),
                                   b["vp"].data_ptr(), B, T, states.data_ptr(), f0.data_ptr(), voiced.data_ptr(), ws.data_ptr(),
                                   ws.numel(), stream()), "mm_pyin_decode")
            return states, f0, voiced
        return call
    add(name, "mm_pyin_decode", "pyin", data, setup)


pyin_decode_case()


# ---- interp_NAN and the regrid ------------------------------------------------------------------------------------------------
INTERP_KINDS = ("pchip", "nearest", "nearest-up", "previous", "next", "zero", "slinear")


def _gap_sets(name, rows, n):
    out = []
    for k in (0, 1):
        r = _seed(name, k)
        x = np.cumsum(r.standard_normal((rows, n)), axis=1)
        x[r.random((rows, n)) < 0.3] = np.nan
        x[:, 0] = np.nan                     # a gap before the first and behind the last valid sample
        x[:, n - 3:] = np.nan
        x[:, 1:3] = 1.0 + k                  # two valid samples below the smallest count
        out.append(x)
    return tuple(out)


def interp_case(kind, ragged, rows=4, n=2500):
    """ctypes: interp_nan_batch / interp_nan_ragged_batch read the smallest number of valid samples back, by design (the
    reference's errors); n = 2500 is three segments of 1024 samples."""
    import torch
    lin = kind == "linear"
    entry = "mm_interp_nan" + ("_linear" if lin else "") + ("_ragged" if ragged else "") + "_f64"
    name = f"{entry[3:]}/{kind}"

    def data():
        d = {"x": _gap_sets(name, rows, n)}
        if ragged:
            d["counts"] = length_sets(rows, n, 3)
        return d

    def setup(env):
        from modulation_mfcc_amd import interp
        L, lib = _lib()
        x = env.buf["x"]
        y = env.out((rows, n), torch.float64)
        code = 0 if lin else interp._INTERP_KINDS[kind]
        ws = env.work(lib.mm_interp_nan_workspace_bytes(code, rows, n))
        cnt = env.buf.get("counts")

        def call():
            if lin and ragged:
                rc = lib.mm_interp_nan_linear_ragged_f64(x.data_ptr(), rows, n, n, cnt.data_ptr(), y.data_ptr(), n, stream())
            elif lin:
                rc = lib.mm_interp_nan_linear_f64(x.data_ptr(), rows, n, n, y.data_ptr(), n, stream())
            elif ragged:
                rc = lib.mm_interp_nan_ragged_f64(code, x.data_ptr(), rows, n, n, cnt.data_ptr(), y.data_ptr(), n, ws.data_ptr(),
                                                  ws.numel(), stream())
            else:
                rc = lib.mm_interp_nan_f64(code, x.data_ptr(), rows, n, n, y.data_ptr(), n, ws.data_ptr(), ws.numel(), stream())
            _ok(rc, entry)
            return y
        return call
    add(name, entry, "interp", data, setup, ragged=ragged)


for _r in (False, True):
    for _k in ("linear",) + INTERP_KINDS:
        interp_case(_k, _r)


def interp_wrapper_case(rows=4, n=2500):
    """interp.interp_nan_ragged_batch with an int64 device tensor of counts.  Its documentation announces ONE read-back (the
    smallest number of valid samples below a row's count, for the reference's errors): the call waits for its stream."""
    name = "interp_nan_ragged_batch/pchip"

    def setup(env):
        from modulation_mfcc_amd import interp
        return lambda: interp.interp_nan_ragged_batch(env.buf["x"], env.buf["counts"], "pchip")
    add(name, "mm_interp_nan_ragged_f64", "interp", lambda: {"x": _gap_sets(name, rows, n), "counts": length_sets(rows, n, 3)}, setup,
        ragged=True, host_sync="interp_nan_ragged_batch: 'the errors taken from the smallest number of valid samples below a "
                               "row's count, in one read-back'")


interp_wrapper_case()


def regrid_case(n=700, cols=5, m=450):
    """ctypes: the package's caller, ema.read_AG50x_arrays, works on a path."""
    import torch
    name = "regrid_linear/5-columns"

    def data():
        ys, tin, tout = [], [], []
        for k in (0, 1):
            r = _seed(name, k)
            ys.append(np.cumsum(r.standard_normal((n, cols)), axis=0).astype(np.float32))
            tin.append(np.cumsum(r.uniform(0.004, 0.006, size=n)))
            tout.append(np.linspace(-0.01, tin[-1][-1] + 0.01, m) + 1e-4 * k)
        return {"y": tuple(ys), "t_in": tuple(tin), "t_out": tuple(tout)}

    def setup(env):
        L, lib = _lib()
        b = env.buf
        out = env.out((m, cols), torch.float64)

        def call():
            _ok(lib.mm_regrid_linear_f32_f64(b["y"].data_ptr(), n, cols, cols, b["t_in"].data_ptr(), b["t_out"].data_ptr(), m,
                                             out.data_ptr(), cols, stream()), "mm_regrid_linear_f32_f64")
            return out
        return call
    add(name, "mm_regrid_linear_f32_f64", "interp", data, setup)


regrid_case()


# ---- peaks --------------------------------------------------------------------------------------------------------------------
def peaks_case(what, ex, kw, ranges=False, rows=4, n=2500):
    name = f"find_peaks{'_ex' if ex else ''}/{what}"

    def data():
        a, b = curve_sets(name, rows, n)
        for x in (a, b):
            x[:, 100:104] = 3.0              # a plateau
        d = {"x": (a, b)}
        if ranges:
            r = np.arange(rows)
            d["lo"] = ((r * 7).astype(np.int32), (r * 11 + 3).astype(np.int32))
            d["hi"] = ((n - r * 5).astype(np.int32), (n - 40 - r * 13).astype(np.int32))
        return d

    def setup(env):
        from modulation_mfcc_amd import calc
        fn = calc.find_peaks_ex_batch if ex else calc.find_peaks_batch
        extra = dict(lo=env.buf["lo"], hi=env.buf["hi"]) if ranges else {}
        return lambda: fn(env.buf["x"], **kw, **extra)
    add(name, "mm_find_peaks_ex" if ex else "mm_find_peaks", "peaks", data, setup)


peaks_case("plain", False, {})
peaks_case("prominence", False, dict(prominence=0.5))
peaks_case("sub-ranges", False, dict(prominence=0.5, negate=True), ranges=True)
peaks_case("distance", True, dict(distance=7))
peaks_case("wlen+width", True, dict(width=2, wlen=60))
peaks_case("plateau_size", True, dict(plateau_size=(1, 6)))


FAMILIES = sorted({c.family for c in CASES})
BY_NAME = {c.name: c for c in CASES}
