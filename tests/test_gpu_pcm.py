"""GPU (-m gpu): the WAVE decode of load_audio, mm_pcm_decode_f32, value by value -- every kernel it can launch
(pcm_decode_s16_kernel<1|2>, pcm_decode_f32_kernel<1|2>: 16 / 32 bytes per thread, 16-byte stores per channel;
pcm_decode_kernel: byte-wise, all six formats, any channel count) driven directly with uint8 device buffers.

The expectation is computed in NumPy from the same bytes: explicit little-endian dtypes, a 24-bit value assembled from
three bytes and sign-extended, (u8 - 128) / 128, s16 / 32768, s24 / 2^23, float32(float64(s32) / 2^31), float32 bits
unchanged, float64.astype(float32).  Every comparison is equality of the uint32 bit patterns: NaN payloads and -0.0
count.  No tolerance anywhere in this file.

Which kernel a call reaches follows from the dispatch (csrc/mm_side.hip, mm_pcm_decode_f32): the vector kernels take
s16 / f32 with one or two channels when d_raw and d_out are 16-byte aligned and, for two channels, out_stride is a
multiple of 4 -- n_frames / (8 / channels) whole vectors; the byte-wise kernel takes the remaining frames and every
other call.  Each case below names the kernel it reaches.  Every output lies in a buffer of NaN sentinels with
out_stride > n_frames: what is between and behind the rows must survive.

MEASURED (MI355X).  Wall time of the file: 3.2 s for its 25 cases (1.6 s of it device set-up; the two 16 MiB streams
0.07 s each, every other case under 0.2 s).  The device's float64 -> float32 conversion equals NumPy's on every value
here, the subnormal results included: nothing is pinned apart.
"""
import ctypes as C
import struct

import numpy as np
import pytest

from modulation_mfcc_amd import _lib

pytestmark = pytest.mark.gpu

U8, S16, S24, S32, F32, F64 = 1, 2, 3, 4, 5, 6
BPS = {U8: 1, S16: 2, S24: 3, S32: 4, F32: 4, F64: 8}
TAIL = 16                        # sentinel floats behind the last row


def np_decode(raw, fmt, channels):
    """Interleaved little-endian frames (uint8 array) -> the float32 bit patterns [channels, n_frames] (uint32)."""
    raw = np.ascontiguousarray(raw, dtype=np.uint8)
    if fmt == U8:
        v = ((raw.astype(np.float32) - np.float32(128.0)) / np.float32(128.0)).astype(np.float32)
    elif fmt == S16:
        v = (raw.view("<i2").astype(np.float32) / np.float32(32768.0)).astype(np.float32)
    elif fmt == S24:
        b = raw.reshape(-1, 3).astype(np.int64)
        q = b[:, 0] | (b[:, 1] << 8) | (b[:, 2] << 16)
        q = np.where(q >= 1 << 23, q - (1 << 24), q)                       # sign extension
        v = (q.astype(np.float32) / np.float32(8388608.0)).astype(np.float32)        # |q| <= 2^23: exact in float32
    elif fmt == S32:
        v = (raw.view("<i4").astype(np.float64) / 2147483648.0).astype(np.float32)
    elif fmt == F32:
        return np.ascontiguousarray(raw.view("<u4").reshape(-1, channels).T)
    else:
        with np.errstate(over="ignore", under="ignore"):
            v = raw.view("<f8").astype(np.float32)
    return np.ascontiguousarray(v.reshape(-1, channels).T).view(np.uint32)


def dev_decode(raw, fmt, channels, gpu, out_stride=None, raw_off=0, out_off=0):
    """mm_pcm_decode_f32 on the bytes `raw` -> uint32 [channels, n_frames].  d_raw = a 16-byte aligned buffer + raw_off
    bytes, d_out = a 16-byte aligned buffer + out_off floats, rows out_stride apart; everything outside the rows is a
    NaN sentinel (its position in the payload) and is checked."""
    import torch
    raw = np.ascontiguousarray(raw, dtype=np.uint8)
    n = raw.size // (BPS[fmt] * channels)
    assert n * BPS[fmt] * channels == raw.size and n >= 1
    stride = n + 4 - n % 4 if out_stride is None else out_stride          # default: a multiple of 4, > n
    assert stride > n
    d_raw = torch.full((raw_off + raw.size + 32,), 0xA5, dtype=torch.uint8, device=gpu)
    d_raw[raw_off:raw_off + raw.size] = torch.from_numpy(raw.copy()).to(gpu)
    total = out_off + channels * stride + TAIL
    sent = np.uint32(0x7FC00000) | (np.arange(total, dtype=np.uint32) & np.uint32(0xFFFFF))
    d_out = torch.from_numpy(sent.view(np.float32).copy()).to(gpu)
    assert d_raw.data_ptr() % 16 == 0 and d_out.data_ptr() % 16 == 0
    lib = _lib.load()
    with torch.cuda.device(gpu):
        rc = lib.mm_pcm_decode_f32(d_raw.data_ptr() + raw_off, fmt, channels, n, d_out.data_ptr() + 4 * out_off, stride,
                                   C.c_void_p(torch.cuda.current_stream(gpu).cuda_stream))
    assert rc == _lib.MM_OK
    got = d_out.cpu().numpy().view(np.uint32)
    rows = got[out_off:out_off + channels * stride].reshape(channels, stride)
    keep = np.ones(total, dtype=bool)
    for c in range(channels):
        keep[out_off + c * stride:out_off + c * stride + n] = False
    np.testing.assert_array_equal(got[keep], sent[keep], err_msg="sentinels before, between or behind the rows")
    return rows[:, :n].copy()


def check(raw, fmt, channels, gpu, **kw):
    got = dev_decode(raw, fmt, channels, gpu, **kw)
    want = np_decode(raw, fmt, channels)
    bad = np.argwhere(got != want)
    assert bad.shape[0] == 0, (fmt, channels, kw, bad.shape[0], bad[:6], [hex(v) for v in got[tuple(bad[:6].T)]],
                               [hex(v) for v in want[tuple(bad[:6].T)]])
    return got


def interleave(chans):
    """Per-channel sample arrays (same dtype, same length) -> the interleaved byte stream."""
    a = np.stack(chans, axis=1)
    return np.ascontiguousarray(a).view(np.uint8).reshape(-1)


def s24_bytes(q):
    q = np.asarray(q, dtype=np.int64) & 0xFFFFFF
    return np.stack([q & 0xFF, (q >> 8) & 0xFF, (q >> 16) & 0xFF], axis=-1).astype(np.uint8)


# ---- values -------------------------------------------------------------------------------------------------------
def test_every_8_bit_code(gpu):
    codes = np.arange(256, dtype=np.uint8)
    got = check(codes, U8, 1, gpu)                                         # pcm_decode_kernel, fmt 1
    assert got.view(np.float32)[0, 0] == -1.0 and got.view(np.float32)[0, 255] == 127.0 / 128.0
    check(interleave([codes, codes[::-1]]), U8, 2, gpu)                    # pcm_decode_kernel, two channels


def test_every_16_bit_code(gpu):
    codes = np.arange(65536, dtype=np.uint32).astype("<u2")
    mixed = ((np.arange(65536, dtype=np.uint32) * 40503) & 0xFFFF).astype("<u2")      # 40503 is odd: a permutation
    assert np.unique(mixed).size == 65536
    a = check(codes.view(np.uint8), S16, 1, gpu)                           # pcm_decode_s16_kernel<1>: 8192 vectors
    f = a.view(np.float32)[0]
    assert f[0x8000] == -1.0 and f[0x7FFF] == 32767.0 / 32768.0 and f[0xFFFF] == -1.0 / 32768.0 and f[0] == 0.0
    b = check(codes.view(np.uint8), S16, 1, gpu, raw_off=2)                # pcm_decode_kernel, fmt 2 (d_raw unaligned)
    np.testing.assert_array_equal(a, b)
    st = interleave([codes, mixed])
    v = check(st, S16, 2, gpu, out_stride=65536 + 4)                       # pcm_decode_s16_kernel<2>: 16384 vectors
    w = check(st, S16, 2, gpu, out_stride=65536 + 5)                       # pcm_decode_kernel (pitch no multiple of 4)
    np.testing.assert_array_equal(v, w)
    np.testing.assert_array_equal(v[0], a[0])


def _int_edges(bits):
    top = 1 << (bits - 1)
    return [top - 1, -top, -1, 1, 0, top - 1 - 64, -top + 1, top - 2, top >> 1, -(top >> 1), (top >> 1) + 1, top - 64]


def test_24_and_32_bit_range_ends_and_random_codes(gpu):
    rng = np.random.default_rng(21)
    q24 = np.array(_int_edges(24) + list(rng.integers(-(1 << 23), 1 << 23, 4096)), dtype=np.int64)
    raw24 = s24_bytes(q24).reshape(-1)
    assert tuple(raw24[:9]) == (0xFF, 0xFF, 0x7F, 0x00, 0x00, 0x80, 0xFF, 0xFF, 0xFF)        # 0x7FFFFF, 0x800000, 0xFFFFFF
    g = check(raw24, S24, 1, gpu).view(np.float32)[0]                      # pcm_decode_kernel, fmt 3
    assert g[0] == 8388607.0 / 8388608.0 and g[1] == -1.0 and g[2] == -1.0 / 8388608.0
    q32 = np.array(_int_edges(32) + list(rng.integers(-(1 << 31), 1 << 31, 4096)), dtype=np.int64).astype("<i4")
    g = check(q32.view(np.uint8), S32, 1, gpu).view(np.float32)[0]         # pcm_decode_kernel, fmt 4
    # INT32_MAX / 2^31 = 1 - 2^-31 rounds to exactly 1.0 in float32; INT32_MAX - 63 is the tie 1 - 2^-25 (to even: 1.0),
    # INT32_MAX - 64 the first code below it (1 - 2^-24); INT32_MIN is -1.0
    assert g[0] == 1.0 and g[1] == -1.0 and g[11] == 1.0 and g[5] == np.float32(1.0 - 2.0 ** -24)
    assert g[2] == np.float32(-(2.0 ** -31)) and g[4] == 0.0


def _f32_patterns(rng, n):
    special = np.array([0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00001, 0x7F800001, 0x7FBFFFFF,
                        0xFFFFFFFF, 0x00000001, 0x807FFFFF, 0x00800000, 0x7F7FFFFF, 0x3F800000], dtype=np.uint32)
    u = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    u[:special.size] = special
    return u.astype("<u4")


def test_float32_bit_patterns_pass_unchanged(gpu):
    """NaN payloads (quiet and signalling), infinities, denormals, -0.0: the decode of float data moves bits."""
    rng = np.random.default_rng(22)
    u = _f32_patterns(rng, 4096)
    a = check(u.view(np.uint8), F32, 1, gpu)                               # pcm_decode_f32_kernel<1>
    np.testing.assert_array_equal(a[0], u)
    b = check(u.view(np.uint8), F32, 1, gpu, out_off=1)                    # pcm_decode_kernel, fmt 5 (d_out unaligned)
    np.testing.assert_array_equal(a, b)
    st = interleave([u, u[::-1].copy()])
    v = check(st, F32, 2, gpu, out_stride=4096 + 8)                        # pcm_decode_f32_kernel<2>
    w = check(st, F32, 2, gpu, out_stride=4096 + 7)                        # pcm_decode_kernel
    np.testing.assert_array_equal(v, w)


def _f64_normal_results():
    e = 2.0 ** -24                                                         # half a float32 ulp at 1.0
    fmax = float(np.finfo(np.float32).max)
    half_ulp_max = 2.0 ** 103                                              # half a float32 ulp at FLT_MAX
    v = [1.0 + e, 1.0 + 3 * e, 1.0 + e + 2.0 ** -50, 1.0 + e - 2.0 ** -50, 1.0 + 5 * e, 1.0 - e / 2, 1.0 - e / 2 - 2.0 ** -52,
         0.1, 1.0 / 3.0, np.pi, fmax, fmax + half_ulp_max / 2, fmax + half_ulp_max, fmax + 2 * half_ulp_max, 1e39, 1e308,
         float("inf"), 0.0, 2.0 ** -126, 2.0 ** -126 * (1 + 2.0 ** -24), 2.0 ** -126 * (1 + 2.0 ** -23)]
    v = np.array(v + [-t for t in v], dtype=np.float64)
    rng = np.random.default_rng(23)
    r = rng.standard_normal(4096) * 10.0 ** rng.uniform(-37, 37, 4096)
    return np.concatenate([v, r]).astype("<f8")


def _f64_subnormal_results():
    m = 2.0 ** -149                                                        # the smallest float32 subnormal
    v = [2.0 ** -126 * (1 - 2.0 ** -25), 2.0 ** -126 * (1 - 2.0 ** -24), 2.0 ** -127, 2.0 ** -127 + m / 2, 3 * m, 2.5 * m,
         1.5 * m, 1.5 * m * (1 + 2.0 ** -30), m, m / 2, m / 2 * (1 + 2.0 ** -40), m / 2 * (1 - 2.0 ** -40), m / 4, 1e-45, 1e-46,
         1e-60, 1e-300, 5e-324, 1.1754942e-38, 7.3e-42]
    v = np.array(v + [-t for t in v], dtype=np.float64)
    rng = np.random.default_rng(24)
    r = rng.uniform(-1.0, 1.0, 2048) * 2.0 ** rng.uniform(-152, -126, 2048)
    return np.concatenate([v, r]).astype("<f8")


def test_float64_rounds_to_float32_as_ieee(gpu):
    """Ties to even in both directions, just above and below a tie, beyond FLT_MAX (the tie at FLT_MAX + half an ulp goes
    to infinity), the smallest normal number: float64 -> float32 results that are normal, zero or infinite."""
    x = _f64_normal_results()
    want = np_decode(x.view(np.uint8), F64, 1).view(np.float32)[0]
    assert want[0] == 1.0 and want[1] == np.float32(1.0 + 2.0 ** -22) and want[2] == np.float32(1.0 + 2.0 ** -23) and want[3] == 1.0
    assert want[10] == np.finfo(np.float32).max and want[11] == want[10] and np.isinf(want[12]) and np.isinf(want[14])
    check(x.view(np.uint8), F64, 1, gpu)                                   # pcm_decode_kernel, fmt 6
    check(x[:4000].view(np.uint8), F64, 2, gpu)


def test_float64_rounds_into_the_float32_subnormals(gpu):
    """float64 values whose float32 image is subnormal or underflows to zero: rounded to the nearest multiple of 2^-149,
    ties to even, signed zeros kept (what NumPy's conversion gives)."""
    x = _f64_subnormal_results()
    want = np_decode(x.view(np.uint8), F64, 1)[0]
    assert want[8] == 1 and want[9] == 0 and want[10] == 1 and want[11] == 0 and want[4] == 3 and want[5] == 2 and want[6] == 2
    assert want[0] == 0x00800000 and want[1] == 0x00800000 and want[2] == 0x00400000
    check(x.view(np.uint8), F64, 1, gpu)                                   # pcm_decode_kernel, fmt 6


# ---- paths --------------------------------------------------------------------------------------------------------
def _stream_of(fmt, channels, n, rng):
    """n frames whose channels carry different content: full-range 16-bit codes / float32 bit patterns."""
    if fmt == S16:
        chans = [rng.integers(0, 1 << 16, n, dtype=np.uint32).astype("<u2") for _ in range(channels)]
    else:
        chans = [_f32_patterns(rng, max(n, 16))[::-1][:n].copy() for _ in range(channels)]
    return interleave(chans)


@pytest.mark.parametrize("fmt", [S16, F32], ids=["s16", "f32"])
def test_mono_vector_kernels_and_their_remainders(fmt, gpu):
    """A vector is 8 frames: n below one vector (n_vec = 0: the byte-wise kernel alone), exactly one, every remainder
    n % 8 after one and after many vectors -- and the same bytes forced off the vector path give the same values."""
    rng = np.random.default_rng(31)
    sizes = list(range(1, 17)) + [8 * 37 + r for r in range(8)] + [8 * 300]
    assert {n % 8 for n in sizes if n >= 8} == set(range(8)) and 8 in sizes and min(sizes) < 8
    for n in sizes:
        raw = _stream_of(fmt, 1, n, rng)
        a = check(raw, fmt, 1, gpu)                                        # pcm_decode_{s16,f32}_kernel<1> + byte-wise rest
        b = check(raw, fmt, 1, gpu, out_stride=n + 1 + n % 2)              # <1> again: one channel needs no aligned pitch
        np.testing.assert_array_equal(a, b)
        for off in (2, 4, 6):
            c = check(raw, fmt, 1, gpu, raw_off=off)                       # pcm_decode_kernel (d_raw off 16 bytes)
            np.testing.assert_array_equal(a, c)
        d = check(raw, fmt, 1, gpu, out_off=1)                             # pcm_decode_kernel (d_out one float off)
        np.testing.assert_array_equal(a, d)


@pytest.mark.parametrize("fmt", [S16, F32], ids=["s16", "f32"])
def test_stereo_vector_kernels_and_their_remainders(fmt, gpu):
    """A vector is 4 stereo frames.  The pitch decides: a multiple of 4 reaches pcm_decode_{s16,f32}_kernel<2>, any
    other the byte-wise kernel -- same values."""
    rng = np.random.default_rng(32)
    sizes = list(range(1, 9)) + [4 * 61 + r for r in range(4)] + [4 * 500]
    assert {n % 4 for n in sizes if n >= 4} == set(range(4)) and 4 in sizes and min(sizes) < 4
    for n in sizes:
        raw = _stream_of(fmt, 2, n, rng)
        a = check(raw, fmt, 2, gpu)                                        # <2> (pitch n + 4 - n % 4) + byte-wise rest
        b = check(raw, fmt, 2, gpu, out_stride=n + 4 - n % 4 + 4)          # <2>, another pitch
        np.testing.assert_array_equal(a, b)
        for p in (1, 2, 3):
            c = check(raw, fmt, 2, gpu, out_stride=n + 4 - n % 4 + p)      # pcm_decode_kernel (pitch no multiple of 4)
            np.testing.assert_array_equal(a, c)
        for off in (2, 4, 6):
            c = check(raw, fmt, 2, gpu, raw_off=off)                       # pcm_decode_kernel (d_raw off 16 bytes)
            np.testing.assert_array_equal(a, c)
        d = check(raw, fmt, 2, gpu, out_off=1)                             # pcm_decode_kernel (d_out one float off)
        np.testing.assert_array_equal(a, d)


@pytest.mark.parametrize("channels", [3, 6])
@pytest.mark.parametrize("fmt", [U8, S16, S24, S32, F32, F64], ids=["u8", "s16", "s24", "s32", "f32", "f64"])
def test_many_channels_in_every_format(fmt, channels, gpu):
    """pcm_decode_kernel, the only kernel for three channels and more: each channel carries its own content, so a slip
    of the de-interleave (frame / channel index) shows."""
    rng = np.random.default_rng(40 + fmt)
    n = 1001
    if fmt == F64:
        vals = rng.standard_normal((n, channels)) * 10.0 ** rng.uniform(-30, 30, (n, channels))
        raw = np.ascontiguousarray(vals.astype("<f8")).view(np.uint8).reshape(-1)
    elif fmt == F32:
        raw = interleave([_f32_patterns(rng, n)[::-1].copy() for _ in range(channels)])
    else:
        raw = rng.integers(0, 256, n * channels * BPS[fmt], dtype=np.uint8)
    got = check(raw, fmt, channels, gpu, out_stride=n + 6)
    assert len({got[c].tobytes() for c in range(channels)}) == channels


# ---- the grid-stride loop -----------------------------------------------------------------------------------------
GRID_VECTORS = 256 * 16 * 256            # the vector kernels' largest grid, in threads: beyond it a thread loops


def _counter(n_samples):
    return ((np.arange(n_samples, dtype=np.uint64) * 40503) & 0xFFFF).astype("<u2")


def test_mono_stream_longer_than_the_grid(gpu):
    """8.4 M mono samples (190 s at 44.1 kHz) fill the grid of pcm_decode_s16_kernel<1>; three more vectors enter its
    grid-stride loop, five more frames the byte-wise kernel.  Sample i holds (40503 i) mod 65536."""
    n = GRID_VECTORS * 8 + 8 * 3 + 5
    got = check(_counter(n).view(np.uint8), S16, 1, gpu)
    assert got.shape == (1, n)


def test_stereo_stream_longer_than_the_grid(gpu):
    """Half as many stereo frames: pcm_decode_s16_kernel<2> with three vectors in its grid-stride loop, two frames left."""
    n = (GRID_VECTORS * 8 + 8 * 3 + 5) // 2
    assert n // 4 == GRID_VECTORS + 3 and n % 4 == 2
    got = check(_counter(2 * n).view(np.uint8), S16, 2, gpu)
    assert got.shape == (2, n)


# ---- the public entry ---------------------------------------------------------------------------------------------
def _wav(path, raw, sr, channels, bits):
    raw = np.ascontiguousarray(raw, dtype=np.uint8).tobytes()
    fmt = struct.pack("<HHIIHH", 1, channels, sr, sr * channels * bits // 8, channels * bits // 8, bits)
    with open(path, "wb") as f:
        f.write(b"RIFF" + struct.pack("<I", 4 + 8 + len(fmt) + 8 + len(raw)) + b"WAVE")
        f.write(b"fmt " + struct.pack("<I", len(fmt)) + fmt)
        f.write(b"data" + struct.pack("<I", len(raw)) + raw)


def test_load_wav_reaches_the_stereo_vector_kernel(tmp_path, gpu):
    """load_wav decodes into rows n_frames apart: a stereo 16-bit file with a multiple of 4 frames goes through
    pcm_decode_s16_kernel<2>, one frame more through the byte-wise kernel; a 6-channel 24-bit file."""
    from modulation_mfcc_amd import load_wav
    rng = np.random.default_rng(50)
    for n in (4 * 777, 4 * 777 + 1):
        raw = _stream_of(S16, 2, n, rng)
        p = str(tmp_path / f"st{n}.wav")
        _wav(p, raw, 44100, 2, 16)
        got, sr = load_wav(p, gpu)
        assert sr == 44100.0 and tuple(got.shape) == (2, n) and got.is_contiguous()
        np.testing.assert_array_equal(got.cpu().numpy().view(np.uint32), np_decode(raw, S16, 2))
    raw = rng.integers(0, 256, 1500 * 6 * 3, dtype=np.uint8)
    p = str(tmp_path / "six.wav")
    _wav(p, raw, 48000, 6, 24)
    got, sr = load_wav(p, gpu)
    assert sr == 48000.0 and tuple(got.shape) == (6, 1500)
    np.testing.assert_array_equal(got.cpu().numpy().view(np.uint32), np_decode(raw, S24, 6))
