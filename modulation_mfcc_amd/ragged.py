"""The host rules of ragged batches -- a padded batch [rows, n_max] on the device and a count per row -- in one place
(DESIGN.md section 12.0): the counts (validation, the one upload, grouping, frame counts), the rows (the argument check,
the row pitch), scipy's refusals with the row named, and the list layer under the four list front ends.  Every
``*_ragged_batch`` function of the package is built from these.  A leaf module: numpy, torch (imported lazily, as
everywhere in the package) and nothing else of the package.
"""
from __future__ import annotations

import numpy as np


def is_device_tensor(x):
    """A CUDA(HIP) torch tensor, duck-typed: the package's one such test (a CPU tensor is host data)."""
    return type(x).__module__.startswith("torch") and getattr(x, "is_cuda", False)


def gpu():
    """The current device, where host data goes (numpy curves, files read from disk)."""
    import torch
    if not torch.cuda.is_available():
        raise RuntimeError("modulation_mfcc_amd needs an AMD GPU (gfx950); there is no CPU fallback")
    return torch.device("cuda", torch.cuda.current_device())


# ---- counts: one integer per row ------------------------------------------------------------------------------------
def check_counts(x, batch, hi, device, what):
    """One integer count per clip, in [1, hi]: host values validated -> int64 numpy array; an int64 tensor on `device`
    as it is (shape and type checked only: no read-back)."""
    if is_device_tensor(x):
        import torch
        if x.dtype != torch.int64:
            raise TypeError(f"{what} on the device must be int64, got {x.dtype}")
        if tuple(x.shape) != (int(batch),):
            raise ValueError(f"{what} must have shape ({int(batch)},), got {tuple(x.shape)}")
        if device is not None and x.device != torch.device(device):
            raise ValueError(f"{what} is on {x.device}, the plan on {device}")
        return x.contiguous()
    arr = x.numpy() if type(x).__module__.startswith("torch") else np.asarray(x)
    if arr.dtype == np.bool_ or not np.issubdtype(arr.dtype, np.integer):
        raise TypeError(f"{what} must be integers, got {arr.dtype}")
    if arr.shape != (int(batch),):
        raise ValueError(f"{what} must have shape ({int(batch)},), got {arr.shape}")
    if int(arr.min()) < 1 or int(arr.max()) > int(hi):
        raise ValueError(f"{what} must lie in [1, {int(hi)}], got {int(arr.min())} .. {int(arr.max())}")
    return np.ascontiguousarray(arr, dtype=np.int64)


def check_lengths(lengths, batch, n_samples, device=None):
    """The `lengths` argument of the ragged calls: one valid sample count per clip of a padded [batch, n_samples] batch.

    A host sequence, numpy array or CPU tensor of integers is validated here -- shape [batch], every value in
    [1, n_samples], ValueError otherwise -- and returned as an int64 numpy array.  An int64 tensor on `device` (a
    CUDA(HIP) device) is returned as it is, with no read-back: the kernels clamp its values into [1, n_samples]."""
    return check_counts(lengths, batch, n_samples, device, "lengths")


def check_frames(frames, batch, n_frames_max, padlen=0, device=None):
    """The `frames` argument of the ragged change tail: one valid frame count per clip of a [batch, n_mfcc, n_frames_max]
    batch, checked as check_lengths checks sample counts.  Host values must also exceed `padlen`: scipy's own ValueError
    text for a clip that sosfiltfilt refuses, with the first such clip named.  An int64 tensor on `device` is returned as
    it is, with no read-back: the kernel clamps its values and writes NaN for a clip that is too short."""
    arr = check_counts(frames, batch, n_frames_max, device, "frames")
    refuse_short(arr, n_frames_max, int(padlen) + 1, lambda n: PADLEN_TEXT.format(int(padlen)), "clip", "frames")
    return arr


def counts_on_device(counts, dev):
    """The one upload of validated host counts: non-blocking, on the current stream; a device tensor passes through."""
    if not isinstance(counts, np.ndarray):
        return counts
    import torch
    return torch.from_numpy(counts).to(dev, non_blocking=True)


def group_rows(keys):
    """One host key per row [B] -> [(key, int64 index array of the rows with that key)], ascending key: the grouping behind
    every per-length route (the key is the row's length) and the Hilbert classes (its transform length)."""
    keys = np.asarray(keys)
    return [(int(k), np.flatnonzero(keys == k).astype(np.int64)) for k in np.unique(keys)]


def _frames(n, beyond, hop):
    """1 + (n - beyond) // hop of an int64 numpy array or tensor, as (n + hop - beyond) // hop: one temporary."""
    t = n + (int(hop) - int(beyond))
    t //= int(hop)
    return t


def _int64(counts):
    return counts if type(counts).__module__.startswith("torch") else np.asarray(counts, dtype=np.int64)


def centered_frames(lengths, frame_length, hop_length, center=True):
    """Frames of clips of ``lengths`` samples, 1 + (padded - frame_length) // hop_length with padded = n + 2 *
    (frame_length // 2) when centred -- mm_rms_num_frames / mm_pyin_num_frames per clip -- and 0 for a clip without a
    frame (n < 1; without centring, n < frame_length).  Host integers -> int64 numpy array, no GPU needed; an int64
    tensor -> a tensor on its device, with no read-back."""
    n, frame = _int64(lengths), int(frame_length)
    beyond = frame - 2 * (frame // 2) if center else frame      # the frame's samples that the centre padding does not supply
    t = _frames(n, beyond, hop_length)
    t *= n >= max(beyond, 1)
    return t


def stft_frames(lengths, n_fft, hop_length):
    """Frames of the centred STFT of clips of ``lengths`` >= 1 samples, 1 + (n - n_fft % 2) // hop_length
    (MfccConfig.num_frames per clip): numpy in, numpy out; an int64 tensor in, a tensor out, with no read-back."""
    return _frames(_int64(lengths), int(n_fft) % 2, hop_length)


# ---- rows: the padded batch -----------------------------------------------------------------------------------------
def device_rows(x, dtypes, type_text, shape_text, *, widen=None, one_dim=False, nonempty=True):
    """The [rows, n_max] argument of a ragged call -> x, or its contiguous copy, with unit inner stride and a row stride
    >= n_max (an expand()ed or overlapping layout is copied, a wider pitch is kept as the view it is).

    TypeError(type_text) for anything but a CUDA(HIP) tensor of one of ``dtypes``; with ``widen`` every other type is
    converted to it instead.  ValueError(shape_text) for anything but two dimensions -- ``one_dim`` takes [n] as [1, n]
    -- and, with ``nonempty``, for a batch without a row or a column."""
    if not is_device_tensor(x) or (widen is None and x.dtype not in dtypes):
        raise TypeError(type_text)
    if one_dim and x.dim() == 1:
        x = x.unsqueeze(0)
    if x.dim() != 2 or (nonempty and (x.shape[0] < 1 or x.shape[1] < 1)):
        raise ValueError(shape_text)
    if widen is not None and x.dtype not in dtypes:
        x = x.to(widen)
    rows, n_max = x.shape
    if (n_max > 1 and x.stride(1) != 1) or (rows > 1 and x.stride(0) < n_max):
        x = x.contiguous()
    return x


def batch_rows(x, shape_text, *, pitched=False):
    """The [n] or [rows, n] argument of a single-length call -> ([rows, n] with unit inner stride, whether x was [n]);
    ValueError(shape_text) for any other number of dimensions.  A strided inner axis is copied; with ``pitched`` (the
    entries that take their row pitch from row_pitch) only where n > 1, and rows closer than n (expand()ed, overlapping)
    are copied as well, as device_rows copies them."""
    squeeze = x.dim() == 1
    x2 = x.unsqueeze(0) if squeeze else x
    if x2.dim() != 2:
        raise ValueError(shape_text)
    rows, n = x2.shape
    if ((n > 1 and x2.stride(1) != 1) or (rows > 1 and x2.stride(0) < n)) if pitched else x2.stride(1) != 1:
        x2 = x2.contiguous()
    return x2, squeeze


def lens_arg(d_lens):
    """The lengths argument of an entry that serves both forms: nothing for the single-length entry (``d_lens`` None), the
    device pointer for its ``_ragged`` twin, which takes it right behind the row pitch."""
    return () if d_lens is None else (d_lens.data_ptr(),)


def row_pitch(x):
    """Elements between the rows of [rows, n] as the kernels want it (>= n; the stride of a single row says nothing:
    numpy's x[None, :] gives 0)."""
    return x.stride(0) if x.shape[0] > 1 else x.shape[1]


# ---- refusals: what scipy says to a row that is too short --------------------------------------------------------------
PADLEN_TEXT = "The length of the input vector x must be greater than padlen, which is {}."    # sosfiltfilt's, filtfilt's
SG_WINDOW_TEXT = "If mode is 'interp', window_length must be less than or equal to the size of x."      # savgol_filter's


def sos_padlen(sos):
    """scipy.signal.sosfiltfilt's default padlen for [n_sec, 6] sections: 3 * ntaps."""
    return 3 * (2 * sos.shape[0] + 1 - min(int((sos[:, 2] == 0).sum()), int((sos[:, 5] == 0).sum())))


class RowRefused(ValueError):
    """scipy's own ValueError for one row of a ragged batch, the row named: ``base`` is scipy's text, ``row`` the index."""

    def __init__(self, base, row, n):
        super().__init__(f"{base} (row {int(row)} has {int(n)} samples)")
        self.base, self.row, self.n = base, int(row), int(n)


def refuse_short(lens, n_max, least, text, noun="row", unit="samples"):
    """Rows shorter than ``least`` are the ones the single call refuses, with ``text`` (a string, or a function of the
    row's length): host counts raise it with the first such row named, before any launch; device counts only where not
    even n_max reaches (such rows come out NaN).  Rows raise RowRefused, which a list front end catches to name its
    clip; another ``noun`` (a batch whose rows are the caller's clips) raises the finished ValueError, without the count
    when ``unit`` is None."""
    if isinstance(lens, np.ndarray):
        short = np.flatnonzero(lens < least)
        if short.size:
            i, n = int(short[0]), int(lens[short[0]])
            base = text(n) if callable(text) else text
            if noun == "row":
                raise RowRefused(base, i, n)
            raise ValueError(f"{base} ({noun} {i} has {n} {unit})") if unit else named(ValueError(base), i, noun)
    elif n_max < least:
        raise ValueError(text(n_max) if callable(text) else text)


# ---- lists: clips of any lengths -> padded batches, and errors that name a clip -----------------------------------------
def named(e, i, noun="clip"):
    """The error to raise for clip ``i`` in place of ``e``: the same type and text with `` (clip i)`` appended -- for a
    RowRefused, scipy's text without the row, as a ValueError.  A caught ``e`` stays on as the cause."""
    err = ValueError(f"{e.base} ({noun} {int(i)})") if isinstance(e, RowRefused) else type(e)(f"{e} ({noun} {int(i)})")
    if e.__traceback__ is not None:
        err.__cause__ = e
    return err


def blame_clip(err, one, idx):
    """A batched call raised ``err``: run ``one(b)`` clip by clip and raise the first clip's own error with its index;
    ``err`` itself when no clip alone reproduces it."""
    for b, i in enumerate(idx):
        try:
            one(b)
        except type(err) as e:
            raise named(e, i)
    raise err


def split_by_dtype(sigs):
    """1-D tensors -> (indices of the float32 ones, indices of the others): the two batches of a list front end, so that
    every clip is computed in the precision it has alone (the others are packed as float64).  None entries -- clips a
    front end handles on the host -- are in neither."""
    import torch
    return ([i for i, s in enumerate(sigs) if s is not None and s.dtype == torch.float32],
            [i for i, s in enumerate(sigs) if s is not None and s.dtype != torch.float32])


def pack(sigs, dtype):
    """1-D tensors on one device -> (x [B, n_max] of ``dtype`` on that device, lengths int64 numpy [B]); a clip of another
    type is converted on the copy.  The padding behind each clip is left as allocated: the ragged calls never read it."""
    import torch
    lengths = np.array([s.shape[0] for s in sigs], dtype=np.int64)
    x = torch.empty((len(sigs), int(lengths.max())), dtype=dtype, device=sigs[0].device)
    for b, s in enumerate(sigs):
        x[b, :lengths[b]].copy_(s, non_blocking=True)
    return x, lengths


def packed_groups(sigs):
    """The batches of a list front end: (idx, x, lengths) for the float32 clips and for the others (as float64), each
    where there is one -- ``idx`` the clips' places in ``sigs``, ``x`` / ``lengths`` as pack returns them."""
    import torch
    for idx, dtype in zip(split_by_dtype(sigs), (torch.float32, torch.float64)):
        if idx:
            yield (idx,) + pack([sigs[i] for i in idx], dtype)
