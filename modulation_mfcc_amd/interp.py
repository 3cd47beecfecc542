"""Gap filling: the reference's ``interp_NAN`` (script/calc.py:345-385) on the GPU, every kind of it.

    interp_NAN(X, method='linear')                      -> the reference's signature: numpy curves and device tensors
    interp_nan_batch(x, method)                         -> 'linear' and the seven segmented kinds, device tensors only
    interp_nan_ragged_batch(x, counts, method)          -> the same with a count per row
    interp_nan_spline_batch(x, 'quadratic' | 'cubic')   -> scipy's spline kinds on the device
    interp_nan_spline_ragged_batch(x, counts, method)   -> the same with a count per row

Ten method names in three families (``_METHODS``): 'linear' (csrc/mm_interp.hip, a workgroup per row), the segmented
kinds 'pchip', 'nearest', 'nearest-up', 'previous', 'next', 'zero', 'slinear' (csrc/mm_interp.hip, a workgroup per
INTERP_SEGMENT samples) and the splines 'quadratic', 'cubic' (csrc/mm_spline.hip).  What a family asks of a row and what
it refuses with is one ``_Family`` each; the five calls are front ends -- their own order of argument checks -- over one
body, ``_fill``.
"""
from __future__ import annotations

import collections

import numpy as np
from scipy import interpolate

from . import ragged

__all__ = ["interp_NAN", "interp_nan_batch", "interp_nan_ragged_batch", "interp_nan_spline_batch",
           "interp_nan_spline_ragged_batch"]

INTERP_SEGMENT = 1024       # samples per workgroup of the segmented interp_NAN kernels (kIpSeg of csrc/mm_interp_seg.hip.inc)
SPLINE_CHUNK = 1024         # knots per workgroup of the spline solve (kSpChunk of csrc/mm_spline.hip): longer rows are cut
# interp_NAN methods of mm_interp_nan_f64 (MM_INTERP_* of include/modmfcc.h)
_INTERP_KINDS = {"pchip": 0, "nearest": 1, "nearest-up": 2, "previous": 3, "next": 4, "zero": 5, "slinear": 6}
# interp_NAN methods of mm_interp_spline_f64 (MM_SPLINE_* of include/modmfcc_spline.h): the kind is the spline's degree
_SPLINE_KINDS = {"quadratic": 2, "cubic": 3}
_INTERP_HOST_KINDS = ("quadratic", "cubic")     # a banded solve over all knots: interp_NAN runs them through scipy on the host

_MSG_TWO = "x and y arrays must have at least 2 entries"                    # scipy interp1d with one point
_MSG_EMPTY = "cannot reshape array of size 0 into shape (0,newaxis)"         # scipy interp1d of empty x
_MSG_NO_SAMPLE = "index 0 is out of bounds for axis 0 with size 0"           # the reference's np.argwhere(...)[0] of an empty array
_MSG_SPLINE_FEW = "The number of derivatives at boundaries does not match: expected {}, got 0+0"   # make_interp_spline's


# ---------------------------------------------------------------------------------------------------------------------
# the three families: what each asks of a row, and what it says to a row that falls short
# ---------------------------------------------------------------------------------------------------------------------
def _linear_refuse(kind, fewest):
    raise ValueError(_MSG_TWO)


def _segmented_refuse(kind, fewest):
    if kind == _INTERP_KINDS["slinear"]:
        raise ValueError(_MSG_TWO)
    if kind == _INTERP_KINDS["pchip"]:
        raise IndexError(_MSG_NO_SAMPLE)
    raise ValueError(_MSG_EMPTY)


def _spline_refuse(kind, fewest):
    """scipy's ValueError for the row with the fewest valid samples among the rows that have a NaN."""
    if fewest < 1:
        raise ValueError(_MSG_EMPTY)
    if fewest <= kind:
        raise ValueError(_MSG_SPLINE_FEW.format(kind + 1 - fewest))


# least(kind)   the valid samples a row needs; ``refuse(kind, fewest)`` raises for a row with fewer
# clean_pass    a row without a NaN needs none: it is returned as it is ('linear' refuses it like any other row)
# as_is         the call without counts returns a tensor with nothing to fill -- no row, no column, or no NaN anywhere --
#               as its clone, without a launch ('linear' takes every tensor to the kernel)
# any_dtype     the call without counts takes a tensor that is not floating point (computed in float64, cast back)
# packed        the call without counts copies a wider row pitch away
_Family = collections.namedtuple("_Family", "least refuse clean_pass as_is any_dtype packed")
_LINEAR = _Family(lambda kind: 2, _linear_refuse, clean_pass=False, as_is=False, any_dtype=True, packed=True)
_SEGMENTED = _Family(lambda kind: 2 if kind == _INTERP_KINDS["slinear"] else 1, _segmented_refuse,
                     clean_pass=True, as_is=True, any_dtype=False, packed=False)
_SPLINE = _Family(lambda kind: kind + 1, _spline_refuse, clean_pass=True, as_is=True, any_dtype=False, packed=False)

# method name -> family, kind code, C entry without / with counts, workspace query (None: the entries take no kind and no
# workspace)
_Method = collections.namedtuple("_Method", "family kind entry ragged_entry workspace")
_METHODS = {"linear": _Method(_LINEAR, 0, "mm_interp_nan_linear_f64", "mm_interp_nan_linear_ragged_f64", None)}
_METHODS.update((name, _Method(_SEGMENTED, kind, "mm_interp_nan_f64", "mm_interp_nan_ragged_f64", "mm_interp_nan_workspace_bytes"))
                for name, kind in _INTERP_KINDS.items())
_METHODS.update((name, _Method(_SPLINE, kind, "mm_interp_spline_f64", "mm_interp_spline_ragged_f64",
                               "mm_interp_spline_workspace_bytes")) for name, kind in _SPLINE_KINDS.items())


# ---------------------------------------------------------------------------------------------------------------------
# the one body
# ---------------------------------------------------------------------------------------------------------------------
def _fill(xd, pitch, counts, m):
    """float64 rows ``xd`` [rows, n] (unit inner stride, ``pitch`` >= n elements from row to row), ``counts`` (validated
    host counts, an int64 device tensor, or None: every row has n samples) and the method's table entry -> the filled
    rows, float64 [rows, n] (zeros behind a row's count); None where the family returns a tensor without a NaN as it is.  Counts the valid
    samples of every row, raises what scipy raises for the row with the fewest, launches on the current stream."""
    import torch
    from . import _lib
    fam, kind = m.family, m.kind
    rows, n = xd.shape
    dev = xd.device
    with torch.cuda.device(dev):
        ok = ~torch.isnan(xd)
        least = fam.least(kind)
        if counts is None:
            cd, valid = None, ok.sum(dim=1)
        else:
            cd = ragged.counts_on_device(counts, dev)
            full = cd.clamp(1, n)
            valid = (ok & (torch.arange(n, device=dev)[None, :] < full[:, None])).sum(dim=1)
            if fam.clean_pass:          # (alone, such a row has n samples: more than any row with a NaN)
                valid = torch.where(valid < full, valid, torch.full_like(valid, least))
        # the one read-back
        if fam.clean_pass or cd is not None:
            fewest = int(valid.min())
            if cd is None and fam.as_is and fewest == n:
                return None
        else:                           # (a batch without a row has no row to refuse)
            fewest = 0 if bool((valid < least).any()) else least
        if fewest < least:
            fam.refuse(kind, fewest)
        y = torch.empty((rows, n), dtype=torch.float64, device=dev)
        lib = _lib.load()
        args = [xd.data_ptr(), rows, n, pitch] + ([] if cd is None else [cd.data_ptr()]) + [y.data_ptr(), n]
        if m.workspace is not None:
            ws = _lib.workspace(getattr(lib, m.workspace)(kind, rows, n), dev)
            args = [kind] + args + [ws.data_ptr(), ws.numel()]
        _lib.call(m.entry if cd is None else m.ragged_entry, dev, *args)
    return y


def _alone(x, m, X):
    """A call without counts on a device tensor [n] or [rows, n] (``X``: the argument's name in the refusals)."""
    import torch
    fam = m.family
    squeeze = x.dim() == 1
    xs = x.unsqueeze(0) if squeeze else x
    if xs.dim() != 2:
        raise ValueError(f"{X} must be [n] or [rows, n]")
    if not (fam.any_dtype or xs.is_floating_point()):
        raise TypeError(f"{X} must be a floating-point tensor")
    rows, n = xs.shape
    if fam.as_is and (rows == 0 or n == 0):
        return x.clone()
    xd = xs.to(torch.float64)
    if fam.packed or xd.stride(1) != 1 or xd.stride(0) < n:
        xd = xd.contiguous()
    # (the segmented entry gets a single row's stride as the tensor has it, and refuses a [1, n] view whose stride is
    # below n -- numpy's x[None, :] gives 0 -- with ValueError: kept as it was when this module was written)
    y = _fill(xd, xd.stride(0) if fam is _SEGMENTED else ragged.row_pitch(xd), None, m)
    if y is None:
        return x.clone()
    y = y.to(x.dtype)
    return y[0] if squeeze else y


def _ragged_rows(x, who):
    import torch
    return ragged.device_rows(x, (torch.float64,), f"{who} takes a CUDA(HIP) tensor", "x must be [rows, n_max]",
                              widen=torch.float64, nonempty=False)


def _with_counts(x, xd, counts, m):
    """A call with counts: ``xd`` = _ragged_rows(x)."""
    if not x.is_floating_point():
        raise TypeError("x must be a floating-point tensor")
    rows, n = x.shape
    if rows == 0 or n == 0:
        return x.clone()
    return _fill(xd, ragged.row_pitch(xd), ragged.check_counts(counts, rows, n, x.device, "counts"), m).to(x.dtype)


def _device_method(method, who):
    """The table entry of a method of interp_nan_batch / interp_nan_ragged_batch."""
    if method in _INTERP_HOST_KINDS:
        raise NotImplementedError(f"method={method!r} needs a banded solve over all knots; not on the device")
    if method not in _METHODS:
        raise ValueError(f"{who}: unknown method {method!r}")
    return _METHODS[method]


def _spline_method(method, who):
    if method not in _SPLINE_KINDS:
        raise ValueError(f"{who}: method must be 'quadratic' or 'cubic', got {method!r}")
    return _METHODS[method]


# ---------------------------------------------------------------------------------------------------------------------
# the calls
# ---------------------------------------------------------------------------------------------------------------------
def interp_nan_batch(x, method: str = "linear"):
    """interp_NAN along the last axis of a CUDA(HIP) tensor [n] or [rows, n] of any float dtype, on the device only:
    computed in float64 and cast back.  ``method``: 'linear' (mm_interp_nan_linear_f64) or one of 'pchip', 'nearest',
    'nearest-up', 'previous', 'next', 'zero', 'slinear' (mm_interp_nan_f64; rows are cut into segments of INTERP_SEGMENT
    samples, one workgroup each).  'quadratic' and 'cubic' need a solve over all knots: NotImplementedError here
    (interp_NAN runs them through scipy on the host); any other name is a ValueError.  Rows with too few valid samples
    raise what the reference raises (interp_NAN's doc string), after one read-back of the smallest count."""
    if not ragged.is_device_tensor(x):
        raise TypeError("interp_nan_batch takes a CUDA(HIP) tensor; interp_NAN also takes numpy curves")
    return _alone(x, _device_method(method, "interp_nan_batch"), "X")


def interp_nan_ragged_batch(x, counts, method: str = "linear"):
    """interp_nan_batch with a count per row: ``x`` [rows, n_max] on the device, ``counts`` [rows] (host integers,
    validated: ValueError outside [1, n_max]; or an int64 device tensor, clamped by the kernels) -> [rows, n_max] of x's
    dtype.  Row b holds interp_nan_batch(x[b, :counts[b]], method) in the columns [0, counts[b]) and zeros behind them;
    what x holds behind a row's count never matters.  The methods and the errors are interp_nan_batch's, the errors taken
    from the smallest number of valid samples below a row's count, in one read-back."""
    xd = _ragged_rows(x, "interp_nan_ragged_batch")
    return _with_counts(x, xd, counts, _device_method(method, "interp_nan_ragged_batch"))


def interp_nan_spline_batch(x, method: str = "cubic"):
    """interp_NAN's 'quadratic' and 'cubic' kinds along the last axis of a CUDA(HIP) tensor [n] or [rows, n] of any float
    dtype, on the device only (mm_interp_spline_f64): computed in float64 and cast back.  scipy's
    interp1d(valid indices, valid values, method, fill_value='extrapolate') at the NaN samples -- the not-a-knot cubic
    spline, the quadratic spline with its knots at the midpoints -- within a few of scipy's own roundings, not bit for
    bit; samples before the first and behind the last valid one are extrapolated with the end pieces.  The valid samples
    of a row are compacted by rank, the tridiagonal system of a row is solved in LDS, in chunks of SPLINE_CHUNK knots
    for a longer row.  A row without a NaN is returned as it is; a row with a NaN and fewer than 3 ('quadratic') or 4
    ('cubic') valid samples raises scipy's ValueError, after one read-back of the smallest count.  Another method name
    is a ValueError, a host array a TypeError.  interp_NAN and interp_nan_batch do not route here."""
    m = _spline_method(method, "interp_nan_spline_batch")
    if not ragged.is_device_tensor(x):
        raise TypeError("interp_nan_spline_batch takes a CUDA(HIP) tensor")
    return _alone(x, m, "x")


def interp_nan_spline_ragged_batch(x, counts, method: str = "cubic"):
    """interp_nan_spline_batch with a count per row: ``x`` [rows, n_max] on the device, ``counts`` [rows] (host integers,
    validated: ValueError outside [1, n_max]; or an int64 device tensor, clamped by the kernels) -> [rows, n_max] of x's
    dtype.  Row b holds interp_nan_spline_batch(x[b, :counts[b]], method) in the columns [0, counts[b]), bit for bit, and
    zeros behind them; what x holds behind a row's count never matters.  The errors are interp_nan_spline_batch's, taken
    from the smallest number of valid samples below a row's count, in one read-back."""
    m = _spline_method(method, "interp_nan_spline_ragged_batch")
    return _with_counts(x, _ragged_rows(x, "interp_nan_spline_ragged_batch"), counts, m)


def _interp_nan_host(X, method):
    # script/calc.py:345-385 as written
    import copy
    newX = copy.copy(X)
    mynans = np.isnan(newX)
    if np.sum(mynans) == 0:
        return newX
    justnans = np.empty(np.size(X))
    justnans[:] = np.nan
    if method == "pchip":
        if np.argwhere(mynans)[0] == 0:
            newX[0] = newX[np.argwhere(np.isnan(newX) == 0)[0]]
        if np.argwhere(mynans)[-1] == len(X) - 1:
            newX[-1] = newX[np.argwhere(np.isnan(newX) == 0)[-1]]
        mynans = np.isnan(newX)
        f = interpolate.PchipInterpolator(np.where(mynans == 0)[0], newX[mynans == 0], extrapolate=False)
    else:
        f = interpolate.interp1d(np.where(mynans == 0)[0], newX[mynans == 0], method, fill_value="extrapolate")
    justnans[mynans] = f(np.squeeze(np.where(mynans)))
    newX[mynans] = justnans[mynans]
    return newX


def interp_NAN(X, method: str = "linear"):
    """script/calc.py:345-385: NaN samples of a curve filled by interpolation.  'linear' (scipy interp1d, extrapolated at
    the ends) runs on the device (mm_interp_nan_linear_f64) for numpy curves and CUDA(HIP) tensors ([n] or [rows, n]).
    A CUDA(HIP) tensor stays on the device for 'pchip' (PchipInterpolator after the reference's end fix), 'nearest',
    'nearest-up', 'previous', 'next', 'zero' and 'slinear' too (interp_nan_batch, mm_interp_nan_f64); only 'quadratic' and
    'cubic', which solve a banded system over all knots, take a device tensor through scipy on the host and back.  A
    numpy curve with any method but 'linear' runs the reference's own scipy calls.  On the device a row without a valid
    sample raises IndexError under 'pchip' and scipy's ValueError for empty input otherwise; 'linear' and 'slinear' need
    two valid samples (ValueError)."""
    if method == "linear":
        if ragged.is_device_tensor(X):
            return _alone(X, _METHODS[method], "X")
        a = np.asarray(X)
        if np.sum(np.isnan(a)) == 0:
            return a.copy()
        import torch
        y = _alone(torch.from_numpy(np.ascontiguousarray(a)).to(ragged.gpu()), _METHODS[method], "X")
        return y.cpu().numpy()
    if ragged.is_device_tensor(X):
        if method in _INTERP_KINDS:
            return _alone(X, _METHODS[method], "X")
        import torch
        rows = X.cpu().numpy()
        out = _interp_nan_host(rows, method) if rows.ndim == 1 else np.stack([_interp_nan_host(r, method) for r in rows])
        return torch.from_numpy(np.ascontiguousarray(out)).to(X.device)
    return _interp_nan_host(X, method)
