"""Articulograph data: ``read_AG50x`` of the reference (script/calc.py:173-219, called from script/main.py:1310).

A Carstens AG50x ``.pos`` file is a short text header followed by float32 records, one per sample time, of
``channels x 7`` values (x, z, y, phi, theta, rms, extra).  The reference regrids every one of those columns to a target
rate with ``scipy.interpolate.interp1d(original_time, column, 'linear')``; here the records go to the device as they lie
in the file and one kernel (mm_regrid_linear_f32_f64, csrc/mm_interp.hip) does all columns, in scipy's arithmetic.  The
result is a device tensor, ready for velocity_batch, applyFilter and find_peaks_batch.  The time axes are the
reference's, quirks included, computed with numpy on the host exactly as it writes them.
"""
from __future__ import annotations


import numpy as np

from . import ragged

DIMENSIONS = ["x", "z", "y", "phi", "theta", "rms", "extra"]
# float32 values per record, by channel count: the reference's table.  Its entry for 32 channels is no multiple of 7,
# so such a file fails in numpy's reshape there, and here.
RECORD_FLOATS = {8: 56, 16: 112, 32: 256}

__all__ = ["read_pos_header", "read_AG50x_arrays", "read_AG50x", "DIMENSIONS"]


def _parse_header(content: bytes):
    # line 2 holds the header's size in bytes; the header's lines 3 and 4 end in "=<channels>" and "=<rate>"
    second = content.split(b"\n", 2)[1]
    header_size = int(second.decode("utf8"))
    lines = content[:header_size].decode("utf8").split("\n")
    return dict(header_size=header_size, channels=int(lines[2].split("=")[1]), samplerate=int(lines[3].split("=")[1]),
                lines=lines)


def read_pos_header(path):
    """The header of a ``.pos`` file -> dict(header_size, channels, samplerate, lines).  Host only."""
    with open(path, "rb") as f:
        return _parse_header(f.read())


def read_AG50x_arrays(path, target_sample_rate=200, device=None):
    """``read_AG50x`` without xarray -> dict(ema, time, channels, dimensions, attrs): ``ema`` a float64 CUDA(HIP) tensor
    [m, channels, 7] on ``device`` (default: the current one), ``time`` the numpy [m] target times, ``channels``
    np.arange(channels), ``dimensions`` the seven names, ``attrs`` the reference's (device, duration,
    original_samplerate, resampled_samplerate).

    The reference's arithmetic, kept to the letter: ``original_time = np.linspace(0, n / rate, n)`` (spacing
    n / rate / (n - 1), not 1 / rate), ``time = np.arange(0, original_time[-1], 1 / target_sample_rate)``, both taken on
    the host; the values by interp1d's linear rule for float32 samples on the device (mm_regrid_linear_f32_f64).  A
    header that announces 32 channels raises numpy's ValueError, as it does in the reference."""
    import torch
    from . import _lib
    with open(path, "rb") as f:
        content = f.read()
    h = _parse_header(content)
    data = np.frombuffer(content[h["header_size"]:], np.float32)
    data = np.reshape(data, (-1, RECORD_FLOATS[h["channels"]]))
    pos = data.reshape(len(data), -1, 7)
    n, channels = pos.shape[0], pos.shape[1]
    original_time = np.linspace(0, n / h["samplerate"], n)
    new_time = np.arange(0, original_time[-1], 1 / target_sample_rate)
    if n < 2:
        raise ValueError("x and y arrays must have at least 2 entries")      # interp1d's, for a file of one record
    dev = torch.device(device) if device is not None else ragged.gpu()
    m, cols = len(new_time), channels * 7
    out = torch.empty((m, channels, 7), dtype=torch.float64, device=dev)
    if m > 0:
        y = torch.from_numpy(np.array(data)).to(dev)              # a writable copy: np.frombuffer's view is read-only
        t_in = torch.from_numpy(original_time).to(dev)
        t_out = torch.from_numpy(new_time).to(dev)
        _lib.call("mm_regrid_linear_f32_f64", dev, y.data_ptr(), n, cols, cols, t_in.data_ptr(), t_out.data_ptr(), m,
                  out.data_ptr(), cols)
    return dict(ema=out, time=new_time, channels=np.arange(channels), dimensions=list(DIMENSIONS),
                attrs=dict(device="AG50x", duration=new_time[-1], original_samplerate=h["samplerate"],
                           resampled_samplerate=target_sample_rate))


def read_AG50x(path_to_pos_file, target_sample_rate=200):
    """script/calc.py:173-219: the ``.pos`` file regridded to ``target_sample_rate`` as the reference's xarray.Dataset
    (variable ``ema`` over time x channels x dimensions).  The regrid runs on the device (read_AG50x_arrays); the
    Dataset holds host memory, so use read_AG50x_arrays to keep the data on the device.  xarray is imported here, on
    first use."""
    try:
        import xarray as xr
    except ImportError as e:
        raise ImportError("read_AG50x returns an xarray.Dataset and xarray is not installed; "
                          "read_AG50x_arrays gives the same data without it") from e
    a = read_AG50x_arrays(path_to_pos_file, target_sample_rate)
    return xr.Dataset(
        data_vars=dict(ema=(["time", "channels", "dimensions"], a["ema"].cpu().numpy())),
        coords=dict(time=(["time"], a["time"]), channels=(["channels"], a["channels"]),
                    dimensions=(["dimensions"], a["dimensions"])),
        attrs=a["attrs"])
