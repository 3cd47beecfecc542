"""CPU: the host side of the interp_NAN kinds and of the articulograph reader (csrc/mm_interp.hip, modulation_mfcc_amd.ema):
exported symbols, argument checks that happen before any launch, the workspace formula, the .pos header."""
import ctypes as C

import numpy as np
import pytest

from modulation_mfcc_amd import _lib, interp

KINDS = ["pchip", "nearest", "nearest-up", "previous", "next", "zero", "slinear"]


def write_pos(path, data, channels, rate, header_size=70):
    """A .pos file as the reader expects it: four text lines padded to the size line 2 states, then float32 records."""
    head = f"AG50xDATA_V002\n{header_size:08d}\nNumberOfChannels={channels}\nSamplingFrequencyHz={rate}\n".encode("utf8")
    assert len(head) <= header_size
    with open(path, "wb") as f:
        f.write(head + b" " * (header_size - len(head)))
        f.write(np.ascontiguousarray(data, dtype=np.float32).tobytes())


def test_library_exports_the_interp_symbols():
    lib = C.CDLL(_lib.LIB_PATH)
    for name in ("mm_interp_nan_f64", "mm_interp_nan_workspace_bytes", "mm_regrid_linear_f32_f64"):
        assert hasattr(lib, name), name
        assert name in _lib.PROTOTYPES


def test_public_names_import_from_the_package_root():
    from modulation_mfcc_amd import interp_nan_batch, read_AG50x, read_AG50x_arrays, read_pos_header
    from modulation_mfcc_amd import calc, ema
    assert calc.interp_nan_batch is interp_nan_batch is interp.interp_nan_batch
    assert calc.read_AG50x is read_AG50x is ema.read_AG50x
    assert calc.read_AG50x_arrays is read_AG50x_arrays and calc.read_pos_header is read_pos_header
    assert interp.INTERP_SEGMENT == 1024
    assert sorted(interp._INTERP_KINDS) == sorted(KINDS) and sorted(interp._INTERP_KINDS.values()) == list(range(7))


def test_the_method_table_has_every_kind_once_with_the_librarys_entries_and_codes():
    """interp._METHODS: the ten method names, each with the C entry pair, the workspace query and the kind code that the
    prototype tables and the two headers list; the moved constants still equal the kernels'."""
    import os
    import re
    from conftest import ROOT
    T = interp._METHODS
    assert sorted(T) == sorted(["linear"] + KINDS + ["quadratic", "cubic"]) and len(T) == 10
    head = open(os.path.join(ROOT, "include", "modmfcc.h")).read()
    codes = {m.group(1).lower().replace("_", "-"): int(m.group(2)) for m in re.finditer(r"\bMM_INTERP_([A-Z_]+)\s*=\s*(\d+)", head)}
    assert sorted(codes) == sorted(KINDS)
    codes.update(quadratic=_lib.MM_SPLINE_QUADRATIC, cubic=_lib.MM_SPLINE_CUBIC)
    want = {"linear": (interp._LINEAR, _lib.PROTOTYPES, "mm_interp_nan_linear_f64", "mm_interp_nan_linear_ragged_f64", None)}
    want.update({k: (interp._SEGMENTED, _lib.PROTOTYPES, "mm_interp_nan_f64", "mm_interp_nan_ragged_f64", "mm_interp_nan_workspace_bytes")
                 for k in KINDS})
    want.update({k: (interp._SPLINE, _lib.PROTOTYPES_SPLINE, "mm_interp_spline_f64", "mm_interp_spline_ragged_f64",
                     "mm_interp_spline_workspace_bytes") for k in ("quadratic", "cubic")})
    for name, m in T.items():
        family, table, entry, ragged_entry, workspace = want[name]
        assert (m.family, m.entry, m.ragged_entry, m.workspace) == (family, entry, ragged_entry, workspace), name
        one, many = table[m.entry][1], table[m.ragged_entry][1]
        assert table[m.entry][0] is C.c_int and table[m.ragged_entry][0] is C.c_int
        assert len(many) == len(one) + 1 and one[-1] is C.c_void_p and many[-1] is C.c_void_p, name      # the counts; the stream
        if name == "linear":
            assert m.kind == 0 and one[0] is C.c_void_p                    # no kind argument, no workspace
        else:
            assert m.kind == codes[name], name
            assert one[0] is C.c_int32 and many[0] is C.c_int32 and table[m.workspace] == (C.c_size_t, [C.c_int32, C.c_int64, C.c_int64])
    assert {k: T[k].kind for k in KINDS} == interp._INTERP_KINDS and {k: T[k].kind for k in ("quadratic", "cubic")} == interp._SPLINE_KINDS
    assert interp.INTERP_SEGMENT == interp.SPLINE_CHUNK == 1024
    csrc = os.path.join(ROOT, "modulation_mfcc_amd", "csrc")
    seg = open(os.path.join(csrc, "mm_interp_seg.hip.inc")).read()
    assert "kIpThreads = 256;" in seg and "kIpPer = 4;" in seg and "kIpSeg = kIpThreads * kIpPer;" in seg
    assert f"kSpChunk = {interp.SPLINE_CHUNK};" in open(os.path.join(csrc, "mm_spline.hip")).read()


def test_entry_points_validate_before_any_launch():
    lib = _lib.load()
    S = interp.INTERP_SEGMENT
    for kind in range(7):
        assert lib.mm_interp_nan_workspace_bytes(kind, 1024, 1000) == 2 * 1024 * 16 + 1024 * 16
        assert lib.mm_interp_nan_workspace_bytes(kind, 1, 300001) == 2 * 4864 + 256       # 294 segments, padded to 256 B
        assert lib.mm_interp_nan_workspace_bytes(kind, 64, S) == lib.mm_interp_nan_workspace_bytes(kind, 64, 1)
        assert lib.mm_interp_nan_workspace_bytes(kind, 64, S + 1) == lib.mm_interp_nan_workspace_bytes(kind, 64, S) + 2 * 64 * 16
    assert lib.mm_interp_nan_workspace_bytes(7, 1, 10) == 0 and lib.mm_interp_nan_workspace_bytes(-1, 1, 10) == 0
    assert lib.mm_interp_nan_workspace_bytes(0, 0, 10) == 0 and lib.mm_interp_nan_workspace_bytes(0, 1, 0) == 0
    assert lib.mm_interp_nan_workspace_bytes(0, 1, 2 ** 31 - S) == 0                     # int32 indices
    one = C.c_void_p(256)            # never dereferenced: every call below fails its checks first
    assert lib.mm_interp_nan_f64(0, None, 1, 10, 10, one, 10, one, 1 << 20, None) == _lib.MM_ERR_INVALID_ARG
    assert lib.mm_interp_nan_f64(7, one, 1, 10, 10, one, 10, one, 1 << 20, None) == _lib.MM_ERR_INVALID_ARG
    assert lib.mm_interp_nan_f64(0, one, 1, 10, 9, one, 10, one, 1 << 20, None) == _lib.MM_ERR_INVALID_ARG
    assert lib.mm_interp_nan_f64(0, one, 1, 10, 10, one, 9, one, 1 << 20, None) == _lib.MM_ERR_INVALID_ARG
    assert lib.mm_interp_nan_f64(0, one, 0, 10, 10, one, 10, one, 1 << 20, None) == _lib.MM_ERR_INVALID_ARG
    assert lib.mm_interp_nan_f64(0, one, 1, 10, 10, one, 10, None, 1 << 20, None) == _lib.MM_ERR_INVALID_ARG
    assert lib.mm_interp_nan_f64(0, one, 1, 10, 10, one, 10, one, 15, None) == _lib.MM_ERR_WORKSPACE
    assert lib.mm_regrid_linear_f32_f64(None, 2, 1, 1, one, one, 1, one, 1, None) == _lib.MM_ERR_INVALID_ARG
    assert lib.mm_regrid_linear_f32_f64(one, 1, 1, 1, one, one, 1, one, 1, None) == _lib.MM_ERR_INVALID_ARG    # n < 2
    assert lib.mm_regrid_linear_f32_f64(one, 2, 4, 3, one, one, 1, one, 4, None) == _lib.MM_ERR_INVALID_ARG
    assert lib.mm_regrid_linear_f32_f64(one, 2, 4, 4, one, one, 0, one, 4, None) == _lib.MM_ERR_INVALID_ARG
    assert lib.mm_regrid_linear_f32_f64(one, 2, 4, 4, one, one, 1, one, 3, None) == _lib.MM_ERR_INVALID_ARG
    assert lib.mm_version() == 123


def test_interp_nan_batch_takes_device_tensors_only():
    with pytest.raises(TypeError):
        interp.interp_nan_batch(np.array([1.0, np.nan, 3.0]), "pchip")


@pytest.mark.parametrize("channels,rate,size", [(16, 250, 70), (8, 400, 128), (32, 1250, 4096)])
def test_read_pos_header(tmp_path, channels, rate, size):
    from modulation_mfcc_amd import read_pos_header
    p = tmp_path / "a.pos"
    write_pos(p, np.zeros((3, 7 * channels)), channels, rate, header_size=size)
    h = read_pos_header(p)
    assert (h["header_size"], h["channels"], h["samplerate"]) == (size, channels, rate)
    assert h["lines"][0] == "AG50xDATA_V002" and h["lines"][2] == f"NumberOfChannels={channels}"


def test_a_32_channel_header_is_numpys_value_error(tmp_path):
    """The reference's table gives 256 floats a record for 32 channels: they do not reshape to (-1, 7).  No layout is
    guessed; the error comes before anything touches the device."""
    from modulation_mfcc_amd import read_AG50x_arrays
    p = tmp_path / "b.pos"
    write_pos(p, np.zeros((4, 256)), 32, 250)
    with pytest.raises(ValueError, match="reshape"):
        read_AG50x_arrays(p)
    write_pos(p, np.zeros((4, 224)), 32, 250)            # 32 x 7 floats a record: no multiple of 256 either way
    with pytest.raises(ValueError, match="reshape"):
        read_AG50x_arrays(p)
    write_pos(p, np.zeros((4, 28)), 4, 250)              # a channel count the table does not have: the reference's KeyError
    with pytest.raises(KeyError):
        read_AG50x_arrays(p)
