"""The workspace-taking entries of include/*.h against the ctypes tables and the case registries, on the host, and the
self-checks of tests/ws_arena.py on CPU tensors.  tests/test_gpu_workspace.py holds every one of these entries to the
workspace contract (DESIGN.md "Workspace contract"); this file makes sure none can arrive without being held."""
import glob
import os
import re

import pytest

import stream_cases as S
import ws_arena as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# entry -> the sizers that may size its workspace (the first is the one its wrapper calls)
SIZER_OF = {
    "mm_mfcc_f32": ("mm_workspace_bytes",),
    "mm_mfcc_modspec_f32": ("mm_workspace_bytes",),
    "mm_mfcc_ragged_f32": ("mm_ragged_workspace_bytes",),
    "mm_mfcc_change_f64": ("mm_change_workspace_bytes_for", "mm_change_workspace_bytes"),
    "mm_mfcc_change_ragged_f64": ("mm_change_ragged_workspace_bytes_for",),
    "mm_sosfiltfilt_f64": ("mm_sosfiltfilt_workspace_bytes",),
    "mm_sosfiltfilt_f32_f64": ("mm_sosfiltfilt_workspace_bytes",),
    "mm_sosfiltfilt_ragged_f64": ("mm_sosfiltfilt_ragged_workspace_bytes",),
    "mm_sosfiltfilt_ragged_f32_f64": ("mm_sosfiltfilt_ragged_workspace_bytes",),
    "mm_hilbert_envelope": ("mm_hilbert_workspace_bytes",),
    "mm_hilbert_envelope_ragged": ("mm_hilbert_ragged_workspace_bytes",),
    "mm_hilbert_rfft_f32": ("mm_hilbert_rfft_workspace_bytes",),
    "mm_pyin_decode": ("mm_pyin_decode_workspace_bytes",),
    "mm_pyin_f32": ("mm_pyin_workspace_bytes",),
    "mm_pyin_f64": ("mm_pyin_workspace_bytes",),
    "mm_pyin_ragged_f32": ("mm_pyin_ragged_workspace_bytes",),
    "mm_pyin_ragged_f64": ("mm_pyin_ragged_workspace_bytes",),
    "mm_interp_nan_f64": ("mm_interp_nan_workspace_bytes",),
    "mm_interp_nan_ragged_f64": ("mm_interp_nan_workspace_bytes",),
    "mm_find_peaks": ("mm_find_peaks_workspace_bytes",),
    "mm_find_peaks_ex": ("mm_find_peaks_ex_workspace_bytes",),
    "mm_interp_spline_f64": ("mm_interp_spline_workspace_bytes",),
    "mm_interp_spline_ragged_f64": ("mm_interp_spline_workspace_bytes",),
    "mm_lombscargle_f64": ("mm_lombscargle_workspace_bytes",),
    "mm_modpsd_f32": ("mm_modpsd_workspace_bytes",),
    "mm_modcsd_f32": ("mm_modcsd_workspace_bytes",),
    "mm_zoom2d_f32": ("mm_zoom2d_workspace_bytes",),
    "mm_zoom2d_f64": ("mm_zoom2d_workspace_bytes",),
    "mm_zoom2d_ragged_f32": ("mm_zoom2d_workspace_bytes",),
    "mm_zoom2d_ragged_f64": ("mm_zoom2d_workspace_bytes",),
}

CASE_MODULES = ("test_gpu_zoom", "test_gpu_lomb", "test_gpu_modpsd", "test_gpu_modcsd", "test_gpu_spline")


def _headers():
    for path in sorted(glob.glob(os.path.join(ROOT, "include", "*.h"))):
        yield os.path.basename(path), re.sub(r"/\*.*?\*/", " ", open(path).read(), flags=re.S)


def workspace_prototypes():
    """{header: names} of all prototypes of include/*.h that have a ``size_t ...bytes`` parameter AND ``void* stream`` in
    the last place (the parser of tests/test_stream_host.py, over every header)."""
    found = {}
    for header, text in _headers():
        for m in re.finditer(r"\b(mm_\w+)\s*\(([^;{}()]*)\)\s*;", text):
            params = [p.strip() for p in m.group(2).split(",")]
            if re.fullmatch(r"void\s*\*\s*stream", params[-1]) and any(re.fullmatch(r"size_t\s+\w*bytes", p) for p in params):
                found.setdefault(header, []).append(m.group(1))
    return found


def workspace_entries():
    return [n for names in workspace_prototypes().values() for n in names]


def all_cases():
    """stream_cases.CASES and the STREAM_CASES lists of the five modules whose entries live in headers of their own."""
    import importlib
    cases = list(S.CASES)
    for mod in CASE_MODULES:
        cases += importlib.import_module(mod).STREAM_CASES
    return cases


def test_the_headers_have_30_workspace_taking_prototypes():
    """The count pins the parser.  Counted by hand in the headers, family by family.  modmfcc.h, 21: 3 of the MFCC front
    end (mm_mfcc_f32, mm_mfcc_modspec_f32, mm_mfcc_ragged_f32), 2 change tails (single and ragged; the three forms of the
    single one are one entry), 4 sosfiltfilt (f64 and f32_f64, each single and ragged), 3 Hilbert (envelope, ragged
    envelope, rfft), 5 of pYIN (decode, f32, f64, ragged f32, ragged f64), 2 interp_nan (single and ragged), 2 peak
    searches.  modmfcc_spline.h 2, modmfcc_lomb.h 1, modmfcc_modpsd.h 1, modmfcc_modcsd.h 1, modmfcc_zoom.h 4.  Every
    size_t parameter of a prototype that ends in ``void* stream`` is a workspace size."""
    found = workspace_prototypes()
    per_header = {h: len(v) for h, v in found.items()}
    assert per_header == {"modmfcc.h": 21 == 3 + 2 + 4 + 3 + 5 + 2 + 2 and 21, "modmfcc_spline.h": 2, "modmfcc_lomb.h": 1,
                          "modmfcc_modpsd.h": 1, "modmfcc_modcsd.h": 1, "modmfcc_zoom.h": 4}, per_header
    names = workspace_entries()
    assert len(names) == len(set(names)) == 30 == 21 + 2 + 1 + 1 + 1 + 4, names
    assert sorted(names) == sorted(SIZER_OF)
    # no size_t parameter in a stream-taking prototype that the pattern above does not take for a workspace size
    for _, text in _headers():
        for m in re.finditer(r"\b(mm_\w+)\s*\(([^;{}()]*\bstream\b[^;{}()]*)\)\s*;", text):
            assert ("size_t" in m.group(2)) == (m.group(1) in names), m.group(1)


def test_every_workspace_entry_has_a_sizer_in_the_bindings():
    import ctypes as C
    bound = {n: proto for t in W.tables() for n, proto in t.items()}
    for entry, sizers in SIZER_OF.items():
        assert entry in bound and C.c_size_t in bound[entry][1] and bound[entry][1][-1] is C.c_void_p, entry
        for s in sizers:
            assert "_workspace_bytes" in s and s in bound and bound[s][0] is C.c_size_t, (entry, s)
    used = {s for sizers in SIZER_OF.values() for s in sizers}
    assert sorted(used) == sorted(W.sizer_names()), "a sizer of the bindings sizes no entry, or the other way round"
    # and the header declares each of them as a size_t function
    text = " ".join(t for _, t in _headers())
    for s in used:
        assert re.search(r"\bsize_t\s+" + s + r"\s*\(", text), s


def test_every_workspace_entry_has_a_case_and_the_case_lists_import_without_a_gpu():
    cases = all_cases()
    assert len({c.name for c in cases}) == len(cases)
    covered = {c.entry for c in cases}
    missing = sorted(set(workspace_entries()) - covered)
    assert not missing, f"workspace-taking entries without a case: {missing}"
    for mod in CASE_MODULES:
        import importlib
        own = importlib.import_module(mod).STREAM_CASES
        assert own and all(isinstance(c, S.Case) for c in own), mod
    print(f"{len(cases)} cases, {sum(c.entry in SIZER_OF for c in cases)} of them on the {len(SIZER_OF)} workspace-taking entries")


# ---- the arena's self-checks, on CPU tensors ------------------------------------------------------------------------------------
@pytest.mark.parametrize("fill", W.PATTERNS)
@pytest.mark.parametrize("nbytes", [0, 1, 255, 256, 257, 10000])
def test_arena_layout(nbytes, fill):
    import torch
    a = W.Arena(nbytes, "cpu", fill)
    assert W.GUARD == 256 * 1024 and a.base.numel() == 2 * W.GUARD + (nbytes + 255) // 256 * 256 and a.base.dtype == torch.uint8
    assert a.ws.numel() == nbytes and bool((a.base == fill).all())
    if nbytes:
        assert a.ws.data_ptr() == a.base.data_ptr() + W.GUARD
    a.check("untouched")
    a.ws.fill_(fill ^ 0x5A)                      # the workspace is the entry's: writing all of it alters no guard
    a.check("workspace written")
    a.refill()
    assert bool((a.base == fill).all())


@pytest.mark.parametrize("fill", W.PATTERNS)
def test_arena_sees_a_write_on_either_side_and_names_the_offset(fill):
    n = 1000
    for index, text in ((W.GUARD + n, r"0 bytes past the workspace's end \(offset \+0 from its end\)"),
                        (W.GUARD + n + 23, r"offset \+23 from its end"),            # in the slack of the round-up
                        (W.GUARD + 1024 + 77, r"offset \+101 from its end"),        # in the guard proper
                        (2 * W.GUARD + 1024 - 1, r"offset \+262167 from its end"),  # its last byte: 24 + 262144 - 1
                        (W.GUARD - 1, r"1 bytes in front of the workspace's start \(offset -1 from its start\)"),
                        (0, r"offset -262144 from its start")):
        a = W.Arena(n, "cpu", fill)
        a.base[index] = fill ^ 0x01
        with pytest.raises(AssertionError, match=text):
            a.check("self-check")
        a.refill()
        a.check("refilled")
    a = W.Arena(n, "cpu", fill)                  # the FIRST altered byte is the one reported
    a.base[W.GUARD + n + 5] = fill ^ 0xFF
    a.base[W.GUARD + n + 900] = fill ^ 0xFF
    with pytest.raises(AssertionError, match=r"offset \+5 from its end"):
        a.check("self-check")


def test_arenas_keep_refill_check_and_count():
    import torch
    A = W.Arenas("cpu", 0x7F)
    views = [A.get(n) for n in (16, 0, 4096)]
    assert A.count == 3 and A.sizes == [16, 0, 4096] and A.of(views[2]).nbytes == 4096
    ptr = A.all[0].base.data_ptr()
    del views                                    # what a wrapper does right after its call
    assert A.all[0].base.data_ptr() == ptr and bool((A.all[0].base == 0x7F).all())
    A.all[2].ws.view(torch.float32).fill_(1.0)
    A.check("all intact")
    A.refill()
    assert bool((A.all[2].ws == 0x7F).all())
    A.all[2].base[W.GUARD - 3] = 0
    with pytest.raises(AssertionError, match=r"arena 2 of 3.*offset -3 from its start"):
        A.check("self-check")
    A.close()
    assert A.count == 0


def test_the_patterns_are_what_the_module_says():
    import numpy as np
    assert W.PATTERNS == (0x00, 0xFF, 0x7F)
    f = np.frombuffer(bytes([0x7F] * 8), dtype=np.float32)[0]
    d = np.frombuffer(bytes([0x7F] * 8), dtype=np.float64)[0]
    i = np.frombuffer(bytes([0x7F] * 4), dtype=np.int32)[0]
    assert 3.38e38 < f < 3.40e38 and 1.3e306 < d < 1.5e306 and i == 2139062143
    assert np.isnan(np.frombuffer(bytes([0xFF] * 8), dtype=np.float32)).all() and np.isnan(np.frombuffer(bytes([0xFF] * 8), dtype=np.float64)[0])
    assert np.frombuffer(bytes([0xFF] * 4), dtype=np.int32)[0] == -1
    # float_key() of csrc/mm_common.h: a float >= 0 is its own bits, a negative one lies below every positive one -- so the
    # 0x7F word is the key of 3.39e38 and beats the key of every log-mel value there can be; 0xFF (-1) beats none >= 0
    def key(v):
        b = int(np.array([v], dtype=np.float32).view(np.int32)[0])
        return b if b >= 0 else b ^ 0x7FFFFFFF
    assert key(f) == i and all(key(v) < i for v in (-3e38, -100.0, 0.0, 200.0, 1e38)) and key(-100.0) < -1 < key(0.0)


def test_the_hand_out_condition():
    A = W.Arenas("cpu", 0)
    A.sized.append(("mm_x_workspace_bytes", 0))
    A.check_handed_out("a Welch call without a second launch")
    A.sized.append(("mm_x_workspace_bytes", 4096))
    with pytest.raises(AssertionError, match="no workspace was taken"):
        A.check_handed_out("self-check")
    A.get(4096)
    A.check_handed_out("exactly what the sizer named")
    A.get(4112)
    with pytest.raises(AssertionError, match=r"\[4112\] bytes"):
        A.check_handed_out("self-check")
