"""The registry of tests/stream_cases.py against include/modmfcc.h, on the host: every compute entry of the C ABI has a
case (so a new entry cannot arrive without its stream contract being tested: tests/test_gpu_streams.py), and every
case's two data sets really are two."""
import os
import re

import numpy as np
import pytest

import stream_cases as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def stream_prototypes():
    """The names of all prototypes of include/modmfcc.h whose LAST parameter is ``void* stream``."""
    text = open(os.path.join(ROOT, "include", "modmfcc.h")).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    names = []
    for m in re.finditer(r"\b(mm_\w+)\s*\(([^;{}()]*)\)\s*;", text):
        params = [p.strip() for p in m.group(2).split(",")]
        if re.fullmatch(r"void\s*\*\s*stream", params[-1]):
            names.append(m.group(1))
    return names


def test_the_header_has_47_stream_taking_prototypes():
    """The count pins the parser: a prototype it failed to recognise would otherwise leave the completeness check blind.
    Counted by hand in the header, family by family: 9 of the MFCC front end and its tail, 12 filters and stencils, 5
    envelopes, 7 of the input side, 7 of pYIN, 5 interpolations, 2 peak searches.  No prototype mentions a stream anywhere
    but in its last place."""
    names = stream_prototypes()
    assert len(names) == len(set(names)) == 47 == 9 + 12 + 5 + 7 + 7 + 5 + 2, names
    assert names[0] == "mm_mfcc_f32" and names[-1] == "mm_find_peaks_ex"
    text = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "modmfcc.h")).read(), flags=re.S)
    anywhere = [m.group(1) for m in re.finditer(r"\b(mm_\w+)\s*\(([^;{}()]*\bstream\b[^;{}()]*)\)\s*;", text)]
    assert anywhere == names


def test_every_compute_entry_has_a_case():
    names = set(stream_prototypes())
    covered = {c.entry for c in S.CASES}
    assert not names - covered, f"compute entries without a case in tests/stream_cases.py: {sorted(names - covered)}"
    assert not covered - names, f"cases that name a symbol the header lacks: {sorted(covered - names)}"
    print(f"{len(S.CASES)} cases cover {len(names)} entries: " +
          ", ".join(f"{n} x{sum(c.entry == n for c in S.CASES)}" for n in sorted(names)))


def test_the_bindings_know_every_compute_entry():
    """The ctypes table of the package declares every one of them with a void* in the last place."""
    import ctypes as C
    from modulation_mfcc_amd._lib import PROTOTYPES
    for n in stream_prototypes():
        assert n in PROTOTYPES and PROTOTYPES[n][1][-1] is C.c_void_p, n


def test_case_names_are_unique_and_threads_cases_take_a_handle():
    assert len({c.name for c in S.CASES}) == len(S.CASES)
    text = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "modmfcc.h")).read(), flags=re.S)
    with_handle = {m.group(1) for m in re.finditer(r"\b(mm_\w+)\s*\(\s*(?:const\s+)?mm_(?:plan|hilbert)\s*\*", text)}
    with_handle = (with_handle & set(stream_prototypes())) | {"mm_pyin_f32"}
    threaded = {c.entry for c in S.CASES if c.threads}
    assert threaded == with_handle, (sorted(with_handle - threaded), sorted(threaded - with_handle))


@pytest.mark.parametrize("case", S.CASES, ids=lambda c: c.name)
def test_the_two_data_sets_differ_in_every_buffer(case):
    """Set 0 and set 1 differ in every input buffer, lengths included (same shapes and types: they share the buffers), and
    a ragged case's set 1 has a row at n_max, a row at the smallest length and rows in between."""
    host = case.data()
    assert host, case.name
    for key, (a, b) in host.items():
        a, b = np.asarray(a), np.asarray(b)
        assert a.shape == b.shape and a.dtype == b.dtype, (case.name, key)
        assert a.tobytes() != b.tobytes(), f"{case.name}: buffer {key!r} is the same in both data sets"
    counts = [k for k in host if k in ("lengths", "frames", "counts")]
    assert bool(counts) == (case.ragged and "recs" not in host), case.name
    for k in counts:
        one = host[k][1]
        assert one.dtype == np.int64 and one[0] == one.max() and one[1] == one.min() and len(np.unique(one)) >= 3, (case.name, one)
        assert (host[k][0] != one).all(), case.name
