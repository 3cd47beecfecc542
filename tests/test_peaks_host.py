"""CPU: the drop-in surface of the peak search -- MinMaxFinder's signatures as the reference declares them
(script/calc.py:651-686), the exports, and find_peaks_batch's argument checks.  No GPU compute is called here."""
import inspect
import os
import re

import numpy as np
import pytest

import modulation_mfcc_amd
from conftest import ROOT
from modulation_mfcc_amd import calc


def test_exports():
    for name in ("find_peaks_batch", "peaks_to_list", "MinMaxFinder"):
        assert name in calc.__all__
        assert getattr(modulation_mfcc_amd, name) is getattr(calc, name)
    assert "MinMaxFinder" in calc.__doc__


def test_minmaxfinder_signatures():
    # script/calc.py:652, :664, :676
    want = {"find_in_interval": ["self", "times", "values", "interval"],
            "analyse_minimum": ["self", "x", "y", "interval"],
            "analyse_maximum": ["self", "x", "y", "interval"]}
    for name, params in want.items():
        sig = inspect.signature(getattr(calc.MinMaxFinder, name))
        assert list(sig.parameters) == params
        assert all(p.default is inspect.Parameter.empty and p.kind is inspect.Parameter.POSITIONAL_OR_KEYWORD
                   for p in sig.parameters.values())


def test_find_peaks_batch_signature():
    sig = inspect.signature(calc.find_peaks_batch)
    assert list(sig.parameters) == ["x", "negate", "height", "threshold", "prominence", "lo", "hi"]
    assert all(p.kind is inspect.Parameter.KEYWORD_ONLY for n, p in sig.parameters.items() if n != "x")
    assert sig.parameters["negate"].default is False
    assert all(sig.parameters[k].default is None for k in ("height", "threshold", "prominence", "lo", "hi"))


def test_find_peaks_batch_rejects_host_arrays_and_wrong_dtypes():
    import torch
    for bad in (np.zeros(8), [0.0, 1.0, 0.0], torch.zeros(8, dtype=torch.float64), torch.zeros(8, dtype=torch.int32),
                torch.zeros((2, 8), dtype=torch.float16)):
        with pytest.raises(TypeError):
            calc.find_peaks_batch(bad)


def test_no_interval_needs_no_device(capsys):
    f = calc.MinMaxFinder()
    assert f.analyse_maximum([0.0, 1.0], [1.0, 2.0], None) == ([], [])
    assert f.analyse_minimum([0.0, 1.0], [1.0, 2.0], None) == ([], [])
    assert capsys.readouterr().out == "No interval specified.\n" * 2
    t, v = f.find_in_interval([0.0, 1.0, 2.0, 3.0], [5, 6, 7, 8], (1.0, 2.0))
    assert isinstance(t, np.ndarray) and t.tolist() == [1.0, 2.0] and v.tolist() == [6, 7]
    t, v = f.find_in_interval([0.0, 1.0, 2.0], [5, 6], (0.0, 9.0))            # pairs: the shorter one decides
    assert t.tolist() == [0.0, 1.0] and v.tolist() == [5, 6]
    t, v = f.find_in_interval([], [], (0.0, 9.0))
    assert isinstance(t, np.ndarray) and t.size == 0 and v.size == 0


def test_segment_length_matches_the_kernels():
    src = open(os.path.join(ROOT, "modulation_mfcc_amd", "csrc", "mm_peaks.hip")).read()
    threads = int(re.search(r"constexpr int kPkThreads = (\d+);", src).group(1))
    per = int(re.search(r"constexpr int kPkPer = (\d+);", src).group(1))
    assert "constexpr int kPkSeg = kPkThreads * kPkPer;" in src
    assert calc.FIND_PEAKS_SEGMENT == threads * per


def test_condition_intervals():
    import math
    assert calc._peak_interval("height", 2) == [2.0, math.inf]
    assert calc._peak_interval("height", (None, 3.5)) == [-math.inf, 3.5]
    assert calc._peak_interval("height", (None, None)) == [-math.inf, math.inf]
    with pytest.raises(TypeError):
        calc._peak_interval("height", np.zeros(4))
    with pytest.raises(ValueError):
        calc._peak_interval("height", (1.0, math.nan))
