"""The yardstick of the device IIR tests (tests/sos_oracle.py) checked on the host: it is scipy.signal.sosfiltfilt where
scipy is accurate, it is sharper than scipy where scipy is not, and its padlen is scipy's.  No GPU."""
import re

import numpy as np
import pytest
import scipy.signal

import sos_oracle as Q

DESIGNS = Q.foreign_designs()


def _scipy_padlen(sos):
    """The number in scipy's own 'greater than padlen' message."""
    with pytest.raises(ValueError, match="greater than padlen") as e:
        scipy.signal.sosfiltfilt(sos, np.zeros(3))
    return int(re.search(r"which is (\d+)", str(e.value)).group(1))


@pytest.mark.parametrize("name", sorted(DESIGNS))
def test_padlen_is_scipys(name):
    sos = DESIGNS[name]
    pad = Q.padlen_of(sos)
    assert pad == _scipy_padlen(sos)
    x = np.arange(pad, dtype=np.float64)
    with pytest.raises(ValueError, match=f"greater than padlen, which is {pad}"):
        Q.sosfiltfilt_ext(sos, x)
    assert Q.sosfiltfilt_ext(sos, np.arange(pad + 1, dtype=np.float64)).shape == (pad + 1,)


def test_padlen_takes_the_smaller_zero_count():
    # one b2 == 0 and one a2 == 0: ntaps 5 - 1; two b2 == 0, no a2 == 0: 5 - 0 -- `max` instead of `min` gives 4 | 3
    assert Q.padlen_of(DESIGNS["b2zero_a2zero"]) == 12 and Q.padlen_of(DESIGNS["two_b2zero"]) == 15
    for order in (1, 2, 3, 5, 8):
        for kind in ("low", "high"):
            sos = scipy.signal.butter(order, 0.2, kind, output="sos")
            assert Q.padlen_of(sos) == _scipy_padlen(sos) == 3 * (order + 1)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("name", sorted(DESIGNS))
def test_oracle_is_scipy_where_scipy_is_accurate(name, dtype):
    """Poles no closer than 0.97 to the unit circle: float64 and extended precision agree to 1e-13 of the maximum
    (the Bessel band-pass removes the envelope's large slow part, so its output is small against its states: scipy's own
    rounding is 1 - 3e-13 of the output's maximum there, the figure of its row in docs/experiments.md -- bound 3e-13)."""
    sos = DESIGNS[name]
    pad = Q.padlen_of(sos)
    rng = np.random.default_rng(21)
    bound = 3e-13 if name == "bessel2_band" else 1e-13
    for n in (pad + 1, 1088 - 2 * pad, 2000):
        x = Q.envelope_rows(rng, 2, n, dtype)
        want = scipy.signal.sosfiltfilt(sos, x, axis=1)
        got = Q.sosfiltfilt_ext(sos, x)
        assert got.dtype == want.dtype == np.float64 and got.shape == want.shape
        assert Q.rel_err(want, got) <= bound, (n, Q.rel_err(want, got))
        np.testing.assert_array_equal(Q.sosfiltfilt_ext(sos, x[1]), got[1])     # a single curve: the same numbers
    if dtype == np.float32 and name != "gain_half":
        # the extension is formed in float32: extending the upcast curve instead moves the result by ~1e-8 near the ends
        assert Q.rel_err(Q.sosfiltfilt_ext(sos, x.astype(np.float64)), got) > 1e-10


# scipy 1.15 float64 against an 80-bit sequential restatement, relative to max|y| (docs/experiments.md, "The IIR
# filter near the unit circle"): filter, n, scipy's error there
_TABLE = [((6, 1.5e-3), 12000, 2.8e-12), ((6, 5e-4), 12000, 3.9e-11), ((8, 5e-4), 12000, 2.2e-11),
          ((6, 2.7e-4), 6000, 8.6e-11), ((4, 1e-4), 12000, 6.9e-10), ((2, 2e-5), 6000, 6.3e-8)]


def test_oracle_is_sharper_than_scipy_near_the_unit_circle():
    """scipy's float64 error against the oracle reproduces the measured table to its order of magnitude and grows as the
    cut-off shrinks: were the oracle no sharper than scipy the differences would not follow the conditioning (and an
    oracle in plain float64 would give 0 at every point)."""
    rng = np.random.default_rng(0)
    errs = []
    for (order, wn), n, table in _TABLE:
        sos = scipy.signal.butter(order, wn, output="sos")
        x = Q.envelope_rows(rng, 1, n)[0]
        e = Q.rel_err(scipy.signal.sosfiltfilt(sos, x), Q.sosfiltfilt_ext(sos, x))
        errs.append(e)
        assert table / 10 <= e <= table * 10, (order, wn, e, table)
    by_wn = {wn: e for ((_, wn), _, _), e in zip(_TABLE, errs)}
    assert by_wn[1.5e-3] < by_wn[2.7e-4] < by_wn[1e-4] < by_wn[2e-5]
    # the extended result rounds to float64 once: the float64 oracle output and the long double one differ by <= 1/2 ulp
    sos = scipy.signal.butter(6, 5e-4, output="sos")
    x = Q.envelope_rows(rng, 1, 3000)[0]
    ld = Q.sosfiltfilt_ext_ld(sos, x)
    assert ld.dtype == np.longdouble and Q.rel_err(Q.sosfiltfilt_ext(sos, x), ld) <= 2.0 ** -53


def test_oracle_refuses_what_scipy_refuses():
    sos = scipy.signal.butter(4, 0.2, output="sos")
    x = np.zeros(100)
    for bad in (sos * 2.0, sos.ravel(), sos[None], sos[:, :5]):
        with pytest.raises(ValueError) as es:
            scipy.signal.sosfiltfilt(bad, x)
        with pytest.raises(ValueError) as eo:
            Q.sosfiltfilt_ext(bad, x)
        assert str(eo.value) == str(es.value)


def test_package_validation_is_scipys():
    """filters.sos_sections -- what sosfiltfilt_batch, applyFilter(coeffs=) and MfccPlan.mfcc_change run before they launch
    anything -- raises scipy's ValueErrors with scipy's messages."""
    from modulation_mfcc_amd.filters import sos_sections
    sos = scipy.signal.butter(4, 0.2, output="sos")
    np.testing.assert_array_equal(sos_sections(sos), sos)
    np.testing.assert_array_equal(sos_sections(sos[0]), sos[:1])          # one section as a 6-vector: scipy's atleast_2d
    np.testing.assert_array_equal(sos_sections(sos.tolist()), sos)
    for bad in (sos * 2.0, sos.ravel(), sos[None], sos[:, :5]):
        with pytest.raises(ValueError) as es:
            scipy.signal.sosfiltfilt(bad, np.zeros(100))
        with pytest.raises(ValueError) as ep:
            sos_sections(bad)
        assert str(ep.value) == str(es.value)
    with pytest.raises(ValueError, match=re.escape("sos[:, 3] should be all ones")):
        sos_sections(sos * 2.0)
