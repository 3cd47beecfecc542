"""The shared-runs form of the fused kernels' mel run table (mm_build_mel_runs_shared) on the host: every
run once, the weights of every filter exactly those of the dense mel matrix, one producer per consumer, and the
overlapping-runs table (mm_build_mel_runs) exactly what its documented rule gives."""
import numpy as np
import pytest

from modulation_mfcc_amd.plan import MfccConfig

CONSUMER, PRODUCER = 1 << 16, 1 << 17

C16K = dict(sr=16000, n_fft=512, win_length=400, hop_length=160, n_mels=40, n_mfcc=13, fmin=100.0, fmax=8000.0)
PLANS = {
    "c16k": C16K,
    "mel64": dict(C16K, n_mels=64),
    "mel13": dict(C16K, n_mels=13),           # fewer filters than waves: empty parts
    "mel16": dict(C16K, n_mels=16),           # one filter per part (equal cuts)
}
CASES = [(name, weighted) for name in PLANS for weighted in (False, True)]


@pytest.fixture(scope="module", params=CASES, ids=lambda c: "%s-%s" % (c[0], "fused-cuts" if c[1] else "equal-cuts"))
def table(request):
    name, weighted = request.param
    cfg = MfccConfig(**PLANS[name])
    hdr, grp, part = cfg.mel_runs_shared(16, weighted=weighted)
    return cfg, hdr, grp, part


def _parts(part):
    """(wave, run0, run1, m0, m1, flags) of the parts that have a filter."""
    out = []
    for w, (r0, r1, m0, m1f) in enumerate(part.tolist()):
        m1, flags = m1f & 0xFFFF, m1f & ~0xFFFF
        if m1 > m0:
            out.append((w, r0, r1, m0, m1, flags))
        else:
            assert r0 == r1 and flags == 0, "an empty part has no runs and no hand-over"
    return out


def test_every_run_appears_exactly_once(table):
    cfg, hdr, grp, part = table
    weighted = [int(d) for (k4, ng, go, d) in hdr.tolist() if ng > 0 and np.any(grp[go:go + ng] != 0)]
    assert sorted(weighted) == sorted(set(weighted)), "a run with a weight is listed twice"
    assert hdr[:, 3].tolist() == list(range(-1, cfg.n_mels)), "runs -1 .. n_mels-1, in order, once"
    # the parts tile the run list and the filters
    ps = _parts(part)
    assert ps[0][1] == 0 and ps[-1][2] == len(hdr) and all(a[2] == b[1] for a, b in zip(ps, ps[1:]))
    assert ps[0][3] == 0 and ps[-1][4] == cfg.n_mels and all(a[4] == b[3] for a, b in zip(ps, ps[1:]))
    for i, (w, r0, r1, m0, m1, flags) in enumerate(ps):
        first_run = m0 - 1 if i == 0 else m0
        assert hdr[r0:r1, 3].tolist() == list(range(first_run, m1)), (w, m0, m1)
    # the groups are laid out back to back
    assert hdr[0, 2] == 0 and (hdr[1:, 2] == hdr[:-1, 2] + hdr[:-1, 1]).all() and hdr[-1, 2] + hdr[-1, 1] == len(grp)


def test_gathered_weights_equal_the_dense_matrix(table):
    cfg, hdr, grp, part = table
    W = cfg.mel_filterbank()
    n_pad = 4 * ((cfg.n_bins + 3) // 4)
    R = np.zeros((cfg.n_mels, n_pad), dtype=np.float32)
    for (k4, ng, go, d) in hdr.tolist():
        assert k4 % 4 == 0 and k4 + 4 * ng <= n_pad
        for g in range(ng):
            lo, hi = grp[go + g, :4], grp[go + g, 4:]
            if d >= 0:
                assert not ((R[d, k4 + 4 * g:k4 + 4 * g + 4] != 0) & (lo != 0)).any(), "a weight is listed twice"
                R[d, k4 + 4 * g:k4 + 4 * g + 4] += lo
            else:
                assert not (lo != 0).any(), "run -1 has no falling filter"
            if d + 1 < cfg.n_mels:
                assert not ((R[d + 1, k4 + 4 * g:k4 + 4 * g + 4] != 0) & (hi != 0)).any(), "a weight is listed twice"
                R[d + 1, k4 + 4 * g:k4 + 4 * g + 4] += hi
            else:
                assert not (hi != 0).any(), "the last run has no rising filter"
    np.testing.assert_array_equal(R[:, :cfg.n_bins], W)
    assert not R[:, cfg.n_bins:].any()


def test_every_consumer_has_one_earlier_producer(table):
    cfg, hdr, grp, part = table
    ps = _parts(part)
    for i, (w, r0, r1, m0, m1, flags) in enumerate(ps):
        assert bool(flags & CONSUMER) == (i > 0), "every part but the first takes its first filter's rising half"
        assert bool(flags & PRODUCER) == (i + 1 < len(ps)), "every part but the last hands over"
        assert flags & ~(CONSUMER | PRODUCER) == 0
    for i, (w, r0, r1, m0, m1, flags) in enumerate(ps):
        if not flags & CONSUMER:
            continue
        producers = [q for q in ps if (q[5] & PRODUCER) and q[4] == m0]
        assert len(producers) == 1 and producers[0][0] < w, "one producer, an earlier part"
        # ... whose last run is run m0 - 1 with the rising weights of filter m0 in it
        assert hdr[producers[0][2] - 1, 3] == m0 - 1 and hdr[r0, 3] == m0


def test_a_walk_of_the_table_gives_the_mel_energies(table):
    """Phase B as the kernel runs it: a consumer holds its first run's sum, the producer's second sum completes it."""
    cfg, hdr, grp, part = table
    W = cfg.mel_filterbank().astype(np.float64)
    P = np.zeros(4 * ((cfg.n_bins + 3) // 4))
    P[:cfg.n_bins] = np.random.default_rng(5).uniform(0.0, 2.0, cfg.n_bins)
    out = np.full(cfg.n_mels, np.nan)
    handed, held = {}, {}
    for (w, r0, r1, m0, m1, flags) in _parts(part):
        carry = 0.0
        for r in range(r0, r1):
            k4, ng, go, dd = hdr[r].tolist()
            sa = sum(float(grp[go + g, :4].astype(np.float64) @ P[k4 + 4 * g:k4 + 4 * g + 4]) for g in range(ng))
            sb = sum(float(grp[go + g, 4:].astype(np.float64) @ P[k4 + 4 * g:k4 + 4 * g + 4]) for g in range(ng))
            if (flags & CONSUMER) and r == r0:
                held[m0] = sa
            elif dd >= m0:
                assert np.isnan(out[dd]); out[dd] = carry + sa
            carry = sb
        if flags & PRODUCER:
            handed[m1] = carry
    assert sorted(handed) == sorted(held)
    for m in held:
        assert np.isnan(out[m]); out[m] = handed[m] + held[m]
    assert not np.isnan(out).any()
    np.testing.assert_allclose(out, W @ P[:cfg.n_bins], rtol=1e-12, atol=1e-15)


@pytest.mark.parametrize("name", sorted(PLANS))
@pytest.mark.parametrize("n_waves", [8, 16])
def test_overlapping_runs_table_is_unchanged(name, n_waves):
    """mm_build_mel_runs against its rule, written out here: per part the runs m0-1 .. m1-1, groups over every bin of the
    run that has a weight, the first run's falling and the last run's rising weights zeroed."""
    cfg = MfccConfig(**PLANS[name])
    wlo, whi, d, spart = cfg.mel_sweep(n_waves)
    hdr, grp, part = cfg.mel_runs(n_waves)
    want_hdr, want_grp, want_part = [], [], []
    for (kb, ke, m0, m1) in spart.tolist():
        r0 = len(want_hdr)
        for dd in range(m0 - 1, m1) if m1 > m0 else ():
            ks = [k for k in range(cfg.n_bins) if d[k] == dd and (wlo[k] != 0 or whi[k] != 0)]
            g0, g1 = (ks[0] // 4, (ks[-1] + 1 + 3) // 4) if ks else (0, 0)
            want_hdr.append([4 * g0, g1 - g0, len(want_grp), dd])
            for g in range(g0, g1):
                row = np.zeros(8, dtype=np.float32)
                for u in range(4):
                    k = 4 * g + u
                    if ks and ks[0] <= k <= ks[-1] and d[k] == dd:
                        row[u] = 0.0 if dd == m0 - 1 else wlo[k]
                        row[4 + u] = 0.0 if dd == m1 - 1 else whi[k]
                want_grp.append(row)
        want_part.append([r0, len(want_hdr), m0, m1])
    np.testing.assert_array_equal(hdr, np.array(want_hdr, dtype=np.int32).reshape(-1, 4))
    np.testing.assert_array_equal(grp, np.array(want_grp, dtype=np.float32).reshape(-1, 8))
    np.testing.assert_array_equal(part, np.array(want_part, dtype=np.int32))


def test_shared_table_is_smaller_by_the_overlap():
    """c16k: 56 runs walked by the overlapping form, 41 distinct ones."""
    cfg = MfccConfig(**C16K)
    hdr_o, grp_o, _ = cfg.mel_runs(16)
    hdr_s, grp_s, _ = cfg.mel_runs_shared(16)
    assert len(hdr_o) == 56 and len(hdr_s) == 41
    assert len(grp_s) < len(grp_o)
