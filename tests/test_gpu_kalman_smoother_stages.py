"""The Kalman smoother on the device (csrc/kalman_smoother.h: smooth, after csrc/chain_kalman.h: forward) against the plain-C restatement of
its order contract (tests/fixtures/kalman_smoother_reference.c through tests/kalman_smoother_reference.py), tolerance zero: every element
of [F | S] of every chain has the restatement's bits, at one, two and four waves per chain, in LDS and in device memory.  The shapes:
``kalman_reference.kalman_shapes``; one case per probe has a first step that is missing, one a last step that is missing, one ``P0 = 1e8 I``."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import chain_stage_probes as P  # noqa: E402
import kalman_reference as K  # noqa: E402
import kalman_smoother_reference as KS  # noqa: E402

pytestmark = pytest.mark.gpu


def same_bits(a, b):
    """equal as bit patterns (so +0.0 is not -0.0), a NaN equal to any NaN — the rule of test_gpu_kalman_stages.py"""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(a.view(np.uint64)[~na], b.view(np.uint64)[~nb])


_clean = {}


def clean_run(W):
    if W not in _clean:     # (one probe's outputs at a time)
        _clean.clear()
        _clean[W] = KS.probe(W).run(P.clean_points())
    return _clean[W]


def mismatches(probe, out, points, chains):
    bad = []
    for k, c in enumerate(probe.cases):
        for chain in chains:
            want, got = probe.expected(c, points[chain]), probe.got(out, c, chain)
            if not same_bits(got, want):
                diff = np.flatnonzero(~((got == want) & (np.signbit(got) == np.signbit(want)) | (np.isnan(got) & np.isnan(want))))
                bad.append(f"case {k} {c.name} [{c.mem}] chain {chain}: {diff.size} of {want.size} elements differ, first at {diff[0]}: {got[diff[0]]!r} != {want[diff[0]]!r}")
                break
    return bad


@pytest.mark.parametrize("W", [1, 2, 4])
def test_smoother_has_the_bits_of_the_restatement(hip, W):
    probe = KS.probe(W)
    names = " ".join(c.name for c in probe.cases)
    assert "first step missing" in names and "last step missing" in names and "P0=1e8 I" in names and {c.mem for c in probe.cases} == {"dev", "lds"}
    assert {K.shape_of(c)[2] for c in probe.cases} == set(K.KAL_M) and {K.shape_of(c)[1] for c in probe.cases} == set(K.KAL_T)
    out = clean_run(W)
    points = P.clean_points()
    bad = mismatches(probe, out, points, range(P.N_CHAINS))
    assert not bad, f"{len(bad)} of {len(probe.cases)} cases:\n" + "\n".join(bad[:20])
    for c in probe.cases:
        assert np.isfinite(probe.got(out, c, 3)).all(), c.name
    # the chains of one launch computed different numbers (the scale), so a chain that read its neighbour's scratch shows
    assert not np.array_equal(out[1], out[2])


@pytest.mark.parametrize("W,value", [(W, v) for W in (1, 2, 4) for v in (np.nan, np.inf, -np.inf)])
def test_a_poisoned_series_stays_in_its_series_and_chain(hip, W, value):
    """One chain of the launch gets ``value`` in place of one whole series of y.  Every other chain keeps the bits of the clean run; in
    the chain itself the other series keep theirs, and all of it has the restatement's bits.  The series itself: its innovations are
    not finite at the observed steps, so r is not finite from the last observed step down and the smoothed means there are NaN or
    infinite; a series whose steps are all missing never reads y: nothing changes."""
    probe = KS.probe(W)
    clean = clean_run(W)
    points = P.poisoned_points(value)
    out = probe.run(points)
    me = P.POISONED_CHAIN
    others = [c for c in range(P.N_CHAINS) if c != me]
    assert same_bits(out[others], clean[others])
    bad = mismatches(probe, out, points, [me])
    assert not bad, "\n".join(bad[:20])
    checked = 0
    for c in probe.cases:
        r = c.poison[0]
        R, T, m, mask = K.shape_of(c)
        got, was = KS.split(c, probe.got(out, c, me)), KS.split(c, probe.got(clean, c, me))
        keep = np.ones(R, bool)
        keep[r] = False
        for g, w_ in zip(got, was):
            assert same_bits(g[keep], w_[keep]), c.name
        seen = np.ones(T, bool) if mask is None else mask[r] != 0
        if not seen.any():
            assert same_bits(got[5][r], was[5][r]) and same_bits(got[6][r], was[6][r]), c.name
            continue
        assert not np.isfinite(got[3][r][seen]).any(), c.name               # the stored innovations of the observed steps
        last = int(np.flatnonzero(seen)[-1])
        assert not np.isfinite(got[5][r].reshape(T, m)[last]).all(), c.name      # the smoothed mean at the series' last observed step
        checked += 1
    assert checked >= 10
