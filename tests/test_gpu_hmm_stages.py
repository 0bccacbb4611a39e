"""The HMM stages on the device (csrc/chain_hmm.h: forward, backward, transition_adjoint) against the plain-C restatement of their order
contract (tests/fixtures/hmm_reference.c through tests/hmm_reference.py), tolerance zero: every output element of every chain has the
restatement's bits, at one, two and four waves per chain, in LDS and in device memory.  The shapes and their thinning rule:
``hmm_reference.hmm_shapes``; one case per probe has logE of magnitude -2000, one an impossible state (a column of -inf)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import chain_stage_probes as P  # noqa: E402
import hmm_reference as H  # noqa: E402

pytestmark = pytest.mark.gpu


def same_bits(a, b):
    """equal as bit patterns (so +0.0 is not -0.0), a NaN equal to any NaN — the rule of test_gpu_chain_stages.py"""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(a.view(np.uint64)[~na], b.view(np.uint64)[~nb])


_clean = {}


def clean_run(W):
    if W not in _clean:     # (one probe's outputs at a time)
        _clean.clear()
        _clean[W] = H.probe(W).run(P.clean_points())
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
def test_hmm_stages_have_the_bits_of_the_restatement(hip, W):
    probe = H.probe(W)
    names = " ".join(c.name for c in probe.cases)
    assert "logE~-2000" in names and "-inf column" in names and {c.mem for c in probe.cases} == {"dev", "lds"}
    out = clean_run(W)
    points = P.clean_points()
    bad = mismatches(probe, out, points, range(P.N_CHAINS))
    assert not bad, f"{len(bad)} of {len(probe.cases)} cases:\n" + "\n".join(bad[:20])
    for c in probe.cases:       # finite everywhere (an impossible state is a zero, not a NaN); m of the -inf column case is finite too
        assert np.isfinite(probe.got(out, c, 3)).all(), c.name
    # the chains of one launch computed different numbers (the scale), so a chain that read its neighbour's scratch shows
    assert not np.array_equal(out[1], out[2])


@pytest.mark.parametrize("W,value", [(W, v) for W in (1, 2, 4) for v in (np.nan, np.inf, -np.inf)])
def test_a_poisoned_series_stays_in_its_series_and_chain(hip, W, value):
    """One chain of the launch gets ``value`` in place of one whole series of logE (NaN; +inf; -inf: every state impossible at every
    step).  Every other chain — the three of the same workgroup at one wave per chain among them — keeps the bits of the clean run;
    in the chain itself the other series keep theirs, the poisoned series is NaN from its first step on, the adjoints of P and pi —
    sums over every series — are NaN, and all of it has the restatement's bits."""
    probe = H.probe(W)
    clean = clean_run(W)
    points = P.poisoned_points(value)
    out = probe.run(points)
    me = P.POISONED_CHAIN
    others = [c for c in range(P.N_CHAINS) if c != me]
    assert same_bits(out[others], clean[others])
    bad = mismatches(probe, out, points, [me])
    assert not bad, "\n".join(bad[:20])
    for c in probe.cases:
        r = c.poison[0]
        got, was = H.split(c, probe.got(out, c, me)), H.split(c, probe.got(clean, c, me))
        for g, w_ in zip(got[:5], was[:5]):      # alpha, c, m, beta, w: per series
            keep = np.ones(g.shape[0], bool)
            keep[r] = False
            assert same_bits(g[keep], w_[keep]), c.name
        assert np.isnan(got[0][r]).all() and np.isnan(got[1][r]).all() and np.isnan(got[4][r]).all(), c.name
        assert np.isnan(got[6]).all(), c.name      # pibar sums w_0 of every series
