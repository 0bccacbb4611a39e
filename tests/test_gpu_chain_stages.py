"""The chain stages on the device (csrc/chain_scan.h, chain_matvec.h, chain_linalg.h) against the CPU restatement of their order contracts
(oracle/nuts_oracle.cpp: oracle_chain_*), tolerance zero: every output element of every chain has the oracle's bits.  The routines are
reached through probe densities (tests/chain_stage_probes.py: the shapes, the thinning rules, where the outputs go).

What no device test catches, here or in test_gpu_scan.py: a scan that uses ONE set of wave totals instead of two in turn.  The second
set guards against a wave that still reads a group's totals while another one, a whole group further, overwrites them; rows of more
than 8 * 64 W elements run that code at W = 2 and 4, but the lag it needs — the loads, six DPP steps and LDS writes of a group against
eight LDS reads — is not something the inputs of a test can bring about.  Tried twice with the flip of the set removed: once all of
this file passed, once two of the containment cases at W = 2 differed between two launches — the race fires by chance, a test cannot
count on it.  The alternation is pinned on the source text instead: tests/test_chain_stages_cpu.py::test_scan_wave_totals_use_two_sets_in_turn."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import chain_stage_probes as P  # noqa: E402

import nutpie_amd  # noqa: E402

pytestmark = pytest.mark.gpu


def same_bits(a, b):
    """equal as bit patterns (so +0.0 is not -0.0), a NaN equal to any NaN"""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(a.view(np.uint64)[~na], b.view(np.uint64)[~nb])


_clean = {}


def clean_run(family, W):
    if (family, W) not in _clean:     # (one probe's outputs at a time: they are up to 450 MB)
        _clean.clear()
        _clean[family, W] = P.probe(family, W).run(P.clean_points())
    return _clean[family, W]


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


@pytest.mark.parametrize("family,W", P.PROBES)
def test_device_stage_has_the_bits_of_the_restatement(hip, oracle, family, W):
    probe = P.probe(family, W)
    out = clean_run(family, W)
    points = P.clean_points()
    assert np.isfinite(out).all()
    bad = mismatches(probe, out, points, range(P.N_CHAINS))
    assert not bad, f"{len(bad)} of {len(probe.cases)} cases:\n" + "\n".join(bad[:20])
    # the chains of one launch computed different numbers (the scale), so a chain that read its neighbour's scratch shows
    assert not np.array_equal(out[1], out[2])


POISON = {"scan": [np.nan, np.inf], "matvec": [np.nan, -np.inf], "linalg": [-0.0, 0.0, np.nan, np.inf, 5e-324]}


@pytest.mark.parametrize("family,W,value", [(f, W, v) for f, W in P.PROBES for v in POISON[f]])
def test_non_finite_values_stay_in_their_chain(hip, oracle, family, W, value):
    """One chain of the launch gets ``value`` in place of an element of b (scan), a row of B / G (products), a pivot (Cholesky) or an
    element of the right-hand side (substitutions): every other chain — the three of the same workgroup at one wave per chain among
    them — keeps the bits of the clean run; in the chain itself what does not depend on the element keeps them too, what depends on
    it is non-finite, and all of it has the oracle's bits."""
    probe = P.probe(family, W)
    clean = clean_run(family, W)
    points = P.poisoned_points(value)
    out = probe.run(points)
    me = P.POISONED_CHAIN
    others = [c for c in range(P.N_CHAINS) if c != me]
    assert same_bits(out[others], clean[others])
    bad = mismatches(probe, out, points, [me])
    assert not bad, "\n".join(bad[:20])
    for c in probe.cases:
        got, was = probe.got(out, c, me), probe.got(clean, c, me)
        if family == "scan":
            R = c.p1.shape[0]
            T = c.p1.size // R
            got, was = got.reshape(R, T), was.reshape(R, T)
            r, t = divmod(c.poison[0], T)
            rev = "rev=True" in c.name
            keep = np.ones((R, T), bool)     # forward: the row from t on depends on element t; reversed: the row up to t
            if rev:
                keep[r, :t + 1] = False
            else:
                keep[r, t:] = False
            assert same_bits(got[keep], was[keep]), c.name
            assert not np.isfinite(got[~keep]).any(), c.name
        elif family == "matvec":
            assert not np.isfinite(got).any(), c.name
        elif c.name.startswith("cholesky diagonal") and value == 5e-324:
            K = c.p1.shape[0]                                     # a subnormal positive pivot factors
            assert np.isfinite(got).all() and got[c.poison[0]] == np.sqrt(5e-324) and np.count_nonzero(got) == K, c.name
        elif c.name.startswith("cholesky K=") or c.name.startswith("cholesky diagonal"):
            # -0.0, +0.0, NaN, +inf — and the smallest subnormal where earlier columns are subtracted from it (K // 2 >= 1): not a
            # positive finite pivot, all of L is NaN
            if value != 5e-324 or c.p1.shape[0] > 1:
                assert np.isnan(got).all(), c.name


def test_forward_scan_in_the_expand_step(hip, oracle):
    """``nphip_expand`` is a separate instantiation of the routine, launched by the engine over the stored draws."""
    model, a = P.expand_probe()
    tr = nutpie_amd.sample(model, chains=8, tune=30, draws=12, seed=4, progress_bar=False)
    x, path = tr.posterior.x.values.reshape(-1, P.EXPAND_T), tr.posterior.path.values.reshape(-1, P.EXPAND_T)
    assert len(x) == 8 * 12 and np.isfinite(path).all()
    for row in range(len(x)):
        assert same_bits(path[row], oracle.chain_scan(x[row], a, 0.5, waves=1)), row
