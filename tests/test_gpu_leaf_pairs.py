"""The pair trip of the one-wave register-resident kernels (kernels.hip: Machine::leaf_reg with pair_first): the two leaves of a
level-0 pair taken in one pass, against the oracle and against the same library with ``no_leaf_pairs``.

Every draw and statistic stays bit-identical: a pair computes, per value, what two single leaves compute."""
import ctypes

import numpy as np
import pytest

from nutpie_amd.gaussian import ar1_gaussian
from tests.conftest import FLOAT_STATS, INT_STATS, assert_trace_equal
from tests.test_gpu_parity import DIV_KEYS, oracle_settings, run_engine

KW = dict(chains=4, tune=60, draws=15)
DIMS = [200, 500, 1000]   # 2, 4 and 8 chunks per lane

_want = {}


def _oracle(oracle, dim, seed, **settings):
    # one oracle run per (dim, seed, settings), shared by the cases that compare against it (never modified)
    key = (dim, seed, tuple(sorted(settings.items())))
    if key not in _want:
        m = ar1_gaussian(dim)
        _want[key] = oracle.sample_tridiag(oracle_settings(oracle, W=1, seed=seed, **KW, **settings), m.diag, m.offdiag)
    return _want[key]


def _engine(hip, dim, seed, launch, **settings):
    m = ar1_gaussian(dim)
    got, W = run_engine(hip, hip.TridiagGaussianModel(m.diag, m.offdiag), seed=seed, launch=launch, **KW, **settings)
    assert W == 1
    return got


# evals_per_launch = 1: no pair is ever taken; 3 and 7: every launch boundary changes the parity a trip starts at
@pytest.mark.gpu
@pytest.mark.parametrize("evals", [0, 1, 2, 3, 7])
@pytest.mark.parametrize("dim", DIMS)
def test_pairs_bit_identical_to_the_oracle(hip, oracle, dim, evals):
    got = _engine(hip, dim, dim + 7, dict(evals_per_launch=evals) if evals else {})
    assert_trace_equal(got, _oracle(oracle, dim, dim + 7))


@pytest.mark.gpu
@pytest.mark.parametrize("evals", [0, 5])
@pytest.mark.parametrize("dim", DIMS)
def test_divergences_inside_pairs(hip, oracle, dim, evals):
    # n_steps counts the failed leapfrog.  The doublings before the failing one hold 1 + 2 + 4 + ... leaves, an odd number, so an even
    # n_steps is a failed odd leaf of its doubling, the first of a pair (A: the draw must end as if B had never been taken), and an odd
    # n_steps > 1 a failed second one (B).  The inputs are chosen so that the oracle alone has many of both.
    settings = dict(max_energy_error=0.6, store_divergences=True)
    want = _oracle(oracle, dim, dim + 31, **settings)
    wdiv = np.asarray(want.stats["diverging"]).astype(bool)
    wn = np.asarray(want.stats["n_steps"]).astype(np.int64)
    n_a = int((wdiv & (wn >= 2) & (wn % 2 == 0)).sum()), int((wdiv & (wn >= 2) & (wn % 2 == 1)).sum())
    print(f"dim {dim}: diverging draws with the failed leaf an A: {n_a[0]}, a B: {n_a[1]}")
    assert n_a[0] >= 10 and n_a[1] >= 10, "the case is meant to diverge in both leaves of pairs"
    got = _engine(hip, dim, dim + 31, dict(evals_per_launch=evals) if evals else {}, **settings)
    assert_trace_equal(got, want)
    div = np.asarray(got.stats["diverging"]).astype(bool)
    for k in DIV_KEYS:
        a, b = got.stats[k], want.stats[k]
        assert np.array_equal(np.isnan(a), np.isnan(b)), k
        assert np.array_equal(a[~np.isnan(a)], b[~np.isnan(b)]), k
        assert np.all(np.isnan(a[~div])), k
    assert np.all(np.isfinite(got.stats["divergence_start"][div]))


@pytest.mark.gpu
@pytest.mark.parametrize("settings", [
    dict(maxdepth=3),
    dict(mindepth=3),
    dict(check_turning=False, maxdepth=4),
    dict(maxdepth=12, target_accept=0.95),
], ids=["maxdepth3", "mindepth3", "no-turning-maxdepth4", "deep-trees"])
def test_pairs_under_awkward_settings(hip, oracle, settings):
    got = _engine(hip, 1000, 1007, dict(evals_per_launch=3), **settings)
    assert_trace_equal(got, _oracle(oracle, 1000, 1007, **settings))


@pytest.mark.gpu
def test_launch_accounting_with_and_without_pairs(hip):
    # a chain does exactly as many counted leapfrogs per launch with pairs as without: a pair is admitted only with budget for both
    # leaves, and a draw that ends at the first leaf gives the second one's unit back
    m = ar1_gaussian(1000)

    def start(no_pairs):
        s = hip.PyNutsSettings.Diag(1038)
        s.update(num_tune=KW["tune"], num_draws=KW["draws"], num_chains=KW["chains"], max_energy_error=0.6)
        return hip.PySampler(s, hip.TridiagGaussianModel(m.diag, m.offdiag), manual=True, evals_per_launch=6, no_leaf_pairs=no_pairs)

    a, b = start(False), start(True)
    for launch in range(40):
        a.step(1)
        b.step(1)
        pa, pb = a.progress(), b.progress()
        assert [p.total_num_steps for p in pa] == [p.total_num_steps for p in pb], launch
        assert [p.finished_draws for p in pa] == [p.finished_draws for p in pb], launch
    assert sum(p.total_num_steps for p in pa) > 0
    while not a.step(64)[0]:
        pass
    while not b.step(64)[0]:
        pass
    ta, tb = a.take_results(), b.take_results()
    assert np.array_equal(ta.draws, tb.draws)
    for k in INT_STATS + FLOAT_STATS:
        assert np.array_equal(np.asarray(ta.stats[k]), np.asarray(tb.stats[k])), k
    assert np.asarray(ta.stats["diverging"]).sum() > 0


# ------------------------------------------------------------------------------------ without a GPU
def test_launch_struct_keeps_its_size():
    from nutpie_amd import _lib

    L = _lib.lib()
    assert L.nphip_abi_struct_size(0) == 96 == ctypes.sizeof(_lib._Launch)   # (no_leaf_pairs took the reserved slot)


def test_launch_defaults_leave_pairs_on():
    from nutpie_amd import _lib

    la = _lib._Launch()
    ctypes.memset(ctypes.byref(la), 0xFF, ctypes.sizeof(la))
    _lib.lib().nphip_launch_defaults(ctypes.byref(la))
    assert la.no_leaf_pairs == 0
