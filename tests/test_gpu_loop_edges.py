"""The wave-wide loops that ``_Gen.loop`` writes, on the GPU, at the edges of their shape decisions (tests/loop_edge_models.py): every
case within the rounding bound that tests/loop_edge_reference.py derives from a 50-digit restatement, a chain's bits independent of its
neighbours and of where it sits in a workgroup, a poisoned chain or observation contained, ``with_data`` on the caps of other data, and
the resident form against the batched one.  Libraries are prebuilt (tests/prebuild_loop_edge_cache.py)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import loop_edge_models as M  # noqa: E402
import loop_edge_reference as R  # noqa: E402

import nutpie_amd  # noqa: E402

pytestmark = pytest.mark.gpu


def _table(W):
    """the specialised cases of W (the table; at W = 1 the spilled one too) with their compiled models"""
    return [(c, c.compile()) for c in list(M.cases(W)) + ([M.spill_case()] if W == 1 else [])]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


@pytest.mark.parametrize("W", M.WAVES)
def test_every_case_is_within_the_bound_of_the_reference(hip, W):
    """five positions — a full workgroup of four one-wave chains and a ragged one — per case: logp and every gradient element within
    (n - 1 + c) 2^-53 M of the 50-digit value"""
    worst, failed = 0.0, []
    for c, m in _table(W):
        lp, g = m.logp_and_grad(c.pos)
        ratio = R.check(c.variant, c.G, c.data, c.pos, lp, g)
        print(f"{c.name}: err / bound = {ratio:.3f}")
        worst = max(worst, ratio)
        if not ratio <= 1.0:
            failed.append((c.name, ratio))
    R.record(f"device W={W}", worst)
    assert not failed, failed


@pytest.mark.parametrize("W", M.WAVES)
def test_a_chain_has_the_same_bits_wherever_it_runs(hip, W):
    """alone, in slot 0 and in slot 3 of a workgroup, and in a batch of 37"""
    for c, m in _table(W):
        p = c.pos
        lp1, g1 = m.logp_and_grad(p[:1])
        lp4, g4 = m.logp_and_grad(p[[0, 1, 2, 3]])
        lp3, g3 = m.logp_and_grad(p[[1, 2, 3, 0]])
        rows = np.arange(37) % M.N_POS
        lp37, g37 = m.logp_and_grad(p[rows])
        assert _same(lp1[0], lp4[0]) and _same(g1[0], g4[0]), c.name
        assert _same(lp1[0], lp3[3]) and _same(g1[0], g3[3]), c.name
        for k in np.flatnonzero(rows == 0):
            assert _same(lp1[0], lp37[k]) and _same(g1[0], g37[k]), (c.name, int(k))
        assert _same(lp37[:4], lp4) and _same(g37[1:4], g3[:3]), c.name


@pytest.mark.parametrize("W", M.WAVES)
def test_a_poisoned_chain_leaves_the_others_their_bits(hip, W):
    """NaN, +inf and -inf in a scalar and in a vector element of one chain's position"""
    for c, m in _table(W):
        clean_lp, clean_g = m.logp_and_grad(c.pos)
        others = [0, 1, 3, 4]
        for column in (3, 4 + c.G // 2):
            for poison in (np.nan, np.inf, -np.inf):
                p = c.pos.copy()
                p[2, column] = poison
                lp, g = m.logp_and_grad(p)
                assert _same(lp[others], clean_lp[others]) and _same(g[others], clean_g[others]), (c.name, column, poison)
                assert not np.isfinite(lp[2]) or not np.isfinite(g[2]).all(), (c.name, column, poison)


@pytest.mark.parametrize("W", M.WAVES)
@pytest.mark.parametrize("row", [("2*T+1", "d"), ("4*T+1", "f")])
def test_a_poisoned_observation_stays_in_its_group(hip, W, row):
    """y of one observation of the longest range is NaN: logp, the shared parameters' gradients and that group's element are NaN, every
    other group's element keeps its bits — the capped batch and the reads past a range's end drop values with a select, not a product
    (the short and empty ranges before the long one read its elements)"""
    c = M.case(W, "base", *row)
    m = c.compile()
    clean_lp, clean_g = m.logp_and_grad(c.pos)
    g_long = int(np.argmax(c.counts))
    members = np.flatnonzero(c.data["gi"] == g_long)
    for i in (members[0], members[len(members) // 2], members[-1]):
        y = c.data["y"].copy()
        y[i] = np.nan
        swapped = m.with_data(y=y)
        assert swapped.library_path() == m.library_path()
        lp, g = swapped.logp_and_grad(c.pos)
        assert np.isnan(lp).all() and np.isnan(g[:, :4]).all() and np.isnan(g[:, 4 + g_long]).all()
        keep = np.arange(c.G) != g_long
        assert _same(g[:, 4:][:, keep], clean_g[:, 4:][:, keep]), int(i)
    assert np.isfinite(clean_lp).all() and np.isfinite(clean_g).all()


@pytest.mark.parametrize("W", M.WAVES)
def test_with_data_keeps_the_caps_of_the_old_data_and_stays_exact(hip, W):
    """the specialised form at unchanged lengths: compiled against a longest range of 3 and given ranges of 40 behind a run of empty
    groups (the rest loop takes what is longer than the caps); compiled against ranges of 31, 32, 33 and given one observation per group
    with empty groups (every read past a range's end is dropped).  Same library, within the bound."""
    for with_, given in M.swap_cases(W):
        m = with_.compile()
        swapped = m.with_data(**given.updates())
        assert swapped.library_path() == m.library_path()
        lp, g = swapped.logp_and_grad(given.pos)
        ratio = R.check(given.variant, given.G, given.data, given.pos, lp, g)
        print(f"{with_.name} given {given.profile}: err / bound = {ratio:.3f}")
        assert ratio <= 1.0, (given.name, ratio)


@pytest.mark.parametrize("W", M.WAVES)
@pytest.mark.parametrize("variant", M.VARIANTS)
def test_one_unspecialised_library_takes_every_length_and_profile(hip, W, variant):
    """``specialize=False``: sizes are run-time values; one library per W and variant is given every length of ``obs`` and every profile"""
    base, given = M.sweep(W, variant)
    m = base.compile(specialize=False)
    worst = 0.0
    for c in given:
        swapped = m.with_data(**c.updates())
        assert swapped.library_path() == m.library_path()
        lp, g = swapped.logp_and_grad(c.pos)
        ratio = R.check(c.variant, c.G, c.data, c.pos, lp, g)
        assert ratio <= 1.0, (c.name, ratio)
        worst = max(worst, ratio)
    R.record(f"device W={W} specialize=False {variant}", worst)


@pytest.mark.parametrize("W", [1, 4])
@pytest.mark.parametrize("row", [("T+1", "a"), ("4*T+1", "f")])
def test_resident_and_batched_forms_draw_the_same_bits(hip, W, row):
    """a short job through the resident kernel and through the batched callback of the same library; the reported value on ``group`` from
    the generated expand against the numpy evaluation of the same graph"""
    c = M.case(W, "base", *row)
    kw = dict(chains=5, tune=20, draws=10, seed=11, progress_bar=False, return_raw_trace=True)
    m = c.compile()
    a = nutpie_amd.sample(m, **kw)
    b = nutpie_amd.sample(c.compile(resident=False), **kw)
    assert _same(a.draws, b.draws)
    assert a.expanded is not None and "__flat__" in a.expanded
    got = m._unflatten(a.expanded["__flat__"])
    want = m._expand_draws(a.draws)
    assert got["eff"].shape == want["eff"].shape == (5, 30, c.G)
    for k in want:
        np.testing.assert_allclose(got[k], want[k], rtol=1e-12, atol=1e-13, err_msg=k)
