"""The fixtures the estimator kernel is held to (tests/golden/low_rank_estimator_*.npz, written by tests/golden/make_low_rank_reference.py
from the 50-digit restatement tests/low_rank_reference.py): conditions on their inputs, and a guard against a fixture that has rotted."""
import math

import numpy as np
import pytest

from tests import low_rank_reference as R


@pytest.mark.parametrize("name", R.CASE_NAMES)
def test_fixture_inputs_sit_away_from_every_threshold(name):
    """The kernel decides the rank of the basis on Cholesky pivots and the reference on eigenvalues, and both cut the spectrum at
    ``cutoff`` and at ``k_max`` columns: a case near one of these thresholds would compare two legitimate answers."""
    c, z = R.case(name), R.load(name)
    x, g = R.inputs(c)
    # the stored window is the one the case table describes (to the last bits only under the BLAS threading of the generator)
    assert np.allclose(z["x"], x, rtol=1e-9, atol=1e-9 * np.abs(x).max()) and np.allclose(z["g"], g, rtol=1e-9, atol=1e-9 * np.abs(g).max())
    assert np.array_equal(z["pick"], R.pick_of(c["m"], c["b"]))
    assert (float(z["gamma"]), float(z["cutoff"]), int(z["k_max"])) == (c["gamma"], c["cutoff"], c["k_max"])
    ev = z["gram_ev"]
    assert len(ev) == 2 * c["b"] and ev.max() == 1.0
    assert np.all((ev > 1e-6) | (ev < 1e-13)), ev[(ev <= 1e-6) & (ev >= 1e-13)]
    scores, k, k_max = z["scores"], int(z["k"]), c["k_max"]
    assert len(scores) == int((ev > 1e-10).sum()) and np.all(np.diff(scores) <= 0)
    assert np.abs(scores - math.log(c["cutoff"])).min() >= 5e-3 or len(scores) == 0
    outside = int((scores > math.log(c["cutoff"])).sum())
    assert k == min(outside, k_max)
    if outside > k_max:
        assert scores[k_max - 1] - scores[k_max] >= 1e-2
    assert k >= 1 or name in R.NO_COLUMNS_ALLOWED
    want = {key: z[key] for key in ("dense", "diag", "probe") if key in z}
    assert set(want) == ({"dense"} if c["D"] <= R.DENSE_MAX else {"diag", "probe"})
    assert all(np.isfinite(v).all() for v in want.values())


def test_the_selection_cases_have_to_choose():
    z = R.load("select_40_12_12_kmax16")
    assert int((z["scores"] > math.log(2.0)).sum()) > 16 and int(z["k"]) == 16
    for name in ("select_24_10_10_kmax4", "select_24_10_10_kmax1"):
        z = R.load(name)
        assert int((z["scores"] > math.log(2.0)).sum()) > int(z["k_max"]) == int(z["k"])


@pytest.mark.parametrize("name", R.CASE_NAMES)
def test_fixture_guard_the_numpy_restatement_is_as_far_from_the_reference_as_recorded(name):
    """``err_numpy`` recomputed from the stored inputs equals the stored figure within a factor of 2 (below 1e-15 — a few units of the
    last place of the largest element — both count as equal: one rounding more or less is a factor there)."""
    from oracle import low_rank_estimator as ref

    c, z = R.case(name), R.load(name)
    s2, V, lam = ref.estimate_chain(z["x"], z["g"], float(z["gamma"]), float(z["cutoff"]), int(z["k_max"]), pick=z["pick"])
    assert len(lam) == int(z["k"])
    err = max(R.metric_error(R.metric_summary(s2, V, lam), z), 1e-15)
    stored = max(float(z["err_numpy"]), 1e-15)
    assert stored / 2 <= err <= stored * 2, (err, stored)
    assert c["D"] == z["x"].shape[1]


def test_fixture_guard_the_reference_reproduces_a_small_case():
    pytest.importorskip("mpmath")
    z = R.load("smallest_2_3_2")
    want = R.reference(z["x"], z["g"], z["pick"], float(z["gamma"]), float(z["cutoff"]), int(z["k_max"]))
    assert int(want["k"]) == int(z["k"])
    for key in ("dense", "scores", "gram_ev"):
        assert np.array_equal(want[key], z[key]), key


def test_a_constant_window_and_a_non_finite_one_give_exactly_the_identity():
    """What tests/test_gpu_low_rank_estimator.py asserts of the kernel, of estimate() on the CPU: a chain whose proposals were all
    rejected repeats one draw for the whole window — its mean is that draw, not the rounded sum over m (which left a ratio of two
    rounding residues as the scaling: sigma^2 = 32, 256, ...)."""
    torch = pytest.importorskip("torch")
    from nutpie_amd import low_rank as lr

    x, g = R.window_problem(np.random.default_rng(733), 3, 12, 33, 3)
    x[0, 7, 11] = np.inf
    x[1], g[1] = x[1, 0], g[1, 0]
    sig2, V, lam = lr.metric_of(lr.estimate(torch.as_tensor(x), torch.as_tensor(g), 1e-5, 2.0))
    for c in (0, 1):
        assert bool((sig2[c] == 1.0).all()) and bool((V[c] == 0.0).all()) and bool((lam[c] == 1.0).all())
    assert int((lam[2] != 1.0).sum()) >= 3


def test_the_case_table_needs_no_mpmath():
    import subprocess
    import sys

    code = "import sys; from tests import low_rank_reference as R; assert len(R.CASES) == 23; assert 'mpmath' not in sys.modules"
    subprocess.run([sys.executable, "-c", code], check=True, cwd=R.GOLDEN + "/../..")
