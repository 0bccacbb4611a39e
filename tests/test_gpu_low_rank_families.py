"""The kernels that run under a handed-in low-rank metric (kernels.hip: Machine<..., LR>), held to the oracle where trees TURN.

The cases of tests/test_gpu_low_rank.py hand in metrics that fit the target so badly that almost every tree runs to maxdepth: the
velocity-based turning criteria (check1_v / check_a_v / sub_a_v / sub_b_v) are evaluated there, but hardly ever say "turning".  Here
the metrics fit (``matched_metrics``: the target's marginal variances, jittered), so that nine draws in ten end in a U-turn, at several
depths — and the grid lists every instantiation: ``w1_lr`` at 1..8 chunks per lane, ``ring_lr`` at 2 x 5..8 and 4 x 5..8, the
memory-resident form at 1, 4, 8 and 16 waves per chain, every compile-time column count of ``lr_dispatch`` (0, 4, 8, 12, 16) and both sides
of the second reduction of ``lr_coef`` (k <= 8, k > 8).  Divergence records (``replay_divergence`` through the run-time forms ``lr_acc`` /
``lr_apply``), the awkward settings and a column count that changes between hand-ins follow.

Every comparison is bit for bit against ``oracle.sample_tridiag`` with ``set_metric_schedule``.  What a case is meant to exercise is
asserted on the oracle's output alone (``_check_inputs``), in the GPU tests and in one test that needs no GPU."""
import numpy as np
import pytest

from nutpie_amd.gaussian import ar1_gaussian
from tests.conftest import assert_trace_equal
from tests.test_gpu_low_rank import random_metrics, run_engine_with_metrics
from tests.test_gpu_parity import DIV_KEYS, oracle_settings

PAUSES = [12, 27]


# ------------------------------------------------------------------------------------ metrics that fit the target
_variances = {}


def marginal_variances(dim):
    """diag(P^-1) of the tridiagonal precision of ``ar1_gaussian(dim)`` without the dense inverse: with the pivots of the elimination
    from the top, d_i = a_i - b_{i-1}^2 / d_{i-1}, and from the bottom, e_i = a_i - b_i^2 / e_{i+1}:  (P^-1)_ii = 1 / (d_i + e_i - a_i)."""
    if dim not in _variances:
        m = ar1_gaussian(dim)
        a, b = np.asarray(m.diag, dtype=np.float64), np.asarray(m.offdiag, dtype=np.float64)
        d, e = a.copy(), a.copy()
        for i in range(1, dim):
            d[i] = a[i] - b[i - 1] ** 2 / d[i - 1]
        for i in range(dim - 2, -1, -1):
            e[i] = a[i] - b[i] ** 2 / e[i + 1]
        _variances[dim] = 1.0 / (d + e - a)
    return _variances[dim]


def matched_metrics(rng, updates, chains, dim, k):
    """Metrics under which the trees turn: random orthonormal columns, sigma^2 = the target's marginal variances times exp(0.3 N(0, 1)) per
    update and chain, eigenvalues within a factor of two of one."""
    _, V, _ = random_metrics(rng, updates, chains, dim, k)
    sig2 = marginal_variances(dim) * np.exp(0.3 * rng.normal(size=(updates, chains, dim)))
    lam = np.exp(rng.uniform(np.log(0.5), np.log(2.0), size=(updates, chains, k)))
    return sig2, V, lam


# ------------------------------------------------------------------------------------ the cases
class Case:
    """One job: model, metrics, settings, launch — and the kernel it is meant to run on (family, waves per chain, chunks per wave)."""

    def __init__(self, section, dim, k, geometry, *, chains, tune, draws, seed, waves=0, launch=None, settings=None, pauses=PAUSES, name=None):
        self.section, self.dim, self.k, self.geometry = section, dim, k, geometry
        self.kw = dict(chains=chains, tune=tune, draws=draws, seed=seed)
        self.waves, self.launch, self.settings, self.pauses = waves, dict(launch or {}), dict(settings or {}), list(pauses)
        family, W, nv = geometry
        self.id = f"{section}-{dim}-{family}-{W}x{nv}-k{k}" + (f"-{name}" if name else "")

    def metrics(self):
        """(what the engine is handed per update, what the oracle's schedule holds)"""
        rng = np.random.default_rng(self.dim + self.k)
        sig2, V, lam = matched_metrics(rng, len(self.pauses), self.kw["chains"], self.dim, self.k)
        return [(sig2[u], V[u] if self.k else None, lam[u] if self.k else None) for u in range(len(self.pauses))], (sig2, V, lam)


class ShrinkingColumns(Case):
    """k = 16, then the first five of the second update's columns, then none.  The oracle's schedule has one column count: it gets 16 three
    times, the absent columns as zero columns with eigenvalue one — for finite values the same arithmetic ((1 - 1) * 0 = 0 and
    fma(0, 0, w) = w), as the engine's own passes, rounded up to four columns, already rely on."""

    def metrics(self):
        handed, (sig2, V, lam) = super().metrics()
        V, lam = V.copy(), lam.copy()
        V[1, :, 5:], lam[1, :, 5:] = 0.0, 1.0
        V[2], lam[2] = 0.0, 1.0
        return [handed[0], (sig2[1], handed[1][1][:, :5].copy(), handed[1][2][:, :5].copy()), (sig2[2], None, None)], (sig2, V, lam)


def _grid():
    # every register instantiation under the metric, every column class of lr_dispatch (k rounded up to 0, 4, 8, 12, 16), k = 8 and k = 9
    rows = [
        (100, 1, 1, 1, {}), (200, 1, 2, 4, dict(evals_per_launch=1)), (380, 1, 3, 5, {}), (500, 1, 4, 8, {}),
        (640, 1, 5, 9, dict(evals_per_launch=7)), (700, 1, 6, 12, {}), (896, 1, 7, 13, {}), (1000, 1, 8, 16, dict(evals_per_launch=1)),
        (1100, 2, 5, 16, {}), (1500, 2, 6, 13, dict(evals_per_launch=1)), (1700, 2, 7, 8, {}), (2048, 2, 8, 5, {}),
        (2500, 4, 5, 12, {}), (3000, 4, 6, 1, dict(evals_per_launch=5)), (3500, 4, 7, 9, {}), (4096, 4, 8, 16, {}),
    ]
    # one wave per chain: five chains = a full workgroup of four and a partial one
    cases = [Case("grid", dim, k, ("w1_lr" if W == 1 else "ring_lr", W, nv), chains=5 if W == 1 else 3, tune=40, draws=10, seed=dim + 5, launch=launch,
                  settings=dict(store_mass_matrix=True)) for dim, W, nv, k, launch in rows]
    # the memory-resident form at the wave counts that have no case elsewhere
    for dim, W, k, waves, launch in [(5003, 8, 7, 8, {}), (6000, 16, 3, 16, {}), (1000, 1, 8, 0, dict(no_register_kernel=True))]:
        cases.append(Case("grid", dim, k, ("memory", W, -1), chains=5 if W == 1 else 3, tune=40, draws=10, seed=dim + 5, waves=waves, launch=launch,
                          settings=dict(store_mass_matrix=True)))
    return cases


def _divergence_cases():
    rows = [(500, 5, ("w1_lr", 1, 4), {}), (1000, 16, ("w1_lr", 1, 8), dict(evals_per_launch=7)), (1300, 4, ("ring_lr", 2, 6), {}),
            (2500, 9, ("ring_lr", 4, 5), dict(evals_per_launch=9)), (1000, 16, ("memory", 1, -1), dict(no_register_kernel=True)),
            (5003, 2, ("memory", 4, -1), {})]
    return [Case("div", dim, k, geo, chains=4, tune=60, draws=15, seed=dim + 17, launch=launch, settings=dict(store_divergences=True, max_energy_error=0.6))
            for dim, k, geo, launch in rows]


AWKWARD = [
    ("maxdepth3", dict(maxdepth=3), dict(evals_per_launch=5)),
    ("mindepth3", dict(mindepth=3), {}),
    ("no-turning-maxdepth4", dict(check_turning=False, maxdepth=4), {}),
    ("deep-trees", dict(maxdepth=12, target_accept=0.95), {}),
    ("jitter-mindepth2", dict(step_size_jitter=0.2, mindepth=2), dict(evals_per_launch=13)),
    ("draw-based-gradient-stored", dict(use_grad_based_mass_matrix=False, store_gradient=True), {}),
]


def _awkward_cases():
    return [Case("awkward", dim, 7, geo, chains=3, tune=50, draws=12, seed=dim + 3, launch=launch, settings=settings, name=name)
            for dim, geo in [(1000, ("w1_lr", 1, 8)), (1300, ("ring_lr", 2, 6))] for name, settings, launch in AWKWARD]


GRID, DIVERGENCES, AWKWARD_CASES = _grid(), _divergence_cases(), _awkward_cases()
SHRINKING = [ShrinkingColumns("shrinking", 700, 16, ("w1_lr", 1, 6), chains=5, tune=40, draws=10, seed=705, pauses=[10, 20, 30],
                              settings=dict(store_mass_matrix=True))]
ALL = GRID + DIVERGENCES + AWKWARD_CASES + SHRINKING


def _ids(cases):
    return [c.id for c in cases]


# ------------------------------------------------------------------------------------ geometry, oracle, conditions on the inputs
def _check_geometry(hip, case):
    """A case must not quietly run on another kernel: the family, the waves per chain and the chunks per wave the host chooses."""
    g = hip.test_choose_geometry(case.dim, low_rank_metric=True, waves_per_chain=case.waves, no_register_kernel=bool(case.launch.get("no_register_kernel")))
    assert (g["family"], g["W"], g["NV"]) == case.geometry and g["in_table"], (case.id, g)
    return g


_want = {}


def _oracle(oracle, case):
    # one oracle run per case, shared by the GPU test and the test of the inputs (never modified)
    if case.id not in _want:
        handed, (sig2, V, lam) = case.metrics()
        model = ar1_gaussian(case.dim)
        s = oracle_settings(oracle, W=case.geometry[1], **case.kw, **case.settings)
        s.set_metric_schedule(case.pauses, sig2, V if case.k else None, lam if case.k else None)
        _want[case.id] = (handed, (sig2, V, lam), oracle.sample_tridiag(s, model.diag, model.offdiag))
    return _want[case.id]


def _check_inputs(case, want):
    """What the case is there for, on the oracle's output alone (conditions, not tolerances: a case that misses one gets other inputs)."""
    st = {k: np.asarray(want.stats[k])[:, case.pauses[0]:] for k in ("depth", "diverging", "maxdepth_reached")}
    depth, div, maxd = st["depth"].astype(np.int64), st["diverging"].astype(bool), st["maxdepth_reached"].astype(bool)
    turned = ~maxd & ~div
    print(f"{case.id}: {turned.sum()} of {turned.size} draws under the metric end in a U-turn, at depths {sorted(set(depth[turned].tolist()))}; "
          f"{div.sum()} diverge ({(div & (depth >= 2)).sum()} at depth >= 2), {maxd.sum()} at maxdepth; "
          f"{int(np.asarray(want.stats['n_steps']).sum())} leapfrogs")
    if case.section in ("grid", "shrinking"):
        assert turned.mean() >= 0.8, "the case is meant to end its draws in U-turns"
        assert len(set(depth[turned].tolist())) >= 3, "... at several depths"
    elif case.section == "div":
        assert (div & (depth >= 2)).sum() >= 20, "the case is meant to diverge deep inside doublings (leaves replayed)"
        assert turned.sum() >= 40
    else:
        if case.settings.get("maxdepth") in (3, 4):
            assert maxd.sum() > 0
        if case.settings.get("maxdepth") == 12:
            assert depth.max() >= 10, "deep trees are the point"


def _engine(hip, case):
    handed, _, _ = _want[case.id]
    model = ar1_gaussian(case.dim)
    chains = case.kw["chains"]
    s = hip.PyNutsSettings.Diag(case.kw["seed"])
    s.update(num_tune=case.kw["tune"], num_draws=case.kw["draws"], num_chains=chains, low_rank_metric=True, **case.settings)
    s.set_pause_draws(case.pauses)
    smp = hip.PySampler(s, hip.TridiagGaussianModel(model.diag, model.offdiag), waves_per_chain=case.waves, manual=True, **case.launch)
    nxt = 0
    for _ in range(100000):
        done, _, _ = smp.step(4)
        if done:
            break
        if nxt < len(handed) and smp.waiting().all():
            smp.set_metric(np.arange(chains), *handed[nxt])
            nxt += 1
    assert done and nxt == len(handed)
    W = smp.waves_per_chain      # (before the results are taken: that empties the sampler)
    return smp.take_results(), W


def _run(hip, oracle, case):
    _check_geometry(hip, case)
    handed, (sig2, V, lam), want = _oracle(oracle, case)
    _check_inputs(case, want)
    if type(case) is Case:
        # (the driver of tests/test_gpu_low_rank.py: one column count for every update)
        model = ar1_gaussian(case.dim)
        got, W = run_engine_with_metrics(hip, hip.TridiagGaussianModel(model.diag, model.offdiag), case.pauses, sig2, V, lam, waves=case.waves,
                                         launch=case.launch, **case.kw, **case.settings)
    else:
        got, W = _engine(hip, case)
    assert W == case.geometry[1]
    assert_trace_equal(got, want)
    if case.settings.get("store_mass_matrix"):
        assert np.array_equal(got.stats["mass_matrix_inv"], want.stats["mass_matrix_inv"])
        assert np.array_equal(got.stats["mass_matrix_inv"][:, case.pauses[-1] + 3], sig2[-1])      # the diagonal part is the handed-in sigma^2, kept
    return got, want


# ------------------------------------------------------------------------------------ on the GPU
@pytest.mark.gpu
@pytest.mark.parametrize("case", GRID, ids=_ids(GRID))
def test_every_instantiation_under_a_metric_that_fits(hip, oracle, case):
    _run(hip, oracle, case)


@pytest.mark.gpu
@pytest.mark.parametrize("case", DIVERGENCES, ids=_ids(DIVERGENCES))
def test_divergence_records_under_the_metric(hip, oracle, case):
    # replay_divergence rebuilds the failed leapfrog with the memory-resident lf1, whose low-rank branch applies the columns four at a time
    # at run time (lr_acc / lr_apply), where the leaf that failed used the compile-time forms: the two have to agree bit for bit
    got, want = _run(hip, oracle, case)
    div = np.asarray(got.stats["diverging"]).astype(bool)
    for k in DIV_KEYS:
        a, b = got.stats[k], want.stats[k]
        assert np.array_equal(np.isnan(a), np.isnan(b)), k
        assert np.array_equal(a[~np.isnan(a)], b[~np.isnan(b)]), k
        assert np.all(np.isnan(a[~div])), k
    assert np.all(np.isfinite(got.stats["divergence_start"][div]))


@pytest.mark.gpu
@pytest.mark.parametrize("case", AWKWARD_CASES, ids=_ids(AWKWARD_CASES))
def test_awkward_settings_under_the_metric(hip, oracle, case):
    got, want = _run(hip, oracle, case)
    if case.settings.get("store_gradient"):
        assert np.array_equal(got.stats["gradient"], want.stats["gradient"])


@pytest.mark.gpu
@pytest.mark.parametrize("case", SHRINKING, ids=_ids(SHRINKING))
def test_column_count_that_changes_between_hand_ins(hip, oracle, case):
    _run(hip, oracle, case)


# ------------------------------------------------------------------------------------ without a GPU
@pytest.mark.parametrize("case", ALL, ids=_ids(ALL))
def test_the_inputs_exercise_what_they_are_meant_to(oracle, case):
    """The oracle alone over every case: the geometry the host chooses is the one the case names, and the trees turn / diverge / reach
    maxdepth as the case needs — so that a change of the inputs that empties a case is noticed without a GPU."""
    from nutpie_amd import _lib

    _check_geometry(_lib, case)
    _check_inputs(case, _oracle(oracle, case)[2])


def test_marginal_variances_against_the_dense_inverse():
    for dim in (2, 100, 380):
        np.testing.assert_allclose(marginal_variances(dim), np.diag(ar1_gaussian(dim).covariance()), rtol=1e-10, atol=0)
