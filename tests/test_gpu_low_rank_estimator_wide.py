"""nphip_low_rank_estimate_wide (nutpie_amd/csrc/lowrank_est_wide.hip: up to 1024 dimensions, 64 basis draws) against the 50-digit
reference of the estimator — the 23 fixtures of the narrow kernel, whose shapes it accepts too, and the wide-only cases of
tests/low_rank_reference_wide.py —, its launch paths against each other bit for bit, the shapes it refuses, and which of the two
kernels ``low_rank.estimate_window`` takes.  Every test is one or two launches over at most 8 chains."""
import numpy as np
import pytest

from tests import low_rank_reference as R
from tests import low_rank_reference_wide as W

pytestmark = pytest.mark.gpu

SWEEP_WORDS = (0, 1)   # the diagnostic words of a chain: sweeps of the two Jacobi passes (square root, spectrum of S)
MAX_SWEEPS = 30        # lowrank_est_wide.hip: kMaxSweeps — a solver that stops there has not converged


def _nan_trace(x, g, n_all, chains, lo, pad):
    """Trace-shaped arrays [n_all, lo + m + pad, D] that hold the windows x, g [n, m, D] of ``chains`` at [lo, lo + m) and NaN everywhere
    else: a read outside the window or of another chain turns the metric into the identity instead of hiding in a tolerance."""
    n, m, D = x.shape
    tr_x, tr_g = np.full((n_all, lo + m + pad, D), np.nan), np.full((n_all, lo + m + pad, D), np.nan)
    tr_x[chains, lo:lo + m], tr_g[chains, lo:lo + m] = x, g
    return tr_x, tr_g


def _case_data(name):
    if name in W.CASE_NAMES:
        z = W.load(name)
        x, g = W.inputs(W.case(name))
        assert W.digest(x, g) == str(z["sha256"])
        return z, x, g
    z = R.load(name)
    return z, z["x"], z["g"]


@pytest.mark.parametrize("name", R.CASE_NAMES + W.CASE_NAMES)
def test_kernel_against_the_high_precision_reference(hip, name):
    """The project's bound: 10 x the worse of two independent float64 formulations of the same estimator (numpy with SVD and sqrtm,
    torch with LAPACK eigendecompositions) on the same inputs against the exact answer, and no less than 1e-12 — measured against the
    CPU formulations, never against the kernel."""
    import torch

    z, x, g = _case_data(name)
    pick = z["pick"]
    m, D = x.shape
    gamma, cutoff, k_max, k = float(z["gamma"]), float(z["cutoff"]), int(z["k_max"]), int(z["k"])
    lo, chain = 4, 1
    tr_x, tr_g = _nan_trace(x[None], g[None], 3, [chain], lo, 3)
    assert hip.low_rank_estimate_wide_supported(D, m, len(pick), k_max)
    sig2, V, lam, k_used = hip.low_rank_estimate_wide(torch.as_tensor(tr_x, device="cuda"), torch.as_tensor(tr_g, device="cuda"), torch.tensor([chain], device="cuda"),
                                                      lo, lo + m, pick, gamma, cutoff, k_max)
    diag = hip.low_rank_estimate_wide.last_diag
    assert tuple(diag.shape) == (1, 16)
    sweeps = [int(diag[0, w].item()) for w in SWEEP_WORDS]
    sig2, V, lam, k_used = sig2[0].cpu().numpy(), V[0].cpu().numpy(), lam[0].cpu().numpy(), int(k_used[0])
    assert V.shape == (k_max, D) and lam.shape == (k_max,)
    err = R.metric_error(R.metric_summary(sig2, V.T, lam), z)
    bound = max(10.0 * max(float(z["err_numpy"]), float(z["err_torch"])), 1e-12)
    print("low_rank_estimator_wide_accuracy %-30s err_numpy %.2e err_torch %.2e kernel %.2e bound %.2e k %d sweeps %d %d"
          % (name, float(z["err_numpy"]), float(z["err_torch"]), err, bound, k_used, sweeps[0], sweeps[1]))
    assert k_used == k
    assert (V[k_used:] == 0.0).all() and (lam[k_used:] == 1.0).all()
    if k_used:
        assert np.abs(V[:k_used] @ V[:k_used].T - np.eye(k_used)).max() < 1e-9
    assert (lam[:k_used] != 1.0).all()
    assert all(1 <= s < MAX_SWEEPS for s in sweeps), sweeps
    assert err <= bound, (err, bound)


# ------------------------------------------------------------------ launch paths, bit for bit
N_CH, BAD, CONST = 7, 2, 4
LP_D, LP_M, LP_LO = 140, 40, 5


@pytest.fixture(scope="module")
def launch(hip):
    """Seven chains of a (140, 40, 40) problem in a NaN-padded trace — chain 2 with an inf in its window, chain 4 with a constant
    window — and their metrics from one launch with a workgroup per chain."""
    import torch

    x, g = R.window_problem(np.random.default_rng(733), N_CH, LP_M, LP_D, 3)
    x[BAD, 7, 11] = np.inf
    x[CONST], g[CONST] = x[CONST, 0], g[CONST, 0]
    tr_x, tr_g = _nan_trace(x, g, N_CH, np.arange(N_CH), LP_LO, 4)
    dx, dg = torch.as_tensor(tr_x, device="cuda"), torch.as_tensor(tr_g, device="cuda")
    pick = np.arange(LP_M)

    def run(chains, dx=dx, dg=dg, max_workgroups=0):
        idx = None if chains is None else torch.as_tensor(np.asarray(chains, dtype=np.int64), device="cuda")
        return hip.low_rank_estimate_wide(dx, dg, idx, LP_LO, LP_LO + LP_M, pick, 1e-5, 2.0, 16, max_workgroups)

    base = run(np.arange(N_CH))
    torch.cuda.synchronize()
    return dict(run=run, base=base, dx=dx, dg=dg)


def _same(got, want, rows=None):
    import torch

    for a, b in zip(got, want):
        assert torch.equal(a, b if rows is None else b[torch.as_tensor(np.asarray(rows), device=b.device)])


def test_launch_base_is_not_vacuous(launch):
    """The chains the launch-path tests compare have metrics with columns; the window with an inf and the constant window are exactly
    the identity (sigma^2 = 1, V = 0, lambda = 1, no column)."""
    sig2, V, lam, k_used = (t.cpu().numpy() for t in launch["base"])
    for c in range(N_CH):
        if c in (BAD, CONST):
            assert (sig2[c] == 1.0).all() and (V[c] == 0.0).all() and (lam[c] == 1.0).all() and k_used[c] == 0
        else:
            assert k_used[c] >= 3 and np.isfinite(sig2[c]).all() and np.isfinite(V[c]).all() and not (sig2[c] == 1.0).any()
    assert len({sig2[c].tobytes() for c in range(N_CH)}) == N_CH - 1


@pytest.mark.parametrize("max_workgroups", [1, 2, 3, 6])
def test_workgroups_that_take_several_chains_in_turn(launch, max_workgroups):
    """The production launch shape: fewer workgroups than chains, each taking chains slot, slot + grid, ... through the same LDS and
    the same block of scratch — also past the early return of the chain with the non-finite window."""
    _same(launch["run"](np.arange(N_CH), max_workgroups=max_workgroups), launch["base"])


def test_no_chain_list_is_block_index_as_chain(launch):
    _same(launch["run"](None), launch["base"])
    _same(launch["run"](None, max_workgroups=3), launch["base"])


def test_chain_list_permuted_and_with_a_chain_twice(launch):
    order = [5, 2, 0, 6, 4, 1, 3]
    _same(launch["run"](order), launch["base"], order)
    twice = [3, 6, 3, 2]
    _same(launch["run"](twice, max_workgroups=2), launch["base"], twice)


def test_strided_trace_view_against_its_contiguous_copy(launch):
    """Draw stride D + 5, chain stride of more than T rows; the padding holds NaN."""
    import torch

    dx, dg = launch["dx"], launch["dg"]
    n, T, D = dx.shape
    views = []
    for t in (dx, dg):
        big = torch.full((n, T + 3, D + 5), float("nan"), dtype=torch.float64, device="cuda")
        big[:, :T, :D] = t
        views.append(big[:, :T, :D])
    assert views[0].stride() == ((T + 3) * (D + 5), D + 5, 1)
    _same(launch["run"](np.arange(N_CH), dx=views[0], dg=views[1]), launch["base"])
    _same(launch["run"](None, dx=views[0], dg=views[1], max_workgroups=2), launch["base"])


def test_one_chain_alone_and_a_second_launch(launch):
    _same(launch["run"]([3]), launch["base"], [3])
    _same(launch["run"](np.arange(N_CH)), launch["base"])


# ------------------------------------------------------------------ refusals
@pytest.mark.parametrize("what,D,m,pick,k_max,cutoff,gamma,shape_ok", [
    ("dim = 1025", 1025, 12, np.arange(12), 16, 2.0, 1e-5, False),
    ("n_pick = 65", 128, 70, np.arange(65), 16, 2.0, 1e-5, False),
    ("n_pick > m", 24, 5, np.array([0, 1, 2, 3, 4, 0]), 16, 2.0, 1e-5, False),
    ("n_pick > dim", 4, 10, np.arange(6), 16, 2.0, 1e-5, False),
    ("k_max = 0", 24, 10, np.arange(10), 0, 2.0, 1e-5, False),
    ("k_max = 17", 24, 10, np.arange(10), 17, 2.0, 1e-5, False),
    ("m = 1", 24, 1, np.arange(1), 16, 2.0, 1e-5, False),
    ("cutoff = 1", 24, 10, np.arange(10), 16, 1.0, 1e-5, True),
    ("gamma = 0", 24, 10, np.arange(10), 16, 2.0, 0.0, True),
    ("pick entry = m", 24, 10, np.array([0, 1, 10]), 16, 2.0, 1e-5, True),
])
def test_refusals(hip, what, D, m, pick, k_max, cutoff, gamma, shape_ok):
    import torch

    assert bool(hip.low_rank_estimate_wide_supported(D, m, len(pick), k_max)) == shape_ok, what
    t = torch.zeros(2, m + 3, D, dtype=torch.float64, device="cuda")
    with pytest.raises(RuntimeError, match="refused.*dim <= 1024.*64 basis draws"):
        hip.low_rank_estimate_wide(t, t.clone(), None, 1, 1 + m, pick, gamma, cutoff, k_max)


# ------------------------------------------------------------------ routing
def _trace(n, m, D, seed, lo=3):
    import torch

    x, g = R.window_problem(np.random.default_rng(seed), n, m, D, 3)
    tr_x, tr_g = _nan_trace(x, g, n, np.arange(n), lo, 2)
    return torch.as_tensor(tr_x, device="cuda"), torch.as_tensor(tr_g, device="cuda")


def _raise(*a, **k):
    raise AssertionError("low_rank.estimate was called")


def test_routing_a_shape_both_kernels_cover_stays_on_the_narrow_kernel(hip, monkeypatch):
    from nutpie_amd import low_rank as lr

    dx, dg = _trace(3, 20, 48, 11)
    assert hip.low_rank_estimate_supported(48, 20, 20, 16) and hip.low_rank_estimate_wide_supported(48, 20, 20, 16)
    monkeypatch.setattr(lr, "estimate", _raise)
    monkeypatch.setattr(hip, "low_rank_estimate_wide", _raise)
    got = lr.estimate_window(dx, dg, [2, 0], 3, 23, 1e-5, 2.0)
    import torch

    want = hip.low_rank_estimate(dx, dg, torch.tensor([2, 0], device="cuda"), 3, 23, lr.basis_pick(20, None), 1e-5, 2.0, 16)
    _same(got, want[:3])
    assert int(want[3].min()) >= 1


def test_routing_300_dimensions_with_64_basis_draws_goes_to_the_wide_kernel(hip, monkeypatch):
    import torch

    from nutpie_amd import low_rank as lr

    dx, dg = _trace(2, 70, 300, 12)
    assert not hip.low_rank_estimate_supported(300, 70, 64, 16) and hip.low_rank_estimate_wide_supported(300, 70, 64, 16)
    monkeypatch.setattr(lr, "estimate", _raise)
    got = lr.estimate_window(dx, dg, [1, 0], 3, 73, 1e-5, 2.0, basis_draws=64, max_workgroups=1)
    pick = lr.basis_pick(70, 64)
    assert len(pick) == 64
    want = hip.low_rank_estimate_wide(dx, dg, torch.tensor([1, 0], device="cuda"), 3, 73, pick, 1e-5, 2.0, 16)
    _same(got, want[:3])
    assert int(want[3].min()) >= 1


def test_routing_1025_dimensions_stays_with_estimate(hip, monkeypatch):
    import torch

    from nutpie_amd import low_rank as lr

    called = []

    def fake(x, g, gamma, cutoff, k_max=16, basis_draws=None):
        called.append(tuple(x.shape))
        raise _Stop()

    class _Stop(Exception):
        pass

    monkeypatch.setattr(lr, "estimate", fake)
    t = torch.zeros(2, 16, 1025, dtype=torch.float64, device="cuda")
    with pytest.raises(_Stop):
        lr.estimate_window(t, t.clone(), None, 2, 14, 1e-5, 2.0, basis_draws=8)
    assert called == [(2, 12, 1025)]
