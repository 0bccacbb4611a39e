"""The estimator kernels against a 50-digit reference of the estimator (the fixtures tests/golden/low_rank_estimator_*.npz;
tests/low_rank_reference.py has the restatement, the case table and the norm), their launch paths against each other bit for bit, and
the shapes they refuse.  Every test is one or two launches over at most 8 chains.

The tests are written once, for the kernel that the collecting module names in ``KERNEL``: this module runs them for
nphip_low_rank_estimate (nutpie_amd/csrc/lowrank_est.hip: up to 512 dimensions, 32 basis draws), and
tests/test_gpu_low_rank_estimator_wide.py imports them and runs them for nphip_low_rank_estimate_wide (lowrank_est_wide.hip: up to
1024 dimensions, 64 basis draws; it also takes the wide-only cases of tests/low_rank_reference_wide.py)."""
import numpy as np
import pytest

from tests import low_rank_reference as R
from tests import low_rank_reference_wide as W

pytestmark = pytest.mark.gpu

KERNEL = "narrow"   # the row of KERNELS this module's tests run; a module that imports them names its own
__all__ = ["pytest_generate_tests", "K", "launch", "test_kernel_against_the_high_precision_reference", "test_launch_base_is_not_vacuous",
           "test_workgroups_that_take_several_chains_in_turn", "test_no_chain_list_is_block_index_as_chain",
           "test_chain_list_permuted_and_with_a_chain_twice", "test_strided_trace_view_against_its_contiguous_copy",
           "test_one_chain_alone_and_a_second_launch", "test_refusals"]

MAX_SWEEPS = 30   # kMaxSweeps of both kernels — a solver that stops there has not converged

# fn: the binding; sweeps: the diagnostic words with the sweeps of the two Jacobi solvers (square root, spectrum of S); prefix: what the
# accuracy profiles are cut from; launch: (D, m) of the launch-path problem; refused: what a refusal's message has to match
KERNELS = {
    "narrow": dict(fn="low_rank_estimate", cases=R.CASE_NAMES, sweeps=(2, 3), prefix="low_rank_estimator_accuracy", launch=(33, 12), refused="refused"),
    "wide": dict(fn="low_rank_estimate_wide", cases=R.CASE_NAMES + W.CASE_NAMES, sweeps=(0, 1), prefix="low_rank_estimator_wide_accuracy", launch=(140, 40),
                 refused="refused.*dim <= 1024.*64 basis draws"),
}


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


def pytest_generate_tests(metafunc):
    """The fixtures and the refusal table of the collecting module's kernel."""
    kernel = metafunc.module.KERNEL
    if "name" in metafunc.fixturenames:
        metafunc.parametrize("name", KERNELS[kernel]["cases"])
    if "shape_ok" in metafunc.fixturenames:
        metafunc.parametrize("what,D,m,pick,k_max,cutoff,gamma,shape_ok", REFUSALS[kernel])


@pytest.fixture(scope="module")
def K(request):
    return KERNELS[request.module.KERNEL]


def test_kernel_against_the_high_precision_reference(hip, K, name):
    """The project's bound: 10 x the worse of two independent float64 formulations of the same estimator (numpy with SVD and sqrtm,
    torch with LAPACK eigendecompositions) on the same inputs against the exact answer, and no less than 1e-12 — measured against the
    CPU formulations, never against the kernel.  The margin covers the constant between Jacobi and LAPACK and between the
    Cholesky-of-Cg and eigen-of-Cg routes; both routes square the same 1 / gamma conditioning."""
    import torch

    fn = getattr(hip, K["fn"])
    z, x, g = _case_data(name)
    pick = z["pick"]
    m, D = x.shape
    gamma, cutoff, k_max, k = float(z["gamma"]), float(z["cutoff"]), int(z["k_max"]), int(z["k"])
    lo, chain = 4, 1
    tr_x, tr_g = _nan_trace(x[None], g[None], 3, [chain], lo, 3)
    assert getattr(hip, K["fn"] + "_supported")(D, m, len(pick), k_max)
    sig2, V, lam, k_used = fn(torch.as_tensor(tr_x, device="cuda"), torch.as_tensor(tr_g, device="cuda"), torch.tensor([chain], device="cuda"),
                              lo, lo + m, pick, gamma, cutoff, k_max)
    diag = fn.last_diag
    assert tuple(diag.shape) == (1, 16)
    sweeps = [int(diag[0, w].item()) for w in K["sweeps"]]
    sig2, V, lam, k_used = sig2[0].cpu().numpy(), V[0].cpu().numpy(), lam[0].cpu().numpy(), int(k_used[0])
    assert V.shape == (k_max, D) and lam.shape == (k_max,)
    err = R.metric_error(R.metric_summary(sig2, V.T, lam), z)
    bound = max(10.0 * max(float(z["err_numpy"]), float(z["err_torch"])), 1e-12)
    print("%s %-30s err_numpy %.2e err_torch %.2e kernel %.2e bound %.2e k %d sweeps %d %d"
          % (K["prefix"], name, float(z["err_numpy"]), float(z["err_torch"]), err, bound, k_used, sweeps[0], sweeps[1]))
    assert k_used == k
    assert (V[k_used:] == 0.0).all() and (lam[k_used:] == 1.0).all()
    if k_used:
        assert np.abs(V[:k_used] @ V[:k_used].T - np.eye(k_used)).max() < 1e-9
    assert (lam[:k_used] != 1.0).all()
    assert all(1 <= s < MAX_SWEEPS for s in sweeps), sweeps
    assert err <= bound, (err, bound)


def test_the_narrow_scratch_still_holds_the_diagnostic_words(hip):
    """``low_rank_estimate.last_scratch`` ``[n, 4112]``, which older scripts read: words 4096.. of a chain's row are ``last_diag``."""
    import torch

    z = R.load(R.CASE_NAMES[0])
    m = z["x"].shape[0]
    dx, dg = torch.as_tensor(z["x"][None], device="cuda"), torch.as_tensor(z["g"][None], device="cuda")
    hip.low_rank_estimate(dx, dg, None, 0, m, z["pick"], float(z["gamma"]), float(z["cutoff"]), int(z["k_max"]))
    scratch, diag = hip.low_rank_estimate.last_scratch, hip.low_rank_estimate.last_diag
    assert tuple(scratch.shape) == (1, 4112) and torch.equal(scratch[:, 4096:], diag)
    assert (diag[0, :2] == 0).all() and (diag[0, 2:4] >= 1).all() and diag[0, 6] > 0


# ------------------------------------------------------------------ launch paths, bit for bit
N_CH, BAD, CONST = 7, 2, 4
LP_LO = 5


@pytest.fixture(scope="module")
def launch(hip, K):
    """Seven chains of the (33, 12, 12) problem (narrow) or a (140, 40, 40) problem (wide) in a NaN-padded trace — chain 2 with an inf in
    its window, chain 4 with a constant window — and their metrics from one launch with a workgroup per chain."""
    import torch

    fn = getattr(hip, K["fn"])
    lp_d, lp_m = K["launch"]
    x, g = R.window_problem(np.random.default_rng(733), N_CH, lp_m, lp_d, 3)
    x[BAD, 7, 11] = np.inf
    x[CONST], g[CONST] = x[CONST, 0], g[CONST, 0]
    tr_x, tr_g = _nan_trace(x, g, N_CH, np.arange(N_CH), LP_LO, 4)
    dx, dg = torch.as_tensor(tr_x, device="cuda"), torch.as_tensor(tr_g, device="cuda")
    pick = np.arange(lp_m)

    def run(chains, dx=dx, dg=dg, max_workgroups=0):
        idx = None if chains is None else torch.as_tensor(np.asarray(chains, dtype=np.int64), device="cuda")
        return fn(dx, dg, idx, LP_LO, LP_LO + lp_m, pick, 1e-5, 2.0, 16, max_workgroups)

    base = run(np.arange(N_CH))
    torch.cuda.synchronize()
    return dict(run=run, base=base, dx=dx, dg=dg)


def _same(got, want, rows=None):
    import torch

    for a, b in zip(got, want):
        assert torch.equal(a, b if rows is None else b[torch.as_tensor(np.asarray(rows), device=b.device)])


def test_launch_base_is_not_vacuous(launch):
    """The chains the launch-path tests compare have metrics with columns; the window with an inf and the constant window are exactly
    the identity (sigma^2 = 1, V = 0, lambda = 1, no column) — what low_rank.estimate gives on the CPU for both."""
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
    (wide) the same block of scratch — also past the early return of the chain with the non-finite window."""
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
_REFUSED_BY_BOTH = [
    ("n_pick > m", 24, 5, np.array([0, 1, 2, 3, 4, 0]), 16, 2.0, 1e-5, False),
    ("n_pick > dim", 4, 10, np.arange(6), 16, 2.0, 1e-5, False),
    ("k_max = 0", 24, 10, np.arange(10), 0, 2.0, 1e-5, False),
    ("k_max = 17", 24, 10, np.arange(10), 17, 2.0, 1e-5, False),
    ("m = 1", 24, 1, np.arange(1), 16, 2.0, 1e-5, False),
    ("cutoff = 1", 24, 10, np.arange(10), 16, 1.0, 1e-5, True),
    ("gamma = 0", 24, 10, np.arange(10), 16, 2.0, 0.0, True),
    ("pick entry = m", 24, 10, np.array([0, 1, 10]), 16, 2.0, 1e-5, True),
]
REFUSALS = {
    "narrow": [("dim = 513", 513, 12, np.arange(12), 16, 2.0, 1e-5, False), ("n_pick = 33", 64, 40, np.arange(33), 16, 2.0, 1e-5, False)] + _REFUSED_BY_BOTH,
    "wide": [("dim = 1025", 1025, 12, np.arange(12), 16, 2.0, 1e-5, False), ("n_pick = 65", 128, 70, np.arange(65), 16, 2.0, 1e-5, False)] + _REFUSED_BY_BOTH,
}


def test_refusals(hip, K, what, D, m, pick, k_max, cutoff, gamma, shape_ok):
    import torch

    assert bool(getattr(hip, K["fn"] + "_supported")(D, m, len(pick), k_max)) == shape_ok, what
    t = torch.zeros(2, m + 3, D, dtype=torch.float64, device="cuda")
    with pytest.raises(RuntimeError, match=K["refused"]):
        getattr(hip, K["fn"])(t, t.clone(), None, 1, 1 + m, pick, gamma, cutoff, k_max)
