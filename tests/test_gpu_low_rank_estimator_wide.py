"""The tests of tests/test_gpu_low_rank_estimator.py for nphip_low_rank_estimate_wide (nutpie_amd/csrc/lowrank_est_wide.hip: up to 1024
dimensions, 64 basis draws) — the 23 fixtures of the narrow kernel, whose shapes it accepts too, and the wide-only cases of
tests/low_rank_reference_wide.py —, and which of the two kernels ``low_rank.estimate_window`` takes."""
import numpy as np
import pytest

from tests import low_rank_reference as R
from tests.test_gpu_low_rank_estimator import *  # noqa: F401,F403 - the tests themselves, their fixtures and their parametrisation
from tests.test_gpu_low_rank_estimator import _nan_trace, _same

pytestmark = pytest.mark.gpu

KERNEL = "wide"


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
