"""The fixtures the wide estimator kernel is held to (tests/golden/low_rank_estimator_wide_*.npz, written by
tests/golden/make_low_rank_reference_wide.py from the 50-digit restatement tests/low_rank_reference.py on the regenerated inputs of
tests/low_rank_reference_wide.py): the inputs regenerate bit for bit, sit away from every threshold, the fixtures have not rotted, the
C-ABI declares and binds the kernel's two entry points, and every shape goes to the kernel that is to take it."""
import math
import os
import re

import numpy as np
import pytest

from tests import low_rank_reference_wide as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def windows():
    """The regenerated inputs of every case, once."""
    return {c["name"]: W.inputs(c) for c in W.CASES}


def test_the_case_table_covers_what_only_the_wide_kernel_takes():
    assert all(c["D"] > 64 for c in W.CASES)                                     # the fixtures hold the diagonal and the probes
    assert all(c["b"] > 32 or c["D"] > 512 for c in W.CASES)                     # outside the narrow kernel's shape
    assert all(c["b"] <= 64 and c["b"] <= c["m"] and c["b"] <= c["D"] <= 1024 for c in W.CASES)
    assert {33, 64} <= {c["b"] for c in W.CASES} and {159, 160, 161, 513, 1024} <= {c["D"] for c in W.CASES}
    assert any(c["m"] > c["b"] for c in W.CASES) and any(2 * c["b"] > c["D"] for c in W.CASES)
    assert {1, 4, 16} <= {c["k_max"] for c in W.CASES} and {2.0, 100.0} <= {c["cutoff"] for c in W.CASES} and {1e-5, 1e-3} <= {c["gamma"] for c in W.CASES}
    assert {None, "constant_coordinate", "repeated_rows", "scaled"} <= {c["variant"] for c in W.CASES}


@pytest.mark.parametrize("name", W.CASE_NAMES)
def test_inputs_regenerate_bit_for_bit(windows, name):
    """The fixture holds no window: the digest of the regenerated one is the digest of the one the reference saw.  Every entry is a small
    integer times a power of two, so no operation that built it rounded."""
    c, z = W.case(name), W.load(name)
    x, g = windows[name]
    assert x.shape == g.shape == (c["m"], c["D"]) and x.dtype == g.dtype == np.float64
    assert W.digest(x, g) == str(z["sha256"])
    for a in (x, g):
        mant, _ = np.frexp(a)
        assert np.array_equal(mant * 2.0**12, np.round(mant * 2.0**12))          # at most 12 significant bits
    if c["variant"] == "scaled":
        sd = x.std(0)
        assert sd.max() / sd.min() > 1e11                                        # 2^40 between the scales of the first and the last coordinate
    if c["variant"] == "constant_coordinate":
        assert (x[:, 7] == x[0, 7]).all()
    if c["variant"] == "repeated_rows":
        assert np.array_equal(x[5:8], x[0:3]) and np.array_equal(g[5:8], g[0:3])


@pytest.mark.parametrize("name", W.CASE_NAMES)
def test_fixture_inputs_sit_away_from_every_threshold(name):
    """The conditions of tests/test_low_rank_reference_cpu.py, on the wide fixtures: the kernel decides the rank of the basis on
    Cholesky pivots and the reference on eigenvalues, and both cut the spectrum at ``cutoff`` and at ``k_max`` columns."""
    c, z = W.case(name), W.load(name)
    assert np.array_equal(z["pick"], W.pick_of(c["m"], c["b"]))
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
    assert k >= 1 or name in W.NO_COLUMNS_ALLOWED
    want = {key: z[key] for key in ("dense", "diag", "probe") if key in z}
    assert set(want) == {"diag", "probe"}
    assert all(np.isfinite(v).all() for v in want.values())


def test_the_selection_cases_have_to_choose_and_the_large_cutoff_leaves_few():
    for name in ("select_80_33_33_kmax4", "select_80_33_33_kmax1"):
        z = W.load(name)
        assert int((z["scores"] > math.log(2.0)).sum()) > int(z["k_max"]) == int(z["k"])
    z = W.load("cutoff100_80_33_33")
    assert int(z["k"]) < int(z["k_max"])
    assert int(W.load("full_160_64_64")["k"]) == 16 and int((W.load("rows_100_64_64")["gram_ev"] > 1e-10).sum()) == 100


@pytest.mark.parametrize("name", W.CASE_NAMES)
def test_fixture_guard_the_numpy_restatement_is_as_far_from_the_reference_as_recorded(windows, name):
    """``err_numpy`` recomputed from the regenerated inputs equals the stored figure within a factor of 2 (below 1e-15 both count as equal).
    Under the BLAS threading of the generator: at 1e-5 the figure is rounding noise times the formulation's condition number, and an
    SVD shared among threads rounds differently (tile_159: 3.0e-5 on eight threads against 1.5e-5 on one)."""
    from oracle import low_rank_estimator as ref
    from tests.low_rank_reference import one_blas_thread

    z = W.load(name)
    x, g = windows[name]
    with one_blas_thread():
        s2, V, lam = ref.estimate_chain(x, g, float(z["gamma"]), float(z["cutoff"]), int(z["k_max"]), pick=z["pick"])
    assert len(lam) == int(z["k"])
    err = max(W.metric_error(W.metric_summary(s2, V, lam), z), 1e-15)
    stored = max(float(z["err_numpy"]), 1e-15)
    assert stored / 2 <= err <= stored * 2, (err, stored)


def test_fixture_guard_the_reference_reproduces_a_small_problem_of_this_family():
    """The reference on a (66, 4, 4) window of the same construction (seconds), against the numpy restatement: the generator's two
    ingredients — these inputs and tests/low_rank_reference.py::reference — still fit together."""
    pytest.importorskip("mpmath")
    from oracle import low_rank_estimator as ref

    c = dict(W.case("past_narrow_80_33_33"), D=66, m=4, b=4, gamma=1e-3)
    x, g = W.inputs(c)
    pick = W.pick_of(4, 4)
    want = W.reference(x, g, pick, c["gamma"], c["cutoff"], c["k_max"])
    assert set(want) >= {"diag", "probe", "k", "scores", "gram_ev"} and len(want["gram_ev"]) == 8
    s2, V, lam = ref.estimate_chain(x, g, c["gamma"], c["cutoff"], c["k_max"], pick=pick)
    assert len(lam) == int(want["k"])
    assert W.metric_error(W.metric_summary(s2, V, lam), want) < 1e-9


def test_the_case_table_needs_no_mpmath():
    import subprocess
    import sys

    code = "import sys; from tests import low_rank_reference_wide as W; assert len(W.CASES) == 16; assert 'mpmath' not in sys.modules"
    subprocess.run([sys.executable, "-c", code], check=True, cwd=ROOT)


def _arguments(decl):
    return len([a for a in decl.split(",") if a.strip()])


def test_the_header_declares_both_entry_points_and_the_binding_matches():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "nutpie_hip.h")).read(), flags=re.S)
    decl = {name: _arguments(args) for name, args in re.findall(r"\bint\s+(nphip_low_rank_estimate[a-z_]*)\s*\(([^)]*)\)", text)}
    assert decl == {"nphip_low_rank_estimate_supported": 4, "nphip_low_rank_estimate": 20,
                    "nphip_low_rank_estimate_wide_supported": 4, "nphip_low_rank_estimate_wide": 20}
    from nutpie_amd import _lib

    L = _lib.lib()
    for name, n_args in decl.items():
        assert len(getattr(L, name).argtypes) == n_args, name
    assert L.nphip_low_rank_estimate_wide.argtypes == L.nphip_low_rank_estimate.argtypes
    # the shape limits, as the header states them (no GPU needed: the predicate is host code)
    ok = _lib.low_rank_estimate_wide_supported
    assert ok(1024, 256, 64, 16) and ok(1, 2, 1, 1) and ok(300, 256, 64, 16) and ok(24, 10, 10, 16)
    assert not ok(1025, 256, 64, 16) and not ok(300, 256, 65, 16) and not ok(300, 1, 1, 16) and not ok(40, 64, 41, 16)
    assert not ok(300, 32, 33, 16) and not ok(300, 256, 64, 17) and not ok(300, 256, 64, 0)
    assert _lib.WIDE_WORKGROUP_SCRATCH == 3 * 1024 + 3 * 128 * 128 + 16 * 128


def test_every_shape_the_narrow_kernel_takes_the_wide_one_takes_too_and_the_choice_is_narrow_first():
    """``low_rank.estimate_window`` and the driver ask ``low_rank_estimator_for``: the narrow kernel where it covers the shape, else the
    wide one, else neither — over the edges of both kernels' limits (the predicates are host code)."""
    from nutpie_amd import _lib

    seen = set()
    for dim in (1, 31, 32, 256, 512, 513, 1024, 1025):
        for n_pick in (1, 32, 33, 64, 65):
            for m in (1, 2, 40, 256):
                for k_max in (0, 1, 16, 17):
                    shape = (dim, m, n_pick, k_max)
                    narrow, wide = _lib.low_rank_estimate_supported(*shape), _lib.low_rank_estimate_wide_supported(*shape)
                    assert wide or not narrow, shape
                    want = _lib.low_rank_estimate if narrow else _lib.low_rank_estimate_wide if wide else None
                    assert _lib.low_rank_estimator_for(*shape) is want, shape
                    seen.add(getattr(want, "__name__", None))
                    inside = m >= 2 and n_pick <= min(m, dim) and 1 <= k_max <= 16   # the limits as include/nutpie_hip.h states them
                    assert narrow == (inside and dim <= 512 and n_pick <= 32) and wide == (inside and dim <= 1024 and n_pick <= 64), shape
    assert seen == {"low_rank_estimate", "low_rank_estimate_wide", None}
