"""The cases only the wide estimator kernel (``nphip_low_rank_estimate_wide``, nutpie_amd/csrc/lowrank_est_wide.hip) covers: more than
32 basis draws or more than 512 dimensions — TEST INFRASTRUCTURE.  The reference, the norm and the two CPU formulations are those of
tests/low_rank_reference.py, unchanged; this module adds a case table, inputs that regenerate bit for bit, and the fixtures
tests/golden/low_rank_estimator_wide_<case>.npz (written by tests/golden/make_low_rank_reference_wide.py).

A window of 64 x 1024 doubles is too large to commit, and a window drawn through numpy's BLAS does not reproduce its last bits.  So the
inputs here are built from small integers of an explicit 64-bit mixing function (splitmix64's finaliser in ``uint64`` arithmetic, no
``Generator`` stream) by element-wise IEEE operations whose every intermediate is exactly representable — sums of a few small integers
times 0 / +-1 direction entries, added in a Python loop over the directions, times a power of two per coordinate: no BLAS, no library
reduction, the same bits on every machine.  The fixture stores the SHA-256 of the two arrays and the tests compare it.

    x[t, i] = 2^(e_i - 2) (n[t, i] + F sum_j B[i, j] a[t, j] + 8)        g[t, i] = -2^(-e_i - 2) (n[t, i] + h[t, i])

with integers |n|, |h| <= 12 (sums of three of -4 .. 4), |a| <= 8, B in {-1, 0, 1}, F a small integer: draws and gradients share the
noise n and the draws carry ``n_dir`` strong directions more.  These are not gradients of a density, and need not be: what the
estimator sees is a pair of windows whose scaled rows span a subspace with directions far from 1.  The quarter in both keeps
std(x) std(g) of a coordinate near 1, as tests/low_rank_reference.py::window_problem has it: the formulation's condition number grows with
|Cx| |Cg| / gamma^2, and with entries ten times as large both float64 formulations on the CPU were 10 % away from the exact metric.

Importing this module does not import ``mpmath``.
"""
from __future__ import annotations

import hashlib
import os

import numpy as np

from tests.low_rank_reference import GOLDEN, cpu_errors, metric_error, metric_summary, pick_of, probes, reference  # noqa: F401

U64 = np.uint64


def _case(name, D, m, b, seed, n_dir=3, factor=2, gamma=1e-5, cutoff=2.0, k_max=16, variant=None):
    return dict(name=name, D=D, m=m, b=b, seed=seed, n_dir=n_dir, factor=factor, gamma=gamma, cutoff=cutoff, k_max=k_max, variant=variant)


# (D, m, b) as in tests/low_rank_reference.py.  Every D is above 64: the fixtures hold the diagonal and the probe products.  A seed is
# the first that met the conditions tests/test_low_rank_reference_wide_cpu.py asserts (another seed otherwise, never a looser condition).
CASES = [
    _case("past_narrow_80_33_33", 80, 33, 33, 3),                   # one basis draw more than the narrow kernel takes
    _case("full_160_64_64", 160, 64, 64, 5),                        # the whole order-128 subspace, 2b < D
    _case("rows_100_64_64", 100, 64, 64, 1),                        # 2b > D: more basis rows than dimensions
    _case("thinned_200_80_64", 200, 80, 64, 4),                     # moments from 80 draws, basis from basis_pick(80, 64)
    _case("tile_159_40_40", 159, 40, 40, 7),                        # the Gram tiles are 32 dimensions wide
    _case("tile_160_40_40", 160, 40, 40, 10),
    _case("tile_161_40_40", 161, 40, 40, 1),
    _case("large_513_40_40", 513, 40, 40, 2),                       # one dimension more than the narrow kernel takes
    _case("large_1024_64_64", 1024, 64, 64, 4),                     # the limit
    _case("select_80_33_33_kmax4", 80, 33, 33, 3, k_max=4),
    _case("select_80_33_33_kmax1", 80, 33, 33, 3, k_max=1),
    _case("cutoff100_80_33_33", 80, 33, 33, 2, cutoff=100.0),       # fewer than k_max columns
    _case("gamma1e-3_80_33_33", 80, 33, 33, 3, gamma=1e-3),
    _case("constant_coordinate_80_33_33", 80, 33, 33, 3, variant="constant_coordinate"),   # x[:, 7] constant
    _case("repeated_rows_80_33_33", 80, 33, 33, 3, variant="repeated_rows"),               # rows 5, 6, 7 repeat rows 0, 1, 2
    _case("scaled_80_33_33", 80, 33, 33, 3, variant="scaled"),                             # 2^e_i over 2^-20 .. 2^20: twelve orders
]
CASE_NAMES = [c["name"] for c in CASES]
NO_COLUMNS_ALLOWED = ("cutoff100_80_33_33",)


def case(name):
    return CASES[CASE_NAMES.index(name)]


def fixture_path(name):
    return os.path.join(GOLDEN, "low_rank_estimator_wide_%s.npz" % name)


def load(name):
    with np.load(fixture_path(name)) as z:
        return {k: z[k] for k in z.files}


def _mix(a):
    """splitmix64's finaliser on a ``uint64`` array (the arithmetic wraps modulo 2^64)."""
    a = (a ^ (a >> U64(30))) * U64(0xBF58476D1CE4E5B9)
    a = (a ^ (a >> U64(27))) * U64(0x94D049BB133111EB)
    return a ^ (a >> U64(31))


def small_ints(seed, stream, shape, lo, hi):
    """Integers in [lo, hi] as float64, a fixed function of (seed, stream, position)."""
    n = int(np.prod(shape))
    key = _mix(np.array([(seed * 0x9E3779B97F4A7C15 + stream * 0xD1B54A32D192ED03 + 1) % 2**64], dtype=U64))
    h = _mix(_mix(np.arange(n, dtype=U64) * U64(0x9E3779B97F4A7C15) + key) ^ key)
    v = (h >> U64(33)) % U64(hi - lo + 1)
    return (v.astype(np.int64) + lo).astype(np.float64).reshape(shape)


def inputs(c):
    """The float64 window (x, g: [m, D]) of a case, bit for bit on every machine (the module docstring has the construction)."""
    m, D, seed, n_dir, F = c["m"], c["D"], c["seed"], c["n_dir"], float(c["factor"])
    tri = lambda s: small_ints(seed, s, (m, D), -4, 4) + small_ints(seed, s + 1, (m, D), -4, 4) + small_ints(seed, s + 2, (m, D), -4, 4)  # noqa: E731
    n, h = tri(10), tri(20)
    a = small_ints(seed, 30, (m, n_dir), -8, 8)
    B = small_ints(seed, 31, (D, n_dir), -1, 1)
    span = 20 if c["variant"] == "scaled" else 2
    e = small_ints(seed, 32, (D,), -span, span)
    if c["variant"] == "scaled":
        e[0], e[D - 1] = -20.0, 20.0
    strong = np.zeros((m, D))
    for j in range(n_dir):                          # (integers below 2^10: every sum exact)
        strong = strong + a[:, j][:, None] * B[:, j][None, :]
    s = np.ldexp(1.0, e.astype(np.int64))
    x = (n + F * strong + 8.0) * (0.25 * s)[None, :]
    g = -(n + h) * (0.25 / s)[None, :]
    v = c["variant"]
    if v == "repeated_rows":
        x[5:8], g[5:8] = x[0:3], g[0:3]
    elif v == "constant_coordinate":
        x[:, 7] = x[0, 7]
    else:
        assert v in (None, "scaled"), v
    return np.ascontiguousarray(x), np.ascontiguousarray(g)


def digest(x, g):
    return hashlib.sha256(np.ascontiguousarray(x).tobytes() + np.ascontiguousarray(g).tobytes()).hexdigest()


def screen(x, g, pick, gamma):
    """(gram_ev relative ascending, scores descending) in float64 with LAPACK: what the generator looks at before it spends minutes
    of 50-digit arithmetic on a seed.  Only the Gram condition is meaningful at this precision; the scores are a first look."""
    m, D = x.shape
    b = len(pick)
    cx, cg = (x == x[0]).all(0), (g == g[0]).all(0)
    sx, sg = np.where(cx, 0.0, x.std(0, ddof=1)), np.where(cg, 0.0, g.std(0, ddof=1))
    with np.errstate(divide="ignore", invalid="ignore"):
        s = np.sqrt(sx / sg)
    s = np.where(np.isfinite(s) & (s > 0), s, 1.0).clip(1e-10, 1e10)
    Z = np.concatenate([((x - x.mean(0)) / s)[pick], ((g - g.mean(0)) * s)[pick]], 0)
    ev, U = np.linalg.eigh(Z @ Z.T)
    keep = ev > 1e-10 * ev.max()
    P = U[:, keep] * np.sqrt(ev[keep])
    r = int(keep.sum())
    Cx, Cg = P[:b].T @ P[:b] / b + gamma * np.eye(r), P[b:].T @ P[b:] / b + gamma * np.eye(r)
    eg, Ug = np.linalg.eigh(Cg)
    half, ihalf = (Ug * np.sqrt(eg)) @ Ug.T, (Ug / np.sqrt(eg)) @ Ug.T
    em, Um = np.linalg.eigh(half @ Cx @ half)
    S = ihalf @ (Um * np.sqrt(np.maximum(em, 0))) @ Um.T @ ihalf
    es = np.maximum(np.linalg.eigvalsh(0.5 * (S + S.T)), 1e-300)
    le = np.log(es)
    le = le - np.sort(le)[(r - 1) // 2]
    return ev / ev.max(), np.sort(np.abs(le))[::-1]
