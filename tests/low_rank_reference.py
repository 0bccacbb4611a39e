"""A high-precision restatement of the window estimator of ``adaptation="low_rank"`` and the cases the estimator kernel
(``nphip_low_rank_estimate``, nutpie_amd/csrc/lowrank_est.hip) is held to — TEST INFRASTRUCTURE.

:func:`reference` is sequential ``mpmath`` at 50 digits, written from the description in ``nutpie_amd/low_rank.py::estimate``'s docstring
and not from the kernel: moments over all ``m`` draws, the diagonal scaling with its fall-back, the basis rows from ``pick``, an
orthonormal basis of their span from the eigendecomposition of the Gram matrix, ``Cx`` and ``Cg`` with ``gamma I``, the geometric mean
``S = Cx # Cg^-1`` through symmetric square roots, its spectrum divided by the lower median over the span, the ``k_max`` eigenvalues
furthest from 1 in log scale among those outside ``[1 / cutoff, cutoff]``.  No rounding clamp on the spectrum: exact arithmetic needs
none.  An order-64 subspace problem takes most of a minute, so it runs ONCE, in tests/golden/make_low_rank_reference.py; the tests
read the ``.npz`` files that script writes.

CASES is plain data and importing this module does not import ``mpmath``.

The norm every error here is taken in (:func:`metric_error`): for ``D <= 64`` the dense metric ``M^-1 = D^1/2 (I + V (Lambda - I) V') D^1/2``,
max-abs difference over its largest element (a positive definite matrix has it on the diagonal); for larger ``D`` — a 512 x 512 matrix is
too large to commit — the worse of that figure for the diagonal and for the products with four fixed probe vectors (:func:`probes`),
each relative to its own largest element.
"""
from __future__ import annotations

import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
DENSE_MAX = 64      # the dense metric is stored up to this dimension
DPS = 50


def _case(name, D, m, b, seed, n_dir=3, factor=25.0, gamma=1e-5, cutoff=2.0, k_max=16, variant=None):
    return dict(name=name, D=D, m=m, b=b, seed=seed, n_dir=n_dir, factor=factor, gamma=gamma, cutoff=cutoff, k_max=k_max, variant=variant)


# (D, m, b): dimension, draws of the window, basis draws.  Inputs: window_problem(default_rng(seed), 1, m, D, n_dir, factor), then the
# variant.  A seed is whatever first met the conditions tests/test_low_rank_reference_cpu.py asserts on the fixture (no Gram eigenvalue or score
# near a threshold): a case that misses one gets another seed, never a looser condition.
CASES = [
    _case("smallest_1_2_1", 1, 2, 1, 1, n_dir=1),
    _case("smallest_2_3_2", 2, 3, 2, 2, n_dir=1),
    _case("tile_31_12_12", 31, 12, 12, 31),                 # the Gram tiles are 32 dimensions wide
    _case("tile_32_12_12", 32, 12, 12, 32),
    _case("tile_33_12_12", 33, 12, 12, 33),
    _case("fullrank_24_8_8", 24, 8, 8, 24),                 # 2b <= D: the basis has full rank (but for the centring)
    _case("fullrank_70_32_32", 70, 32, 32, 1002),
    _case("deficient_16_12_12", 16, 12, 12, 16),            # 2b > D
    _case("deficient_40_32_32", 40, 32, 32, 40),
    _case("square_64_32_32", 64, 32, 32, 2004, n_dir=1),   # 2b = D (with three strong directions no seed of 150 kept the Gram spectrum above 1e-6)
    _case("thinned_48_40_32", 48, 40, 32, 48),              # moments from 40 draws, basis from basis_pick(40, 32)
    _case("large_256_16_16", 256, 16, 16, 256),
    _case("large_512_6_6", 512, 6, 6, 512),
    _case("select_40_12_12_kmax16", 40, 12, 12, 140, n_dir=20, factor=1e4),   # more directions outside the cutoff than columns
    _case("select_24_10_10_kmax4", 24, 10, 10, 124, k_max=4),
    _case("select_24_10_10_kmax1", 24, 10, 10, 124, k_max=1),
    _case("cutoff100_24_10_10", 24, 10, 10, 124, cutoff=100.0),
    _case("gamma1e-3_24_10_10", 24, 10, 10, 124, gamma=1e-3),
    _case("gamma1_24_10_10", 24, 10, 10, 124, gamma=1.0),
    _case("repeated_rows_24_10_10", 24, 10, 10, 124, variant="repeated_rows"),   # rejected proposals: rows 5, 6, 7 repeat rows 0, 1, 2
    _case("offset_24_10_10", 24, 10, 10, 124, variant="offset"),                 # x * 1e-2 + 1e6, g * 1e2
    _case("scaled_24_10_10", 24, 10, 10, 124, variant="scaled"),                 # x * logspace(-6, 6, D), g / the same
    _case("constant_coordinate_24_10_10", 24, 10, 10, 124, variant="constant_coordinate"),   # x[:, 7] constant
]
CASE_NAMES = [c["name"] for c in CASES]
NO_COLUMNS_ALLOWED = ("smallest_1_2_1", "smallest_2_3_2", "cutoff100_24_10_10")


def case(name):
    return CASES[CASE_NAMES.index(name)]


def fixture_path(name):
    return os.path.join(GOLDEN, "low_rank_estimator_%s.npz" % name)


def load(name):
    with np.load(fixture_path(name)) as z:
        return {k: z[k] for k in z.files}


def window_problem(rng, n, m, D, n_dir, factor=25.0):
    """Draws and gradients [n, m, D] of n Gaussians with ``n_dir`` strong directions (tests/test_gpu_low_rank.py::_window_problem)."""
    B = rng.normal(size=(n, D, n_dir))
    scales = np.exp(rng.normal(size=(n, D)))
    Sigma = np.stack([np.diag(scales[c] ** 2) + factor * (scales[c][:, None] * B[c]) @ (scales[c][:, None] * B[c]).T for c in range(n)])
    x = np.stack([rng.multivariate_normal(np.zeros(D), Sigma[c], size=m) for c in range(n)]) + 2.0
    g = -np.stack([np.linalg.solve(Sigma[c], (x[c] - 2.0).T).T for c in range(n)])
    return x, g


def one_blas_thread():
    """A context in which the BLAS under numpy runs on one thread, where ``threadpoolctl`` is there to say so: the last bits of a large
    product or factorisation depend on how many threads share it, and the fixtures are generated under this."""
    try:
        from threadpoolctl import threadpool_limits
    except ImportError:
        import contextlib

        return contextlib.nullcontext()
    return threadpool_limits(limits=1)


def inputs(c):
    """The float64 window (x, g: [m, D]) of a case (the fixture stores it: its last bits at D = 256 and 512 are the BLAS's)."""
    with one_blas_thread():
        x, g = window_problem(np.random.default_rng(c["seed"]), 1, c["m"], c["D"], c["n_dir"], c["factor"])
    x, g = x[0].copy(), g[0].copy()
    v = c["variant"]
    if v == "repeated_rows":
        x[5:8], g[5:8] = x[0:3], g[0:3]
    elif v == "offset":
        x, g = x * 1e-2 + 1e6, g * 1e2
    elif v == "scaled":
        s = np.logspace(-6, 6, c["D"])
        x, g = x * s, g / s
    elif v == "constant_coordinate":
        x[:, 7] = x[0, 7]
    else:
        assert v is None, v
    return np.ascontiguousarray(x), np.ascontiguousarray(g)


def pick_of(m, b):
    from nutpie_amd import low_rank as lr

    p = lr.basis_pick(m, b)
    assert len(p) == b, (m, b, len(p))
    return p


def probes(D):
    """Four fixed probe vectors [4, D] with small integer entries (exact in any arithmetic, nothing to store)."""
    i = np.arange(D)
    return np.stack([((i * (2 * j + 3) + j) % 7 - 3).astype(np.float64) for j in range(4)])


def dense_metric(sigma2, V, lam):
    """M^-1 = D^1/2 (I + V (Lambda - I) V') D^1/2; V: [D, k]."""
    sd = np.sqrt(sigma2)
    return sd[:, None] * (np.eye(len(sigma2)) + (V * (lam - 1.0)) @ V.T) * sd[None, :]


def metric_summary(sigma2, V, lam):
    """What a fixture stores of a metric: {"dense"} up to DENSE_MAX dimensions, {"diag", "probe"} above."""
    sigma2, V, lam = np.asarray(sigma2, dtype=np.float64), np.asarray(V, dtype=np.float64), np.asarray(lam, dtype=np.float64)
    D = len(sigma2)
    if D <= DENSE_MAX:
        return {"dense": dense_metric(sigma2, V, lam)}
    sd = np.sqrt(sigma2)
    P = probes(D) * sd[None, :]                                       # [4, D]
    prod = (P + ((P @ V) * (lam - 1.0)) @ V.T) * sd[None, :]
    return {"diag": sigma2 * (1.0 + (V * V) @ (lam - 1.0)), "probe": prod}


def metric_error(got, want):
    """The relative max-abs error of a metric summary against the reference's (the module docstring has the norm)."""
    return max(float(np.abs(got[k] - want[k]).max() / np.abs(want[k]).max()) for k in want if k in ("dense", "diag", "probe"))


def reference(x, g, pick, gamma, cutoff, k_max, dps=DPS, intermediates=False):
    """The estimator of one chain's window in ``dps``-digit arithmetic on the float64 inputs taken as exact.  Returns a dict: the
    metric summary (float64), ``k``, ``scores`` (|log| of the re-centred spectrum over the span, descending), ``gram_ev`` (ascending,
    relative to the largest); with ``intermediates`` also ``Cx``, ``Cg`` and ``spectrum`` (of S, before re-centring) as float64."""
    import mpmath as mp

    x, g = np.asarray(x, dtype=np.float64), np.asarray(g, dtype=np.float64)
    m, D = x.shape
    b = len(pick)
    with mp.workdps(dps):
        f = mp.mpf
        X = [[f(float(v)) for v in row] for row in x]
        G = [[f(float(v)) for v in row] for row in g]

        def moments(A, i):
            mu = mp.fsum(A[t][i] for t in range(m)) / m
            return mu, mp.sqrt(mp.fsum((A[t][i] - mu) ** 2 for t in range(m)) / (m - 1))

        s, mx, mg = [], [], []
        for i in range(D):
            mu_x, sd_x = moments(X, i)
            mu_g, sd_g = moments(G, i)
            si = mp.sqrt(sd_x / sd_g) if sd_g != 0 else f(1)
            if not (mp.isfinite(si) and si > 0):
                si = f(1)
            s.append(min(max(si, f("1e-10")), f("1e10")))
            mx.append(mu_x)
            mg.append(mu_g)
        # the basis rows: scaled centred draws, then scaled centred gradients
        Z = [[(X[t][i] - mx[i]) / s[i] for i in range(D)] for t in pick] + [[(G[t][i] - mg[i]) * s[i] for i in range(D)] for t in pick]
        r = 2 * b
        gram = mp.matrix(r, r)
        for i in range(r):
            for j in range(i, r):
                gram[i, j] = gram[j, i] = mp.fdot(Z[i], Z[j])
        ev, U = mp.eigsy(gram)
        ev = [ev[i] for i in range(r)]
        top = max(ev)
        keep = [i for i in range(r) if ev[i] > f("1e-10") * max(top, f("1e-300"))]
        rr = len(keep)
        out = {"gram_ev": np.array([float(e / top) if top > 0 else 0.0 for e in ev])}
        centre = f(1)
        lam, T, scores = [], None, []
        if rr:
            # coordinates of the basis rows in the orthonormal basis Q = Z' U ev^-1/2 of their span: Z Q = U ev^1/2
            P = mp.matrix(r, rr)
            for t in range(r):
                for j, kj in enumerate(keep):
                    P[t, j] = U[t, kj] * mp.sqrt(ev[kj])
            Px, Pg = P[0:b, :], P[b:r, :]
            Cx = Px.T * Px / b + gamma_eye(mp, gamma, rr)
            Cg = Pg.T * Pg / b + gamma_eye(mp, gamma, rr)
            eg, Ug = mp.eigsy(Cg)
            half = _scaled(mp, Ug, [mp.sqrt(eg[i]) for i in range(rr)])
            ihalf = _scaled(mp, Ug, [1 / mp.sqrt(eg[i]) for i in range(rr)])
            mid = half * Cx * half
            em, Um = mp.eigsy((mid + mid.T) / 2)
            S = ihalf * _scaled(mp, Um, [mp.sqrt(em[i]) for i in range(rr)]) * ihalf
            es, W = mp.eigsy((S + S.T) / 2)
            es = [es[i] for i in range(rr)]
            if intermediates:
                out["Cx"] = np.array([[float(Cx[i, j]) for j in range(rr)] for i in range(rr)])
                out["Cg"] = np.array([[float(Cg[i, j]) for j in range(rr)] for i in range(rr)])
                out["spectrum"] = np.array([float(e) for e in es])
            centre = mp.exp(sorted(mp.log(e) for e in es)[(rr - 1) // 2])     # the lower median
            es = [e / centre for e in es]
            score = [abs(mp.log(e)) for e in es]
            order = sorted(range(rr), key=lambda i: -score[i])
            scores = [score[i] for i in order]
            sel = [i for i in order if score[i] > mp.log(f(float(cutoff)))][:k_max]
            lam = [es[i] for i in sel]
            if sel:
                # V = Q W_sel = Z' (U ev^-1/2 W_sel)
                T = mp.matrix(r, len(sel))
                for t in range(r):
                    for c, i in enumerate(sel):
                        T[t, c] = mp.fsum(U[t, kj] / mp.sqrt(ev[kj]) * W[j, i] for j, kj in enumerate(keep))
        k = len(lam)
        V = [[mp.fdot([Z[t][i] for t in range(r)], [T[t, c] for t in range(r)]) for c in range(k)] for i in range(D)]
        sd = [si * mp.sqrt(centre) for si in s]
        lm1 = [l - 1 for l in lam]
        if D <= DENSE_MAX:
            out["dense"] = np.array([[float(sd[i] * sd[j] * ((1 if i == j else 0) + mp.fsum(V[i][c] * lm1[c] * V[j][c] for c in range(k))))
                                      for j in range(D)] for i in range(D)])
        else:
            out["diag"] = np.array([float(sd[i] ** 2 * (1 + mp.fsum(V[i][c] ** 2 * lm1[c] for c in range(k)))) for i in range(D)])
            prod = []
            for p in probes(D):
                ps = [f(float(p[i])) * sd[i] for i in range(D)]
                t = [mp.fdot(ps, [V[i][c] for i in range(D)]) * lm1[c] for c in range(k)]
                prod.append([float(sd[i] * (ps[i] + mp.fdot(V[i], t))) for i in range(D)])
            out["probe"] = np.array(prod)
        out["k"] = np.int64(k)
        out["scores"] = np.array([float(v) for v in scores])
    return out


def gamma_eye(mp, gamma, n):
    return mp.mpf(float(gamma)) * mp.eye(n)


def _scaled(mp, U, d):
    """U diag(d) U'"""
    n = U.rows
    A = mp.matrix(n, n)
    for j in range(n):
        for i in range(n):
            A[i, j] = U[i, j] * d[j]
    return A * U.T


def cpu_errors(x, g, c, want):
    """(err_numpy, err_torch): oracle/low_rank_estimator.py::estimate_chain and low_rank.estimate on the CPU against the reference."""
    import torch

    from nutpie_amd import low_rank as lr
    from oracle import low_rank_estimator as ref

    m, b = c["m"], c["b"]
    pick = pick_of(m, b)
    s2, V, lam = ref.estimate_chain(x, g, c["gamma"], c["cutoff"], c["k_max"], pick=pick)
    err_numpy = metric_error(metric_summary(s2, V, lam), want)
    T = lr.estimate(torch.as_tensor(x)[None], torch.as_tensor(g)[None], c["gamma"], c["cutoff"], k_max=c["k_max"], basis_draws=b if m > b else None)
    s2, Vr, lam = (t[0].numpy() for t in lr.metric_of(T))
    err_torch = metric_error(metric_summary(s2, Vr.T, lam), want)
    return err_numpy, err_torch
