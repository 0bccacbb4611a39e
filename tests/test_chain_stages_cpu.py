"""The CPU restatement of the chain stages' order contracts (oracle/nuts_oracle.cpp: oracle_chain_*; csrc/chain_scan.h, chain_matvec.h,
chain_linalg.h) against a sequential ``np.longdouble`` evaluation of the mathematics.  Every bound is elementwise and derived from the
number of roundings on the path to an element; none was fitted to what the code gives.  ``tests/test_gpu_chain_stages.py`` then holds
the device routines to the restatement bit for bit."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))

LD = np.longdouble
U = 2.0 ** -53



def test_long_double_is_wider_than_double():
    """the reference of this file is one only then (x86-64: a 64-bit significand)"""
    assert np.finfo(LD).eps <= 2.0 ** -63


# --------------------------------------------------------------------------- scan
def scan_reference(a, b, init):
    """(x, X) in long double, sequentially: x_t = a_t x_{t-1} + b_t and the same recurrence on absolute values."""
    a, b = np.broadcast_to(np.asarray(a, dtype=LD), np.shape(b)), np.asarray(b, dtype=LD)
    x, X = np.empty_like(b), np.empty_like(b)
    p, P = LD(init), abs(LD(init))
    for t in range(b.shape[-1]):
        p = a[t] * p + b[t]
        P = abs(a[t]) * P + abs(b[t])
        x[t], X[t] = p, P
    return x, X


def scan_bound(X):
    """|xhat_t - x_t| <= 2 (t + 2) u X_t.

    x_t is the composition of the t + 1 affine maps (a_s, b_s), s <= t, applied to init.  Whatever the bracketing (lanes, waves,
    segments), every b_s and init reach x_t through at most t + 2 rounded operations: one per composition or application on the way
    (a composition (A2 A1, fma(A2, B1, B2)) rounds each component once; composing the identity rounds nothing), and every partial
    product of a's through at most t.  So each term of x_t = sum_s (prod_{s < r <= t} a_r) b_s + (prod a) init is computed with a
    relative error of at most gamma_{t+2} = (t + 2) u / (1 - (t + 2) u) <= 2 (t + 2) u, and the terms' absolute values sum to X_t,
    the recurrence on absolute values: the running-error bound of a sum of products."""
    t = np.arange(X.shape[-1])
    return 2.0 * (t + 2) * U * X


def coefficient_sets(rng, T):
    return {"tanh": np.tanh(rng.normal(size=T)), "one": 1, "wide": rng.uniform(-1.5, 1.5, T), "near_one": 1.0 - 1e-4 * rng.uniform(size=T)}


@pytest.mark.parametrize("T", [1, 63, 64, 65, 257, 2000, 100003])
def test_scan_restatement_within_the_running_error_bound(oracle, T):
    rng = np.random.default_rng(T)
    worst = 0.0
    for name, a in coefficient_sets(rng, T).items():
        b, init = rng.normal(size=T), float(rng.normal())
        x, X = scan_reference(a, b, init)
        bound = scan_bound(X)
        for W in (1, 2, 4):
            got = oracle.chain_scan(b, a, init, waves=W)
            err = np.abs(got.astype(LD) - x)
            ratio = float(np.max(err / bound))
            print(f"T={T} a={name} W={W}: worst error / bound = {ratio:.3f}")
            worst = max(worst, ratio)
            assert np.all(err <= bound), (name, W, ratio)
            if name == "one":
                # the a = 1 variant adds, the array variant fed ones goes through fma(1, x, b) and 1 * 1: the same real numbers, not the
                # same roundings at the identity compositions (-0.0 + 0.0 against fma(1, 0, -0.0)); to the bound, not bit for bit
                arr = oracle.chain_scan(b, np.ones(T), init, waves=W)
                assert np.all(np.abs(arr.astype(LD) - x) <= bound), W
    assert worst <= 1.0


def test_scan_rows_and_inits(oracle):
    rng = np.random.default_rng(5)
    R, T = 3, 130
    a, b, init = np.tanh(rng.normal(size=(R, T))), rng.normal(size=(R, T)), rng.normal(size=R)
    for W in (1, 2, 4):
        got = oracle.chain_scan(b, a, init, waves=W)
        for r in range(R):
            assert np.array_equal(got[r], oracle.chain_scan(b[r], a[r], float(init[r]), waves=W))
        s = oracle.chain_scan(b, 0.7, 0.25, waves=W)
        for r in range(R):
            x, X = scan_reference(0.7, b[r], 0.25)
            assert np.all(np.abs(s[r].astype(LD) - x) <= scan_bound(X))


@pytest.mark.parametrize("T", [1, 2, 64, 65, 257, 1030])
@pytest.mark.parametrize("W", [1, 2, 4])
def test_scan_adjoint_is_the_forward_scan_on_the_flipped_shifted_row(oracle, T, W):
    rng = np.random.default_rng(T + W)
    a, xbar = np.tanh(rng.normal(size=(2, T))), rng.normal(size=(2, T))
    lam = oracle.chain_scan(xbar, a, waves=W, rev=True)
    shifted = np.concatenate([np.zeros((2, 1)), a[:, :0:-1]], axis=1)      # reversed position t carries a_{T-t}; the first one 0
    fwd = oracle.chain_scan(xbar[:, ::-1], shifted, 0.0, waves=W)
    assert np.array_equal(lam, fwd[:, ::-1])
    # and it is the adjoint: lambda_t = a_{t+1} lambda_{t+1} + xbar_t
    x, X = scan_reference(shifted[0], xbar[0, ::-1], 0.0)
    assert np.all(np.abs(lam[0, ::-1].astype(LD) - x) <= scan_bound(X))
    s = oracle.chain_scan(xbar, 0.9, waves=W, rev=True)
    sf = oracle.chain_scan(xbar[:, ::-1], np.concatenate([np.zeros((2, 1)), np.full((2, T - 1), 0.9)], axis=1), 0.0, waves=W)
    assert np.array_equal(s, sf[:, ::-1])
    one = oracle.chain_scan(xbar, 1, waves=W, rev=True)
    assert np.array_equal(one, oracle.chain_scan(xbar[:, ::-1], 1, 0.0, waves=W)[:, ::-1])


def test_scan_zero_coefficient_resets(oracle):
    """a_t = 0 cuts the row: everything from t on is the scan of the tail alone, whatever came before — a wrong partner shows."""
    rng = np.random.default_rng(11)
    T = 700
    a, b = np.tanh(rng.normal(size=T)), rng.normal(size=T)
    for cut in (1, 63, 64, 65, 128, 255, 256, 257, 511, 513):
        a2 = a.copy()
        a2[cut] = 0.0
        for W in (1, 2, 4):
            got = oracle.chain_scan(b, a2, 3.0, waves=W)
            other = oracle.chain_scan(b * np.where(np.arange(T) < cut, 17.0, 1.0), a2, -5.0, waves=W)
            assert np.array_equal(got[cut:], other[cut:]), (cut, W)


# --------------------------------------------------------------------------- products
@pytest.mark.parametrize("n,K,R", [(1, 1, 1), (65, 7, 3), (300, 64, 1), (257, 257, 2), (2000, 200, 4), (33, 1025, 16)])
def test_products_within_the_dot_product_bound(oracle, n, K, R):
    """|ehat - e| <= K u sum |x| |b| (n in place of K for the transpose): one accumulator, one fma — one rounding — per summed index."""
    rng = np.random.default_rng(n + K)
    X, B, G = rng.normal(size=(n, K)), rng.normal(size=(K, R)), rng.normal(size=(n, R))
    E = oracle.chain_times(X, B)
    ref = X.astype(LD) @ B.astype(LD)
    assert np.all(np.abs(E.astype(LD) - ref) <= K * U * (np.abs(X) @ np.abs(B)))
    Ct = oracle.chain_times_t(X, G)
    ref = X.T.astype(LD) @ G.astype(LD)
    assert np.all(np.abs(Ct.astype(LD) - ref) <= n * U * (np.abs(X.T) @ np.abs(G)))


def test_products_are_each_other_transposed(oracle):
    """With one right-hand side, X B sums over the columns of X in ascending order and (X^T)^T G over the rows of X^T: the same
    accumulator, the same fma operands (a product does not depend on the order of its factors) — bitwise equal."""
    rng = np.random.default_rng(2)
    X, v = rng.normal(size=(130, 77)), rng.normal(size=(77, 1))
    assert np.array_equal(oracle.chain_times(X, v), oracle.chain_times_t(np.ascontiguousarray(X.T), v))


# --------------------------------------------------------------------------- Cholesky and substitutions
from chain_stage_probes import spd  # noqa: E402  (the matrices the GPU probes use)


def chol_reference(A):
    A = np.asarray(A, dtype=LD)
    K = len(A)
    L = np.zeros((K, K), dtype=LD)
    for j in range(K):
        L[j, j] = np.sqrt(A[j, j] - L[j, :j] @ L[j, :j])
        for i in range(j + 1, K):
            L[i, j] = (A[i, j] - L[i, :j] @ L[j, :j]) / L[j, j]
    return L


def solve_reference(L, B):
    L, B = np.asarray(L, dtype=LD), np.asarray(B, dtype=LD)
    X = np.zeros_like(B)
    for i in range(len(L)):
        X[i] = (B[i] - L[i, :i] @ X[:i]) / L[i, i]
    return X


KS = [1, 2, 3, 4, 5, 8, 15, 16, 17, 31, 32]


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("cond", [None, 1e12])
def test_cholesky_backward_error(oracle, K, cond):
    """||Lhat Lhat^T - A||_F <= (K + 1) u ||A||_F (Higham, Accuracy and Stability, thm 10.3: |A - Lhat Lhat^T| <= gamma_{K+1} |Lhat||Lhat^T|
    elementwise, and for a positive definite A the entries of |Lhat||Lhat^T| are bounded by sqrt(a_ii a_jj) up to O(u))."""
    A = spd(np.random.default_rng(K), K, cond)
    L, ok = oracle.chain_cholesky(A)
    assert ok and np.all(np.triu(L, 1) == 0) and not np.signbit(np.triu(L, 1)).any()
    Ll = L.astype(LD)
    res = np.linalg.norm((Ll @ Ll.T - A.astype(LD)).astype(np.float64))
    print(f"K={K} cond={cond}: residual / bound = {res / ((K + 1) * U * np.linalg.norm(A)):.3f}")
    assert res <= (K + 1) * U * np.linalg.norm(A)
    # only the lower triangle is read
    A2 = A.copy()
    A2[np.triu_indices(K, 1)] = np.nan
    assert np.array_equal(oracle.chain_cholesky(A2)[0], L)


@pytest.mark.parametrize("pivot", [-0.0, 0.0, np.nan, np.inf, -1.0])
def test_cholesky_bad_pivot_is_all_nan(oracle, pivot):
    A = spd(np.random.default_rng(0), 5)
    A[3, 3] = pivot
    L, ok = oracle.chain_cholesky(A)
    assert not ok and np.isnan(L).all()


def test_cholesky_subnormal_pivot_factors(oracle):
    L, ok = oracle.chain_cholesky(np.array([[5e-324, 0.0], [0.0, 1.0]]))
    assert ok and L[0, 0] == np.sqrt(5e-324) and L[1, 1] == 1.0 and L[1, 0] == 0.0


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("N", [1, 2, 63, 64, 65, 85, 128, 129])
def test_substitutions_backward_error(oracle, K, N):
    """|Lhat xhat - b| <= K u |Lhat| |xhat| elementwise (Higham thm 8.5: the computed solution solves a system with |dL| <= gamma_K |L|;
    an fma per term rounds once), for both substitutions and both layouts of the transposed one."""
    rng = np.random.default_rng(K * 1000 + N)
    L = oracle.chain_cholesky(spd(rng, K, 1e12 if (K + N) % 2 else None))[0]
    B = rng.normal(size=(K, N))
    Ll = L.astype(LD)
    X = oracle.chain_solve_lower(L, B)
    assert np.all(np.abs(Ll @ X.astype(LD) - B) <= K * U * (np.abs(L) @ np.abs(X)))
    Y = oracle.chain_solve_lower_t(L, B)
    assert np.all(np.abs(Ll.T @ Y.astype(LD) - B) <= K * U * (np.abs(L.T) @ np.abs(Y)))
    Yr = oracle.chain_solve_lower_t(L, np.ascontiguousarray(B.T), by_rows=True)
    assert np.array_equal(Yr, Y.T)   # the same operations on another layout


def central(f, P, h):
    """central differences of the scalar f at P (long double), element by element"""
    D = np.zeros(P.shape, dtype=LD)
    for idx in np.ndindex(*P.shape):
        Pp, Pm = P.copy(), P.copy()
        Pp[idx] += h
        Pm[idx] -= h
        D[idx] = (f(Pp) - f(Pm)) / (2 * h)
    return D


def fd_check(got, f, P, mask, rounding):
    """``got`` against the central differences of f with step h.  The tolerance is computed, not picked: the truncation error of D_h is
    h^2 f''' / 6 + O(h^4), so D_h - D_{h/2} = (3/4) of it and 4/3 |D_h - D_{h/2}| estimates it (Richardson); the difference quotient
    itself is rounded in long double, 2 u_ld |f| / h; ``rounding`` is the double-precision error of the adjoint under test."""
    h = LD(2.0) ** -16
    D1, D2 = central(f, P, h), central(f, P, h / 2)
    tol = 4.0 / 3.0 * np.abs(D1 - D2) + 2 * np.finfo(LD).eps * abs(f(P)) / h + rounding
    err = np.abs(got.astype(LD) - D1)
    assert np.all(err[mask] <= tol[mask]), float(np.max(err[mask] / tol[mask]))


@pytest.mark.parametrize("K,N", [(1, 1), (3, 2), (5, 7), (8, 65)])
def test_solve_adjoint_against_central_differences(oracle, K, N):
    rng = np.random.default_rng(K + N)
    L = oracle.chain_cholesky(spd(rng, K))[0]
    B, Xbar = rng.normal(size=(K, N)), rng.normal(size=(K, N))
    X = oracle.chain_solve_lower(L, B)
    Bbar = oracle.chain_solve_lower_t(L, Xbar)
    Lbar = oracle.chain_solve_lower_adj_l(Bbar, X)
    assert np.all(np.triu(Lbar, 1) == 0)
    f = lambda Lp: np.sum(Xbar.astype(LD) * solve_reference(np.tril(Lp), B))  # noqa: E731
    # forward error of the two substitutions and the N-term dot products: (2 K kappa(L) + N) u on the entries' scale
    rounding = (2 * K * np.linalg.cond(L) + N) * U * (np.abs(Bbar) @ np.abs(X.T))
    fd_check(Lbar, f, L.astype(LD), np.tril(np.ones((K, K), bool)), rounding)


@pytest.mark.parametrize("K", [1, 2, 3, 5, 8])
def test_cholesky_adjoint_against_central_differences(oracle, K):
    """f(A) = sum(Lbar * chol(A)) with only the lower triangle of A read and a NON-symmetric Lbar (its upper triangle must not count)."""
    rng = np.random.default_rng(K)
    A = spd(rng, K)
    L = oracle.chain_cholesky(A)[0]
    Lbar = rng.normal(size=(K, K))
    Abar = oracle.chain_cholesky_adj(L, Lbar)
    assert np.all(np.triu(Abar, 1) == 0) and not np.signbit(np.triu(Abar, 1)).any()
    assert np.array_equal(Abar, oracle.chain_cholesky_adj(L, np.tril(Lbar)))

    def f(Ap):
        S = np.tril(Ap) + np.tril(Ap, -1).T
        return np.sum(np.tril(Lbar).astype(LD) * chol_reference(S))

    # two substitutions with K right-hand sides each, on a matrix of the size of L^-T |Phi| L^-1
    Li = np.abs(np.linalg.inv(L))
    rounding = 4 * K * np.linalg.cond(L) * U * (Li.T @ (np.abs(L.T) @ np.abs(np.tril(Lbar))) @ Li)
    rounding = rounding + rounding.T
    fd_check(Abar, f, A.astype(LD), np.tril(np.ones((K, K), bool)), rounding)


# --------------------------------------------------------------------------- the probes of tests/test_gpu_chain_stages.py
def _probe_ids():
    import chain_stage_probes as P

    return P.PROBES


@pytest.mark.parametrize("family,W", _probe_ids())
def test_probe_compiles_for_gfx950(oracle, family, W):
    import chain_stage_probes as P

    probe = P.probe(family, W)
    assert os.path.exists(probe.model.library_path())
    # every case in device memory, and in LDS wherever its arrays fit
    dev = {c.name for c in probe.cases if c.mem == "dev"}
    lds = {c.name for c in probe.cases if c.mem == "lds"}
    assert dev == {c.name for c in probe.cases} and lds == {c.name for c in probe.cases if c.doubles <= P.LDS_DOUBLES} and lds


def test_expand_probe_compiles_for_gfx950():
    import chain_stage_probes as P

    model, _ = P.expand_probe()
    assert "__device__ double nphip_expand(" in model._source and os.path.exists(model.library_path())


def test_probe_lists_hold_the_boundaries():
    import chain_stage_probes as P

    for W in (1, 2, 4):
        S = 64 * W
        Ts = {int(c.name.split("T=")[1].split()[0]) for c in P.probe("scan", W).cases}
        assert Ts >= {1, 2, 63, 64, 65, S - 1, S, S + 1, 4 * S - 1, 4 * S, 4 * S + 1, 8 * S + 1, 2000, 20000, 100003}
        names = " ".join(c.name for c in P.probe("scan", W).cases)
        for word in ("A_ARRAY", "A_SCALAR", "A_ONE", "rev=True", "rev=False", "init=const", "init=scalar", "init=row", "R=1 ", "R=3 ", "R=8 ",
                     "a=tanh", "a=sprinkled", "a=negative", "a=above_one"):
            assert word in names, (W, word)
        multi = [c for c in P.probe("scan", W).cases if f"R=3 T={8 * S + 1} " in c.name]
        assert {("rev=True" in c.name) for c in multi} == {False, True} and any("A_ARRAY" in c.name for c in multi)
        shapes = P.matvec_shapes(W)
        assert {n for n, _, _ in shapes} >= {1, 63, 64, 65, 4 * S - 1, 4 * S, 4 * S + 1, 2000, 20000}
        assert {K for _, K, _ in shapes} >= {1, 7, 8, 9, 63, 64, 65, S - 1, S, S + 1, 200, 4 * S, 4 * S + 1, 600}
        assert {R for _, _, R in shapes} == {1, 2, 3, 4, 15, 16}
    names = [c.name for c in P.probe("linalg", 1).cases]
    for K in P.LINALG_K:
        for routine in ("cholesky", "cholesky_adj", "solve_lower", "solve_lower_t columns", "solve_lower_t rows", "solve_lower_adj_l"):
            assert any(n.startswith(f"{routine} K={K} ") for n in names), (routine, K)
    for N in P.LINALG_N:
        Ks = {int(n.split("K=")[1].split()[0]) for n in names if n.endswith(f" N={N}")}
        assert min(Ks) <= 5 and max(Ks) >= 17, (N, Ks)


def test_prebuild_script_lists_the_probes():
    src = open(os.path.join(os.path.dirname(__file__), "prebuild_density_cache.py")).read()
    assert "chain_stage_probes" in src and "PROBES" in src and "expand_probe" in src


# --------------------------------------------------------------------------- the two sets of wave totals of the scan (W > 1)
def _two_sets_problems(src: str) -> list:
    """What the text of chain_scan.h must say for the wave totals of successive groups of four segments to go to two LDS sets in turn.
    A wave may still read a group's totals while another one, past the same barrier, already writes the next group's: with one set that
    is a write-after-read race which needs a wave to lag a whole group behind, and no input of a device test brings that about (tried:
    with the flip removed the device tests passed in one run and two of them failed in another — by chance, nothing to rely on).  So the alternation is pinned here, on the source, and nowhere on the device."""
    import re

    bad = []
    if not re.search(r"__shared__ double tot_\[NPHIP_JIT_W > 1 \? 2 \* U \* NPHIP_JIT_W \* 2 : 1\];", src):
        bad.append("tot_ does not hold two sets of U W (A, B) pairs")
    body = src[src.index("__device__ __forceinline__ void linear_recurrence("):]
    marks = ["int parity = 0;", "for (int r = 0; r < R; ++r) {", "for (int s0 = 0; s0 < T; s0 += U * SEG) {", "if constexpr (W > 1) {",
             "double* tot = tot_ + parity * (U * W * 2);", "tot[(u * W + wave) * 2] = A[u];", "nphip_chain_barrier();", "parity ^= 1;",
             "const double ta = tot[(u * W + w) * 2]", "} else {"]
    at = 0
    for m in marks:      # in this order: the set is chosen per group, written, the barrier, the flip, the reads — all inside the group loop
        nxt = body.find(m, at)
        if nxt < 0:
            bad.append(f"`{m}` is missing or out of order")
            break
        at = nxt + len(m)
    if len(re.findall(r"\bparity\b", body)) != 3:
        bad.append("parity is touched somewhere else")
    if body.count("nphip_chain_barrier();") != 2:
        bad.append("the barriers are not one per group and one at the end")
    return bad


def test_scan_wave_totals_use_two_sets_in_turn():
    src = open(os.path.join(os.path.dirname(__file__), "..", "nutpie_amd", "csrc", "chain_scan.h")).read()
    assert _two_sets_problems(src) == []
    # the check rejects the ways of losing the alternation
    for old, new in (("                parity ^= 1;\n", ""), ("parity ^= 1;", "parity ^= 0;"), ("tot_ + parity * (U * W * 2)", "tot_"),
                     ("? 2 * U * NPHIP_JIT_W * 2 : 1]", "? U * NPHIP_JIT_W * 2 : 1]"), ("    int parity = 0;\n    for (int r", "    for (int r")):
        assert old in src
        assert _two_sets_problems(src.replace(old, new)), (old, new)
    # ... and moving the flip out of the group loop
    moved = src.replace("                parity ^= 1;\n", "").replace("    nphip_chain_barrier();\n}\n\n}  // namespace nphip_scan", "    parity ^= 1;\n    nphip_chain_barrier();\n}\n\n}  // namespace nphip_scan")
    assert moved != src and _two_sets_problems(moved)
