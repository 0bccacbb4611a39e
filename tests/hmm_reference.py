"""The plain-C restatement of the HMM stages' order contract (tests/fixtures/hmm_reference.c), built with gcc and called
through ctypes, and the probe cases that reach csrc/chain_hmm.h directly (``chain_stage_probes.Probe`` / ``Case``).

Packed results: ``F = [alpha: R T K | c: R T | m: R T]``, ``B = [beta: R T K | w: R T K | Pbar: K K | pibar: K]``."""
from __future__ import annotations

import ctypes
import functools
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import chain_stage_probes as P  # noqa: E402


@functools.lru_cache(maxsize=None)
def lib():
    src, out = os.path.join(HERE, "fixtures", "hmm_reference.c"), os.path.join(HERE, "fixtures", "libhmm_reference.so")
    if not os.path.exists(out) or os.path.getmtime(out) < os.path.getmtime(src):
        subprocess.run(["gcc", "-O2", "-fPIC", "-shared", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"), "-o", out, src, "-lm"], check=True)
    so = ctypes.CDLL(out)
    dp = ctypes.POINTER(ctypes.c_double)
    so.hmm_forward.argtypes = [ctypes.c_int] * 3 + [dp] * 4
    so.hmm_backward.argtypes = [ctypes.c_int] * 3 + [dp] * 4
    so.hmm_forward.restype = so.hmm_backward.restype = None
    return so


def _ptr(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))


def _c(a, n):
    a = np.ascontiguousarray(a, dtype=np.float64).reshape(-1)
    assert a.size == n, (a.size, n)
    return a


def forward(logE, P_, pi, R, T, K):
    """F of one chain"""
    logE, P_, pi = _c(logE, R * T * K), _c(P_, K * K), _c(pi, K)
    F = np.empty(R * T * K + 2 * R * T)
    lib().hmm_forward(R, T, K, _ptr(logE), _ptr(P_), _ptr(pi), _ptr(F))
    return F


def backward(logE, P_, F, R, T, K):
    """B of one chain (with the adjoints of P and pi)"""
    logE, P_, F = _c(logE, R * T * K), _c(P_, K * K), _c(F, R * T * K + 2 * R * T)
    B = np.empty(2 * R * T * K + K * K + K)
    lib().hmm_backward(R, T, K, _ptr(logE), _ptr(P_), _ptr(F), _ptr(B))
    return B


def value(logE, P_, pi, R, T, K):
    """sum_r sum_t (log c_t + m_t), the log in numpy's double precision"""
    F = forward(logE, P_, pi, R, T, K)
    with np.errstate(all="ignore"):
        return float(np.sum(np.log(F[R * T * K:R * T * K + R * T]) + F[R * T * K + R * T:]))


# --------------------------------------------------------------------------- probe cases
HMM_K = [1, 2, 3, 4, 5, 8, 15, 16]
HMM_T = [1, 2, 3, 64, 65]


def group_lanes(K):
    return 1 if K <= 1 else 2 if K <= 2 else 4 if K <= 4 else 8 if K <= 8 else 16


def hmm_shapes(W):
    """The thinning rule.  With S = 64 W / G series side by side (G the group of K), the R classes are 1, 2, S - 1, S, S + 1, 2 S + 1
    (the last series of a pass, the first of the next, a ragged last pass; a lane carries two passes at once, so 2 S + 1 also
    starts a second round).  Every K meets every R class; the T of the list rotate so that every (K, R class) gets two of them,
    and T = 64 / 65 go to the small R only where R T K would pass 8 000 doubles."""
    shapes = []
    for a, K in enumerate(HMM_K):
        S = 64 * W // group_lanes(K)
        for b, R in enumerate([1, 2, S - 1, S, S + 1, 2 * S + 1]):
            if R < 1:
                continue
            for h in (0, 2):
                T = HMM_T[(a + b + h + W) % len(HMM_T)]
                if R * T * K > 8_000:
                    T = HMM_T[(a + b + h) % 3]
                if (R, T, K) not in shapes:
                    shapes.append((R, T, K))
    return shapes


def hmm_cases(W):
    """One case per shape runs ``forward``, ``backward`` and ``transition_adjoint`` in a row (P in p0; logE in p1: scaled by the chain,
    poisoned by whole series; pi in p2, scaled) and stores [F | B]; device memory, and LDS where the arrays fit."""
    rng = np.random.default_rng(500 + W)
    cases = []
    shapes = hmm_shapes(W)
    # one case per W with logE of magnitude -2000 (it underflows without the shift by the step's maximum), one with an impossible state
    far = next(k for k, (R, T, K) in enumerate(shapes) if K >= 3 and T >= 64)
    column = next(k for k, (R, T, K) in enumerate(shapes) if K >= 2 and T >= 3 and k != far)
    for k, (R, T, K) in enumerate(shapes):
        logE = 3.0 * rng.normal(size=(R, T, K))
        tag = ""
        if k == far:
            logE = 30.0 * rng.normal(size=(R, T, K)) - 2000.0
            tag = " logE~-2000"
        if k == column:
            logE[:, :, K - 1] = -np.inf
            tag = " -inf column"
        Pm = rng.uniform(0.1, 1.0, size=(K, K))
        pi = rng.uniform(0.1, 1.0, size=K)
        n_f, n_b = R * T * K + 2 * R * T, 2 * R * T * K + K * K + K
        call = (f"nphip_hmm::forward<{R}, {T}, {K}>(P1, P0, P2, PO, lane); "
                f"nphip_hmm::backward<{R}, {T}, {K}>(P1, P0, PO, PO + {n_f}, lane); "
                f"nphip_hmm::transition_adjoint<{R}, {T}, {K}>(PO, PO + {n_f}, lane);")

        def run(p0, p1, p2, R=R, T=T, K=K):
            with np.errstate(all="ignore"):
                F = forward(p1, p0, p2, R, T, K)
                return np.concatenate([F, backward(p1, p0, F, R, T, K)])

        cases.append(P.Case(f"hmm R={R} T={T} K={K}{tag}", call, Pm, logE, pi, n_f + n_b, run, poison=(R // 2, T * K)))
    return P.with_lds(cases)


@functools.lru_cache(maxsize=None)
def probe(W: int) -> P.Probe:
    return P.Probe(f"hmm W={W}", W, ["chain_hmm.h"], hmm_cases(W))


def split(case: P.Case, flat):
    """(alpha, c, m, beta, w, Pbar, pibar) of one chain's output of a case"""
    R, T, K = case.p1.shape
    cuts = np.cumsum([R * T * K, R * T, R * T, R * T * K, R * T * K, K * K])
    a, c, m, b, w, Pb, pb = np.split(np.asarray(flat), cuts)
    return a.reshape(R, T, K), c.reshape(R, T), m.reshape(R, T), b.reshape(R, T, K), w.reshape(R, T, K), Pb, pb
