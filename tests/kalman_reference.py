"""The plain-C restatement of the Kalman filter stages' order contract (tests/fixtures/kalman_reference.c), built with gcc
and called through ctypes, and the probe cases that reach csrc/chain_kalman.h directly (``chain_stage_probes.Probe`` / ``Case``).

Packed results: ``F = [apred: R T m | Ppred: R T m m | afilt: R T m | v: R T | F: R T]``,
``B = [ybar: R T | hbar: R T | Zbar: R T m | Tbar: m m | Qbar: m m | a0bar: m | P0bar: m m | partials: R (3 m m + m)]``."""
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
    src, out = os.path.join(HERE, "fixtures", "kalman_reference.c"), os.path.join(HERE, "fixtures", "libkalman_reference.so")
    if not os.path.exists(out) or os.path.getmtime(out) < os.path.getmtime(src):
        subprocess.run(["gcc", "-O2", "-fPIC", "-shared", "-ffp-contract=off", "-o", out, src, "-lm"], check=True)
    so = ctypes.CDLL(out)
    dp = ctypes.POINTER(ctypes.c_double)
    so.kalman_forward.argtypes = [ctypes.c_int] * 4 + [dp] * 9
    so.kalman_backward.argtypes = [ctypes.c_int] * 4 + [dp] * 10
    so.kalman_forward.restype = so.kalman_backward.restype = None
    return so


def _ptr(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))


def _c(a, n):
    a = np.ascontiguousarray(a, dtype=np.float64).reshape(-1)
    assert a.size == n, (a.size, n)
    return a


def sizes(R, T, m):
    """the lengths of F and B"""
    return R * T * (2 * m + m * m + 2), R * T * (2 + m) + 3 * m * m + m + R * (3 * m * m + m)


def forward(y, obs, Z, h, Tm, Q, a0, P0, R, T, m):
    """F of one chain; ``obs`` None: no mask"""
    masked = obs is not None
    y, Z, h, Tm, Q, a0, P0 = _c(y, R * T), _c(Z, R * T * m), _c(h, R * T), _c(Tm, m * m), _c(Q, m * m), _c(a0, m), _c(P0, m * m)
    obs = _c(obs, R * T) if masked else np.ones(R * T)
    F = np.empty(sizes(R, T, m)[0])
    lib().kalman_forward(R, T, m, int(masked), _ptr(y), _ptr(obs), _ptr(Z), _ptr(h), _ptr(Tm), _ptr(Q), _ptr(a0), _ptr(P0), _ptr(F))
    return F


def backward(y, obs, Z, h, Tm, Q, F, vbar, Fbar, R, T, m):
    """B of one chain"""
    masked = obs is not None
    n_f, n_b = sizes(R, T, m)
    y, Z, h, Tm, Q, F = _c(y, R * T), _c(Z, R * T * m), _c(h, R * T), _c(Tm, m * m), _c(Q, m * m), _c(F, n_f)
    vbar, Fbar = _c(vbar, R * T), _c(Fbar, R * T)
    obs = _c(obs, R * T) if masked else np.ones(R * T)
    B = np.empty(n_b)
    lib().kalman_backward(R, T, m, int(masked), _ptr(y), _ptr(obs), _ptr(Z), _ptr(h), _ptr(Tm), _ptr(Q), _ptr(F), _ptr(vbar), _ptr(Fbar), _ptr(B))
    return B


def inputs(R, T, m, seed, missing=0.15, dtype=np.float64):
    """(y, obs, Z, h, Tm, Q, a0, P0) of a random model: a contracting transition, positive definite covariances"""
    rng = np.random.default_rng(seed)
    y, Z, h = rng.normal(size=(R, T)), rng.normal(size=(R, T, m)), rng.uniform(0.5, 2.0, size=(R, T))
    obs = (rng.uniform(size=(R, T)) >= missing).astype(np.float64)
    Tm = 0.5 * np.eye(m) + 0.4 * rng.normal(size=(m, m)) / np.sqrt(m)
    A, C = rng.normal(size=(m, m + 2)), rng.normal(size=(m, m + 2))
    Q, P0 = A @ A.T / m + 0.1 * np.eye(m), C @ C.T / m + 0.5 * np.eye(m)
    return tuple(np.asarray(v, dtype=dtype) for v in (y, obs, Z, h, Tm, Q, rng.normal(size=m), P0))


# --------------------------------------------------------------------------- probe cases
KAL_M = [1, 2, 3, 4, 5, 8]
KAL_T = [1, 2, 3, 33]
CAP = 8_000     # R T m m, in doubles


def group_lanes(m):
    return 1 if m <= 1 else 2 if m <= 2 else 4 if m <= 4 else 8


def kalman_shapes(W):
    """The thinning rule.  With S = 64 W / G series side by side (G the group of m), the R classes are 1, 2, S - 1, S, S + 1, 2 S + 1 (the
    last series of a pass, the first of the next, a ragged last pass, a further round).  Every m meets every R class twice, without
    and with a mask; the T of the list rotate, and where R T m m would pass 8 000 doubles the rotation falls back to the T that fit.
    -> [(R, T, m, masked)]"""
    shapes = []
    for a, m in enumerate(KAL_M):
        S = 64 * W // group_lanes(m)
        for b, R in enumerate([1, 2, S - 1, S, S + 1, 2 * S + 1]):
            if R < 1:
                continue
            for masked in (False, True):
                fit = [T for T in KAL_T if R * T * m * m <= CAP]
                T = KAL_T[(a + b + 2 * masked + W) % len(KAL_T)]
                if T not in fit:
                    T = fit[(a + b + 2 * masked) % len(fit)]
                if (R, T, m, masked) not in shapes:
                    shapes.append((R, T, m, masked))
    return shapes


def kalman_cases(W):
    """One case per shape runs ``forward``, forms vbar = (v / F) wv and Fbar = (v / F)^2 wF from the stored v and F (so that a poisoned
    series reaches its adjoints the way it does through the generated loops; wv, wF data; products and true divisions only) and
    runs ``backward``; it stores [F | B | vbar | Fbar].  p0 = [obs | Tm] as they are; p1 = y, scaled by the chain, poisoned by whole
    series; p2 = [Z | h | Q | a0 | P0 | wv | wF], scaled (a positive factor: the covariances stay positive definite).  Device memory,
    and LDS where the arrays fit."""
    rng = np.random.default_rng(600 + W)
    cases = []
    shapes = kalman_shapes(W)
    first_missing = next(k for k, (R, T, m, masked) in enumerate(shapes) if masked and T >= 3 and m >= 2)
    diffuse = next(k for k, (R, T, m, masked) in enumerate(shapes) if T >= 3 and m >= 3 and k != first_missing)
    for k, (R, T, m, masked) in enumerate(shapes):
        y, obs, Z, h, Tm, Q, a0, P0 = inputs(R, T, m, seed=int(rng.integers(1 << 30)))
        tag = " masked" if masked else ""
        if k == first_missing:
            obs[:, 0] = 0.0
            tag += " first step missing"
        if k == diffuse:
            P0 = 1e8 * np.eye(m)
            tag += " P0=1e8 I"
        wv, wF = rng.normal(size=(R, T)), rng.normal(size=(R, T))
        n_f, n_b = sizes(R, T, m)
        rt = R * T
        o_h, o_q = rt * m, rt * m + rt
        o_a0, o_p0 = o_q + m * m, o_q + m * m + m
        o_wv = o_p0 + m * m
        o_v = rt * (2 * m + m * m)
        shape = f"{R}, {T}, {m}, {'true' if masked else 'false'}"
        call = (f"nphip_kalman::forward<{shape}>(P1, P0, P2, P2 + {o_h}, P0 + {rt}, P2 + {o_q}, P2 + {o_a0}, P2 + {o_p0}, PO, lane); "
                f"for (int e = lane; e < {rt}; e += NPHIP_CHAIN_THREADS) {{ const double q = (double)PO[{o_v} + e] / (double)PO[{o_v + rt} + e]; "
                f"PO[{n_f + n_b} + e] = q * (double)P2[{o_wv} + e]; PO[{n_f + n_b + rt} + e] = (q * q) * (double)P2[{o_wv + rt} + e]; }} "
                f"nphip_chain_barrier(); "
                f"nphip_kalman::backward<{shape}>(P1, P0, P2, P2 + {o_h}, P0 + {rt}, P2 + {o_q}, PO, PO + {n_f + n_b}, PO + {n_f + n_b + rt}, PO + {n_f}, lane);")

        def run(p0, p1, p2, R=R, T=T, m=m, masked=masked):
            rt = R * T
            ob, Tm_ = (p0[:rt] if masked else None), p0[rt:]
            Z_, h_, Q_, a0_, P0_, wv_, wF_ = np.split(p2, np.cumsum([rt * m, rt, m * m, m, m * m, rt]))
            with np.errstate(all="ignore"):
                F = forward(p1, ob, Z_, h_, Tm_, Q_, a0_, P0_, R, T, m)
                q = F[rt * (2 * m + m * m):rt * (2 * m + m * m) + rt] / F[rt * (2 * m + m * m) + rt:]
                vbar, Fbar = q * wv_, (q * q) * wF_
                return np.concatenate([F, backward(p1, ob, Z_, h_, Tm_, Q_, F, vbar, Fbar, R, T, m), vbar, Fbar])

        cases.append(P.Case(f"kalman R={R} T={T} m={m}{tag}", call, np.concatenate([obs.reshape(-1), Tm.reshape(-1)]), y,
                            np.concatenate([v.reshape(-1) for v in (Z, h, Q, a0, P0, wv, wF)]), n_f + n_b + 2 * rt, run, poison=(R // 2, T)))
    return P.with_lds(cases)


@functools.lru_cache(maxsize=None)
def probe(W: int) -> P.Probe:
    return P.Probe(f"kalman W={W}", W, ["chain_kalman.h"], kalman_cases(W))


def shape_of(case: P.Case):
    """(R, T, m, the mask or None) of a probe case"""
    R, T = case.p1.shape
    m = int(round(np.sqrt(case.p0.size - R * T)))
    return R, T, m, (case.p0[:R * T].reshape(R, T) if " masked" in case.name else None)


def split(case: P.Case, flat):
    """the per-series arrays (apred, Ppred, afilt, v, F, ybar, hbar, Zbar, partials) as [R, ...] and the four sums over the series
    [Tbar | Qbar | a0bar | P0bar] of one chain's output of a case"""
    R, T, m, _ = shape_of(case)
    rt = R * T
    ps = 3 * m * m + m
    parts = np.split(np.asarray(flat), np.cumsum([rt * m, rt * m * m, rt * m, rt, rt, rt, rt, rt * m, ps, R * ps, rt]))
    per_series = [parts[k].reshape(R, -1) for k in (0, 1, 2, 3, 4, 5, 6, 7, 9, 10, 11)]
    return per_series, parts[8]
