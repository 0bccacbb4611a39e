"""References of the Kalman smoother stage (nutpie_amd/csrc/kalman_smoother.h).

* The plain-C restatement of its order contract (tests/fixtures/kalman_smoother_reference.c), built with gcc and called through ctypes:
  ``smooth``; and the probe cases that reach the device routine directly (``chain_stage_probes.Probe`` / ``Case``), built like
  ``kalman_reference.kalman_cases``: ``forward``, then ``smooth``, storing ``[F | S]``.
* Two independent mpmath forms: (a) ``mp_sequential`` — the filter and the backward recursion, every operation rounded to a chosen
  precision (50 digits: the reference; 53 bits: what the algorithm itself loses in double precision); (b) ``mp_dense`` — no recursion:
  the joint Gaussian law of all the states of a series, conditioned on its observed y in one step, at 50 digits.
* The models tests/test_gpu_kalman_smoother.py compiles (and tests/prebuild_kalman_smoother_cache.py ahead of time).

Packed results: ``F`` as in kalman_reference.py, ``S = [asm: R T m | vsm: R T m]``."""
from __future__ import annotations

import ctypes
import functools
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import chain_stage_probes as P  # noqa: E402
import kalman_models  # noqa: E402
import kalman_reference as K  # noqa: E402

DIGITS = 50


@functools.lru_cache(maxsize=None)
def lib():
    src, out = os.path.join(HERE, "fixtures", "kalman_smoother_reference.c"), os.path.join(HERE, "fixtures", "libkalman_smoother_reference.so")
    if not os.path.exists(out) or os.path.getmtime(out) < os.path.getmtime(src):
        subprocess.run(["gcc", "-O2", "-fPIC", "-shared", "-ffp-contract=off", "-o", out, src, "-lm"], check=True)
    so = ctypes.CDLL(out)
    dp = ctypes.POINTER(ctypes.c_double)
    so.kalman_smooth.argtypes = [ctypes.c_int] * 4 + [dp] * 5
    so.kalman_smooth.restype = None
    return so


def size(R, T, m):
    """the length of S"""
    return 2 * R * T * m


def smooth(obs, Z, Tm, F, R, T, m):
    """S of one chain from the filter's packed F; ``obs`` None: no mask"""
    masked = obs is not None
    Z, Tm, F = K._c(Z, R * T * m), K._c(Tm, m * m), K._c(F, K.sizes(R, T, m)[0])
    obs = K._c(obs, R * T) if masked else np.ones(R * T)
    S = np.empty(size(R, T, m))
    lib().kalman_smooth(R, T, m, int(masked), K._ptr(obs), K._ptr(Z), K._ptr(Tm), K._ptr(F), K._ptr(S))
    return S


def filter_and_smooth(y, obs, Z, h, Tm, Q, a0, P0, R, T, m):
    """(F, S) of the two C restatements, one after the other"""
    F = K.forward(y, obs, Z, h, Tm, Q, a0, P0, R, T, m)
    return F, smooth(obs, Z, Tm, F, R, T, m)


# --------------------------------------------------------------------------- mpmath: (a) the sequential smoother
def _mp_arrays(values, shapes):
    import mpmath

    out = []
    for v, shape in zip(values, shapes):
        a = np.empty(int(np.prod(shape)), dtype=object)
        a[:] = [mpmath.mpf(float(x)) for x in np.asarray(v, dtype=np.float64).reshape(-1)]      # (exact: a double is a binary fraction)
        out.append(a.reshape(shape))
    return out


def mp_sequential(y, obs, Z, h, Tm, Q, a0, P0, R, T, m, prec=None):
    """The filter and the smoother's recursion, every operation rounded to ``prec`` bits (None: 50 digits).  The inputs
    are doubles, taken exactly.  -> dict of object arrays of mpf: apred [R, T, m], Ppred [R, T, m, m], afilt [R, T, m], asm, vsm
    [R, T, m].  P, N and W are used as computed (nothing is symmetrised), as in the contract."""
    import mpmath

    ctx = mpmath.workprec(prec) if prec is not None else mpmath.workdps(DIGITS)
    with ctx:
        y, Z, h, Tm, Q, a0, P0 = _mp_arrays((y, Z, h, Tm, Q, a0, P0), ((R, T), (R, T, m), (R, T), (m, m), (m, m), (m,), (m, m)))
        seen = np.ones((R, T), bool) if obs is None else np.asarray(obs).reshape(R, T) != 0
        zero, one = mpmath.mpf(0), mpmath.mpf(1)
        out = {k: np.empty((R, T) + sh, dtype=object) for k, sh in (("apred", (m,)), ("Ppred", (m, m)), ("afilt", (m,)), ("asm", (m,)), ("vsm", (m,)))}
        v, Fv = np.empty((R, T), dtype=object), np.empty((R, T), dtype=object)
        for q in range(R):
            a, Pm = a0.copy(), P0.copy()
            for t in range(T):
                z = Z[q, t]
                out["apred"][q, t], out["Ppred"][q, t] = a, Pm
                if seen[q, t]:
                    M = Pm.dot(z)
                    v[q, t], Fv[q, t] = y[q, t] - z.dot(a), h[q, t] + z.dot(M)
                    Kg = M / Fv[q, t]
                    af, Pf = a + Kg * v[q, t], Pm - np.outer(Kg, M)
                else:
                    v[q, t], Fv[q, t], af, Pf = zero, one, a, Pm
                out["afilt"][q, t] = af
                if t < T - 1:
                    a, Pm = Tm.dot(af), Q + Tm.dot(Pf).dot(Tm.T)
            r, N = np.full(m, zero, dtype=object), np.full((m, m), zero, dtype=object)
            for t in range(T - 1, -1, -1):
                z, a, Pm = Z[q, t], out["apred"][q, t], out["Ppred"][q, t]
                if t < T - 1:
                    u, W = Tm.T.dot(r), Tm.T.dot(N).dot(Tm)
                else:
                    u, W = np.full(m, zero, dtype=object), np.full((m, m), zero, dtype=object)
                if seen[q, t]:
                    Kg = Pm.dot(z) / Fv[q, t]
                    e = v[q, t] / Fv[q, t] - Kg.dot(u)
                    g, gt = W.dot(Kg), W.T.dot(Kg)
                    D = one / Fv[q, t] + Kg.dot(g)
                    r = u + e * z
                    N = W - np.outer(z, gt) - np.outer(g, z) + D * np.outer(z, z)
                else:
                    r, N = u, W
                out["asm"][q, t] = a + Pm.dot(r)
                Y = Pm.dot(N)
                out["vsm"][q, t] = np.array([Pm[i, i] - Y[i].dot(Pm[i]) for i in range(m)], dtype=object)
        return out


# --------------------------------------------------------------------------- mpmath: (b) dense Gaussian conditioning
def mp_dense(y, obs, Z, h, Tm, Q, a0, P0, R, T, m):
    """Per series: the mean and covariance of x = (state_0 .. state_{T-1}) under the model's prior — E state_{t+1} = Tm E state_t,
    Cov(state_{t+1}, state_s) = Tm Cov(state_t, state_s) for s <= t, Var state_{t+1} = Tm Var state_t Tm^T + Q —, then the
    conditional law given the observed y = H x + e, e ~ N(0, diag h): mean + C H^T S^-1 (y - H mean), C - C H^T S^-1 H C with S =
    H C H^T + diag h.  50 digits.  -> (asm, vsm) object arrays [R, T, m]"""
    import mpmath

    with mpmath.workdps(DIGITS):
        mat = lambda v, r, c: mpmath.matrix([[mpmath.mpf(float(x)) for x in row] for row in np.asarray(v, dtype=np.float64).reshape(r, c)])      # noqa: E731
        Tmm, Qm, P0m = mat(Tm, m, m), mat(Q, m, m), mat(P0, m, m)
        seen = np.ones((R, T), bool) if obs is None else np.asarray(obs).reshape(R, T) != 0
        y, Z, h = np.asarray(y).reshape(R, T), np.asarray(Z).reshape(R, T, m), np.asarray(h).reshape(R, T)
        n = T * m
        mean = mpmath.matrix(n, 1)
        C = mpmath.matrix(n, n)
        mu, V = mat(a0, m, 1), P0m
        for t in range(T):
            mean[t * m:(t + 1) * m, 0] = mu
            C[t * m:(t + 1) * m, t * m:(t + 1) * m] = V
            if t:       # the covariances with every earlier state, from those of the state before
                C[t * m:(t + 1) * m, :t * m] = Tmm * C[(t - 1) * m:t * m, :t * m]
                C[:t * m, t * m:(t + 1) * m] = C[t * m:(t + 1) * m, :t * m].T
            mu, V = Tmm * mu, Tmm * V * Tmm.T + Qm
        asm, vsm = np.empty((R, T, m), dtype=object), np.empty((R, T, m), dtype=object)
        for q in range(R):
            steps = [t for t in range(T) if seen[q, t]]
            post, Cp = mean, C
            if steps:
                H = mpmath.matrix(len(steps), n)
                for k, t in enumerate(steps):
                    for i in range(m):
                        H[k, t * m + i] = mpmath.mpf(float(Z[q, t, i]))
                S = H * C * H.T
                for k, t in enumerate(steps):
                    S[k, k] += mpmath.mpf(float(h[q, t]))
                G = C * H.T * mpmath.inverse(S)
                post = mean + G * (mpmath.matrix([mpmath.mpf(float(y[q, t])) for t in steps]) - H * mean)
                Cp = C - G * H * C
            for t in range(T):
                for i in range(m):
                    asm[q, t, i], vsm[q, t, i] = post[t * m + i, 0], Cp[t * m + i, t * m + i]
        return asm, vsm


def rel_err(got, want):
    """the largest error of an array relative to the largest element of ``want`` (mpf or float entries) -> float"""
    import mpmath

    with mpmath.workdps(DIGITS):
        g, w = np.asarray(got, dtype=object).reshape(-1), np.asarray(want, dtype=object).reshape(-1)
        top = max(abs(mpmath.mpf(x)) for x in w)
        return float(max(abs(mpmath.mpf(a) - mpmath.mpf(b)) for a, b in zip(g, w)) / top)


# --------------------------------------------------------------------------- the models of tests/test_gpu_kalman_smoother.py
SMOOTHED_EXAMPLE = dict(T=50, missing=0.1, smoothed=True, forecast=5)      # level + slope (m = 2): 50 steps, a tenth missing, five steps ahead
LAW = dict(T=kalman_models.LAW_T, seed=kalman_models.LAW_SEED)


def local_level_smoothed(T=kalman_models.LAW_T, seed=kalman_models.LAW_SEED, prior=kalman_models.LAW_PRIOR):
    """``kalman_models.local_level_marginal`` — the same density, so the same draws — reporting the smoothed and the filtered state"""
    from nutpie_amd import symbolic as S

    m = S.Model()
    s_obs, s_level = kalman_models._scales(m, prior)
    m.dim("time", T)
    m.dim("state", 1)
    one = m.product("state", "state")
    y = m.data("y", kalman_models.local_level_data(T, seed), dim="time")
    args = dict(design=m.data("design", np.ones(1), dim="state"), obs_var=s_obs * s_obs, transition=m.data("transition", np.ones(1), dim=one.name),
                state_cov=S.stack([s_level * s_level], one), init_mean=0.0, init_cov=m.data("init_cov", np.full(1, 100.0), dim=one.name))
    m.add_logp(S.kalman_marginal_lpdf(y, **args))
    m.deterministic("smoothed_state", S.kalman_smoothed_state(y, **args))
    m.deterministic("filtered_state", S.kalman_filtered_state(y, **args))
    return m


# --------------------------------------------------------------------------- probe cases
def smoother_cases(W):
    """One case per shape of ``kalman_reference.kalman_shapes(W)`` runs ``forward`` and then ``smooth`` and stores [F | S].  p0 = [obs | Tm]
    as they are; p1 = y, scaled by the chain, poisoned by whole series; p2 = [Z | h | Q | a0 | P0], scaled (a positive factor: the
    covariances stay positive definite).  Named cases: a first step that is missing, a last step that is missing, P0 = 1e8 I.
    Device memory, and LDS where the arrays fit."""
    rng = np.random.default_rng(700 + W)
    cases = []
    shapes = K.kalman_shapes(W)
    first_missing = next(k for k, (R, T, m, masked) in enumerate(shapes) if masked and T >= 3 and m >= 2)
    last_missing = next(k for k, (R, T, m, masked) in enumerate(shapes) if masked and T >= 3 and m >= 2 and k != first_missing)
    diffuse = next(k for k, (R, T, m, masked) in enumerate(shapes) if T >= 3 and m >= 3 and k not in (first_missing, last_missing))
    for k, (R, T, m, masked) in enumerate(shapes):
        y, obs, Z, h, Tm, Q, a0, P0 = K.inputs(R, T, m, seed=int(rng.integers(1 << 30)))
        tag = " masked" if masked else ""
        if k == first_missing:
            obs[:, 0] = 0.0
            tag += " first step missing"
        if k == last_missing:
            obs[:, -1] = 0.0
            tag += " last step missing"
        if k == diffuse:
            P0 = 1e8 * np.eye(m)
            tag += " P0=1e8 I"
        n_f = K.sizes(R, T, m)[0]
        rt = R * T
        o_h, o_q = rt * m, rt * m + rt
        o_a0, o_p0 = o_q + m * m, o_q + m * m + m
        shape = f"{R}, {T}, {m}, {'true' if masked else 'false'}"
        call = (f"nphip_kalman::forward<{shape}>(P1, P0, P2, P2 + {o_h}, P0 + {rt}, P2 + {o_q}, P2 + {o_a0}, P2 + {o_p0}, PO, lane); "
                f"nphip_kalman::smooth<{shape}>(P0, P2, P0 + {rt}, PO, PO + {n_f}, lane);")

        def run(p0, p1, p2, R=R, T=T, m=m, masked=masked):
            rt = R * T
            ob, Tm_ = (p0[:rt] if masked else None), p0[rt:]
            Z_, h_, Q_, a0_, P0_ = np.split(p2, np.cumsum([rt * m, rt, m * m, m]))
            with np.errstate(all="ignore"):
                return np.concatenate(filter_and_smooth(p1, ob, Z_, h_, Tm_, Q_, a0_, P0_, R, T, m))

        cases.append(P.Case(f"smoother R={R} T={T} m={m}{tag}", call, np.concatenate([obs.reshape(-1), Tm.reshape(-1)]), y,
                            np.concatenate([v.reshape(-1) for v in (Z, h, Q, a0, P0)]), n_f + size(R, T, m), run, poison=(R // 2, T)))
    return P.with_lds(cases)


@functools.lru_cache(maxsize=None)
def probe(W: int) -> P.Probe:
    return P.Probe(f"kalman smoother W={W}", W, ["chain_kalman.h", "kalman_smoother.h"], smoother_cases(W))


def split(case: P.Case, flat):
    """the per-series arrays (apred, Ppred, afilt, v, F, asm, vsm) as [R, ...] of one chain's output of a case"""
    R, T, m, _ = K.shape_of(case)
    rt = R * T
    parts = np.split(np.asarray(flat), np.cumsum([rt * m, rt * m * m, rt * m, rt, rt, rt * m]))
    return [p.reshape(R, -1) for p in parts]
