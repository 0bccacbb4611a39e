"""Kalman filter stages: linear Gaussian state-space models (``csrc/chain_kalman.h``).

``kalman_fwd`` (args y, Z, h, Tm, Q, a0, P0 [, obs]) is the filter, ``kalman_bwd`` (args y, Z, h, Tm, Q, the forward result, vbar, Fbar
[, obs]) its adjoint — what the gradient emits, with the adjoints of the stored v and F that the IR's own loops compute as stored
operands.  Each packs its arrays on a dimension of its own: [apred: R T m | Ppred: R T m m | afilt: R T m | v: R T | F: R T] resp.
[ybar: R T | hbar: R T | Zbar: R T m | Tbar: m m | Qbar: m m | a0bar: m | P0bar: m m | per-series partials: R (3 m m + m)];
``kalman_part`` (payload: the offset) reads one of them as a value on the dimension it belongs to, like ``hmm_part``.
payload = (R, T, m, masked)."""

from __future__ import annotations

import numpy as np

from nutpie_amd.expr import _HALF_LOG_2PI, Dim, Expr, _bcast, log
from nutpie_amd.stage_families import Family, np_part, read_part

_KALOPS = ("kalman_fwd", "kalman_bwd")
MAX_KALMAN_STATE = 8   # a lane keeps its row of the state covariance in registers, a group of up to 8 lanes owns a series


def _kalman_sizes(R: int, T: int, m: int) -> tuple[int, int]:
    return R * T * (2 * m + m * m + 2), R * T * (2 + m) + 3 * m * m + m + R * (3 * m * m + m)


def _kalman_forward(y, Z, h, Tm, Q, a0, P0, obs, R: int, T: int, m: int, what: str = "kalman_marginal_lpdf") -> Expr:
    """the filter stage for ``y`` on a dimension of R T elements, ``Z`` on one of R T m (row-major), ``h`` on that of ``y`` — what a front
    end that keeps its tensors flat calls (the torch tracer); the public functions are this on the dimensions of a ``Model``"""
    y, Z, h, Tm, Q, a0, P0 = (Expr.wrap(v) for v in (y, Z, h, Tm, Q, a0, P0))
    steps = y.dim
    if steps is None or steps.size is None or steps.size != R * T:
        raise ValueError(f"{what}: y is a value or data on a fixed-size dimension (R series of T steps)")
    if Z.dim is None or Z.dim.size != R * T * m:
        raise ValueError(f"{what}: design is a value on the {m} states or on product(steps, state)")
    for name, v in (("transition", Tm), ("state_cov", Q), ("init_cov", P0)):
        if v.dim is None or v.dim.size != m * m:
            raise ValueError(f"{what}: {name} is an m x m value on a fixed-size dimension (m = {m}: the states of design)")
    if a0.dim is None or a0.dim.size != m:
        raise ValueError(f"{what}: init_mean is a scalar or a value on the {m} states")
    if h.dim is not steps:
        raise ValueError(f"{what}: obs_var is a scalar or a value on the dimension of y")
    if obs is not None and (obs.op != "data" or obs.dim is not steps):
        raise ValueError(f"{what}: observed is data (0 or 1) on the dimension of y")
    model = steps._model() if steps._model is not None else None
    if model is None:
        raise ValueError(f"{what}: y lives on a dimension of no Model")
    n_f, n_b = _kalman_sizes(R, T, m)
    # (a second filter over the same steps with another split into series or another state: dimensions named after its shape)
    tag = "" if model._dims.get(f"{steps.name}__kf_f", Dim("", n_f)).size == n_f and model._dims.get(f"{steps.name}__kf_b", Dim("", n_b)).size == n_b \
        else f"_{R}x{T}x{m}"
    packed = model.dim(f"{steps.name}__kf_f{tag}", n_f)
    packed._kalman_back = model.dim(f"{steps.name}__kf_b{tag}", n_b)
    args = (y, Z, h, Tm, Q, a0, P0) + ((obs,) if obs is not None else ())
    return Expr("kalman_fwd", args, packed, (int(R), int(T), int(m), obs is not None))


def _kalman_backward(F: Expr, vbar: Expr, Fbar: Expr) -> Expr:
    y, Z, h, Tm, Q = F.args[:5]
    return Expr("kalman_bwd", (y, Z, h, Tm, Q, F, vbar, Fbar) + F.args[7:], F.dim._kalman_back, F.payload)


def _kalman_part(X: Expr, offset: int, dim: Dim) -> Expr:
    return Expr("kalman_part", (X,), dim, int(offset))


def _kalman_terms(F: Expr) -> Expr:
    """the steps' -1/2 obs (log 2 pi + log F + v^2 / F): element-wise IR on the stored v and F"""
    R, T, m, masked = F.payload
    steps = F.args[0].dim
    o = R * T * (2 * m + m * m)
    v, Fv = _kalman_part(F, o, steps), _kalman_part(F, o + R * T, steps)
    terms = (2.0 * _HALF_LOG_2PI) + log(Fv) + v * v / Fv
    if masked:
        terms = F.args[7] * terms
    return -0.5 * terms


def _kalman_args(y, design, obs_var, transition, state_cov, init_mean, init_cov, observed, along, what: str):
    y, Z, h, a0 = Expr.wrap(y), Expr.wrap(design), Expr.wrap(obs_var), Expr.wrap(init_mean)
    steps = y.dim
    if steps is None or steps.size is None:
        raise ValueError(f"{what}: y is a value or data on a fixed-size dimension (steps, or product(series, steps))")
    if along is None or (steps.factors is None and along == steps.name):
        R, T = 1, steps.size
    elif steps.factors is None:
        raise ValueError(f"{what}: along={along!r} names no axis of dimension {steps.name!r}")
    else:
        series, time = steps.factors
        if along == series.name and along != time.name:
            raise ValueError(f"{what}: {along!r} is the outer axis of {steps.name!r}; the time axis must be the inner (second) one")
        if along != time.name:
            raise ValueError(f"{what}: along={along!r} names no axis of dimension {steps.name!r}")
        R, T = series.size, time.size
    model = steps._model() if steps._model is not None else None
    if model is None or Z.dim is None or Z.dim.size is None:
        raise ValueError(f"{what}: design is a value on the states or on product(steps, state), y lives on a dimension of a Model")
    if Z.dim.factors is not None and Z.dim.factors[0] is steps:
        state = Z.dim.factors[1]
    elif Z.dim.factors is None:
        state = Z.dim
        Z = model.broadcast(Z, steps.name, state.name)
    else:
        raise ValueError(f"{what}: design is a value on the states or on product({steps.name!r}, state)")
    if state.size is None:
        raise ValueError(f"{what}: the state dimension has a fixed size")
    if h.dim is None:
        h = _bcast(h, steps)
    if a0.dim is None:
        a0 = _bcast(a0, state)
    obs = None if observed is None else Expr.wrap(observed)
    return y, Z, h, transition, state_cov, a0, init_cov, obs, R, T, state.size, state


def kalman_marginal_lpdf(y, *, design, obs_var, transition, state_cov, init_mean, init_cov, observed=None, along: str | None = None) -> Expr:
    """The log-likelihood of a linear Gaussian state-space model with its state summed out by a Kalman filter:
    ``state_0 ~ N(init_mean, init_cov)`` (before the first observation), ``y_t ~ N(design_t . state_t, obs_var_t)``,
    ``state_{t+1} ~ N(transition state_t, state_cov)``; the value is ``-1/2 sum observed (log 2 pi + log F_t + v_t^2 / F_t)`` with the
    innovations v and their variances F.  ``y``: a value or data on ``steps`` — one series — or on ``product(series, steps)`` with
    ``along`` naming the inner (time) axis: every series its own filter with the same parameters, the values summed; an observation
    offset is ``y - d``.  ``design``: a value on ``product(y.dim, state)`` or on ``state`` alone (the same row at every step);
    ``obs_var``: a scalar or a value on ``y.dim``; ``transition``, ``state_cov``, ``init_cov``: m x m on fixed-size dimensions
    (row-major); ``init_mean``: a scalar or a value on ``state``.  ``observed``: data on ``y.dim``, 0 where the observation is
    missing (the step then only predicts).  m <= 8.  The covariances are used as given (not symmetrised), and the gradient is that of
    what is evaluated.  A step with F <= 0 or a non-finite input makes the density NaN (a divergence; not guarded)."""
    *args, R, T, m, _ = _kalman_args(y, design, obs_var, transition, state_cov, init_mean, init_cov, observed, along, "kalman_marginal_lpdf")
    return _kalman_terms(_kalman_forward(*args, R, T, m)).sum()


def kalman_filtered_state(y, *, design, obs_var, transition, state_cov, init_mean, init_cov, observed=None, along: str | None = None,
                          predicted: bool = False) -> Expr:
    """The mean of the state at every step given the observations up to and including the step (``predicted``: up to the step before),
    a value on ``product(y.dim, state)``.  Meant for ``Model.deterministic``: with the same arguments as the model's
    ``kalman_marginal_lpdf`` it reads the arrays the density computes anyway.  It carries no gradient."""
    *args, R, T, m, state = _kalman_args(y, design, obs_var, transition, state_cov, init_mean, init_cov, observed, along, "kalman_filtered_state")
    F = _kalman_forward(*args, R, T, m, what="kalman_filtered_state")
    steps = F.args[0].dim
    out = steps._model().product(steps.name, state.name)
    return _kalman_part(F, 0 if predicted else R * T * (m + m * m), out)


# ---- reverse mode: the adjoints of the stored v and F arrive through their readers, one after the other; the filter's own adjoint is ONE
# backward stage that takes both, built when the traversal reaches the filter node (every reader has been visited by then)
def _part_adjoint(n: Expr, g: Expr, ad):
    a = n.args[0]
    if a.op != "kalman_fwd":
        return False
    R, T, m, _ = a.payload
    if n.payload < R * T * (2 * m + m * m):       # (the state means: kalman_filtered_state carries no gradient)
        return False
    which = "v" if n.payload == R * T * (2 * m + m * m) else "F"
    slot = ad.pending(a)
    g = _bcast(g, n.dim)
    slot[which] = slot[which] + g if which in slot else g


def _finish(n: Expr, parts: dict, ad):
    R, T, m, _ = n.payload
    y, Z, h, Tm, Q, a0, P0 = n.args[:7]
    back = _kalman_backward(n, *(_bcast(parts.get(k, Expr.const(0.0)), y.dim) for k in ("v", "F")))
    for target, off in ((y, 0), (h, R * T), (Z, 2 * R * T), (Tm, R * T * (2 + m)), (Q, R * T * (2 + m) + m * m),
                        (a0, R * T * (2 + m) + 2 * m * m), (P0, R * T * (2 + m) + 2 * m * m + m)):
        ad.acc(target, _kalman_part(back, off, target.dim))


# ---- host evaluation
def _np_kalman(op: str, args: list[np.ndarray], R: int, T: int, m: int, masked: bool, N: int) -> np.ndarray:
    """the packed result of the filter (``kalman_fwd``) or its adjoint (``kalman_bwd``) by the plain sequential algorithm in matrix form,
    in the precision of its arguments: the checker (the bitwise reference of the device routines is tests/fixtures/kalman_reference.c)"""
    dt = np.result_type(*args)

    def full(v, *shape):
        v = np.asarray(v)
        return np.broadcast_to(v[:, None] if v.ndim == 1 else v, (N, int(np.prod(shape)))).reshape(N, *shape)

    y, Z, h, Tm, Q = full(args[0], R, T), full(args[1], R, T, m), full(args[2], R, T), full(args[3], m, m), full(args[4], m, m)
    fwd = op == "kalman_fwd"
    obs = full(args[7 if fwd else 8], R, T) != 0 if masked else np.ones((N, R, T), bool)
    if fwd:
        a = np.broadcast_to(full(args[5], m)[:, None], (N, R, m)).astype(dt)
        P = np.broadcast_to(full(args[6], m, m)[:, None], (N, R, m, m)).astype(dt)
        apred, Ppred, afilt = np.empty((N, R, T, m), dt), np.empty((N, R, T, m, m), dt), np.empty((N, R, T, m), dt)
        vs, Fs = np.empty((N, R, T), dt), np.empty((N, R, T), dt)
        for t in range(T):
            z, seen = Z[:, :, t], obs[:, :, t]
            apred[:, :, t], Ppred[:, :, t] = a, P
            M = np.einsum("nrij,nrj->nri", P, z)
            v = np.where(seen, y[:, :, t] - np.einsum("nrk,nrk->nr", z, a), 0.0)
            Fv = np.where(seen, h[:, :, t] + np.einsum("nrk,nrk->nr", z, M), 1.0)
            K = np.where(seen[..., None], M / Fv[..., None], 0.0)
            af = a + K * v[..., None]
            Pf = P - K[..., :, None] * M[..., None, :]
            vs[:, :, t], Fs[:, :, t], afilt[:, :, t] = v, Fv, af
            a = np.einsum("nik,nrk->nri", Tm, af)
            P = Q[:, None] + np.einsum("nik,nrkl,njl->nrij", Tm, Pf, Tm)
        return np.concatenate([v_.reshape(N, -1) for v_ in (apred, Ppred, afilt, vs, Fs)], axis=1)
    F = np.asarray(args[5])
    cuts = np.cumsum([R * T * m, R * T * m * m, R * T * m, R * T])
    apred, Ppred, _, vs, Fs = (v_.reshape(N, R, T, *sh) for v_, sh in zip(np.split(F, cuts, axis=1), ((m,), (m, m), (m,), (), ())))
    vbar, Fbar = full(args[6], R, T), full(args[7], R, T)
    ybar, hbar, Zbar = np.zeros((N, R, T), dt), np.zeros((N, R, T), dt), np.zeros((N, R, T, m), dt)
    Tb, Qb = np.zeros((N, R, m, m), dt), np.zeros((N, R, m, m), dt)
    ab, Pb = np.zeros((N, R, m), dt), np.zeros((N, R, m, m), dt)
    for t in range(T - 1, -1, -1):
        z, seen, a, P, v, Fv = Z[:, :, t], obs[:, :, t], apred[:, :, t], Ppred[:, :, t], vs[:, :, t], Fs[:, :, t]
        M = np.einsum("nrij,nrj->nri", P, z)
        K = np.where(seen[..., None], M / Fv[..., None], 0.0)
        af = a + K * v[..., None]
        Pf = P - K[..., :, None] * M[..., None, :]
        if t < T - 1:
            Qb = Qb + Pb
            Tb = Tb + np.einsum("nrij,njl,nrkl->nrik", Pb, Tm, Pf) + np.einsum("nrji,njl,nrlk->nrik", Pb, Tm, Pf) + ab[..., :, None] * af[..., None, :]
            Pfb = np.einsum("nli,nrlj,njk->nrik", Tm, Pb, Tm)
            afb = np.einsum("nik,nri->nrk", Tm, ab)
        else:
            Pfb, afb = np.zeros_like(Pb), np.zeros_like(ab)
        Kb = afb * v[..., None] - np.einsum("nrij,nrj->nri", Pfb, M)
        vb = vbar[:, :, t] + np.einsum("nri,nri->nr", afb, K)
        Fb = Fbar[:, :, t] - np.einsum("nri,nri->nr", Kb, K) / Fv
        Mb = -np.einsum("nrij,nri->nrj", Pfb, K) + Kb / Fv[..., None] + Fb[..., None] * z
        s3, s4 = seen[..., None], seen[..., None, None]
        ybar[:, :, t], hbar[:, :, t] = np.where(seen, vb, 0.0), np.where(seen, Fb, 0.0)
        Zbar[:, :, t] = np.where(s3, Fb[..., None] * M + np.einsum("nrik,nri->nrk", P, Mb) - vb[..., None] * a, 0.0)
        ab = np.where(s3, afb - vb[..., None] * z, afb)
        Pb = np.where(s4, Pfb + Mb[..., :, None] * z[..., None, :], Pfb)
    parts = np.concatenate([Tb.reshape(N, R, -1), Qb.reshape(N, R, -1), ab, Pb.reshape(N, R, -1)], axis=2)
    return np.concatenate([ybar.reshape(N, -1), hbar.reshape(N, -1), Zbar.reshape(N, -1), parts.sum(axis=1), parts.reshape(N, -1)], axis=1)


def _numpy(n: Expr, args, data, N: int, dim_len) -> np.ndarray:
    if n.op == "kalman_part":
        return np_part(n, args, dim_len)
    return _np_kalman(n.op, args, *n.payload, N)


# ---- generated code (every routine ends with the chain's barrier)
def _call(gen, n: Expr) -> str:
    R, T, m, masked = n.payload
    name = lambda a: gen.store_name[a.id]      # noqa: E731
    obs = name(n.args[-1]) if masked else "(const double*)nullptr"
    shape = f"{R}, {T}, {m}, {'true' if masked else 'false'}"
    if n.op == "kalman_fwd":
        y, Z, h, Tm, Q, a0, P0 = n.args[:7]
        return f"    nphip_kalman::forward<{shape}>({name(y)}, {obs}, {name(Z)}, {name(h)}, {name(Tm)}, {name(Q)}, {name(a0)}, {name(P0)}, {name(n)}, lane);"
    y, Z, h, Tm, Q, F, vbar, Fbar = n.args[:8]
    return (f"    nphip_kalman::backward<{shape}>({name(y)}, {obs}, {name(Z)}, {name(h)}, {name(Tm)}, {name(Q)}, {name(F)}, {name(vbar)}, {name(Fbar)}, "
            f"{name(n)}, lane);")


def _section(n: Expr) -> str:
    return f"stage {n.op}<{', '.join(str(int(v)) for v in n.payload)}>"


def _check(nodes, waves_per_chain):
    if max(n.payload[2] for n in nodes) > MAX_KALMAN_STATE:
        raise ValueError(f"a compiled density filters states of up to {MAX_KALMAN_STATE} dimensions (this model: {max(n.payload[2] for n in nodes)})")
    return waves_per_chain


def _series_lengths(payload) -> set[int]:
    R, T, m = payload[:3]
    return {R * T * m, R * T, T}


FAMILY = Family(name="kalman", ops=_KALOPS, readers=("kalman_part",), header="chain_kalman.h", header_deps=("chain_hmm.h",), call=_call,
                read=read_part, numpy=_numpy, adjoint={"kalman_part": _part_adjoint}, finish=_finish,
                refusal="second derivatives of the Kalman filter stages (kalman_filtered_state carries no gradient)",
                check=_check, section=_section, series_lengths=_series_lengths)
