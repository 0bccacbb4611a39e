"""Kalman filter stages: linear Gaussian state-space models (``csrc/chain_kalman.h``).

``kalman_fwd`` (args y, Z, h, Tm, Q, a0, P0 [, obs]) is the filter, ``kalman_bwd`` (args y, Z, h, Tm, Q, the forward result, vbar, Fbar
[, obs]) its adjoint — what the gradient emits, with the adjoints of the stored v and F that the IR's own loops compute as stored
operands.  Each packs its arrays on a dimension of its own: [apred: R T m | Ppred: R T m m | afilt: R T m | v: R T | F: R T] resp.
[ybar: R T | hbar: R T | Zbar: R T m | Tbar: m m | Qbar: m m | a0bar: m | P0bar: m m | per-series partials: R (3 m m + m)];
``kalman_smooth`` (args Z, Tm, the forward result [, obs]) is the fixed-interval smoother of ``csrc/kalman_smoother.h``, run by the expand
step only: it packs [asm: R T m | vsm: R T m], the smoothed state means and variances, on a third dimension and carries no gradient.
``kalman_part`` (payload: the offset) reads one of them as a value on the dimension it belongs to, like ``hmm_part``.
payload = (R, T, m, masked)."""

from __future__ import annotations

import math

import numpy as np

from nutpie_amd.expr import _HALF_LOG_2PI, Dim, Expr, _bcast, _segsum, log
from nutpie_amd.stage_families import Family, np_part, read_part
from nutpie_amd.trace_values import UnsupportedTorchOp, _numel, _Sym

_KALOPS = ("kalman_fwd", "kalman_bwd", "kalman_smooth")
SMOOTHER_HEADER = "kalman_smoother.h"
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


def _kalman_smooth(F: Expr) -> Expr:
    """the smoother stage over the filter stage ``F``, on the dimension ``<steps>__kf_s`` (named after the shape where ``F``'s is)"""
    R, T, m, _ = F.payload
    Z, Tm = F.args[1], F.args[3]
    model = F.dim._model()
    packed = model.dim(F.dim.name.replace("__kf_f", "__kf_s"), 2 * R * T * m)
    return Expr("kalman_smooth", (Z, Tm, F) + F.args[7:], packed, F.payload)


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


def kalman_smoothed_state(y, *, design, obs_var, transition, state_cov, init_mean, init_cov, observed=None, along: str | None = None,
                          variance: bool = False) -> Expr:
    """The mean of the state at every step given ALL the observations of its series (``variance``: the variance of every state
    element, the diagonal of the smoothed covariance), a value on ``product(y.dim, state)``: the posterior of the latent path that
    ``kalman_marginal_lpdf`` sums out, by the fixed-interval smoother (the backward recursion of de Jong / Durbin & Koopman over
    what the filter stored).  On trailing steps with ``observed = 0`` these are the forecast and its variance.  Meant for
    ``Model.deterministic``: with the same arguments as the model's ``kalman_marginal_lpdf`` it reads the filter stage the density
    has, and mean and variance share one smoother stage, which only the expand step runs.  It carries no gradient."""
    *args, R, T, m, state = _kalman_args(y, design, obs_var, transition, state_cov, init_mean, init_cov, observed, along, "kalman_smoothed_state")
    F = _kalman_forward(*args, R, T, m, what="kalman_smoothed_state")
    steps = F.args[0].dim
    out = steps._model().product(steps.name, state.name)
    return _kalman_part(_kalman_smooth(F), R * T * m if variance else 0, out)


# ---- reverse mode: the adjoints of the stored v and F arrive through their readers, one after the other; the filter's own adjoint is ONE
# backward stage that takes both, built when the traversal reaches the filter node (every reader has been visited by then)
def _part_adjoint(n: Expr, g: Expr, ad):
    a = n.args[0]
    if a.op != "kalman_fwd":       # (the adjoint's own parts; the smoother's: kalman_smoothed_state carries no gradient)
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
    """the packed result of the filter (``kalman_fwd``), its adjoint (``kalman_bwd``) or the smoother (``kalman_smooth``) by the plain
    sequential algorithm in matrix form, in the precision of its arguments: the checker (the bitwise references of the device routines
    are tests/fixtures/kalman_reference.c and kalman_smoother_reference.c)"""
    dt = np.result_type(*args)

    def full(v, *shape):
        v = np.asarray(v)
        return np.broadcast_to(v[:, None] if v.ndim == 1 else v, (N, int(np.prod(shape)))).reshape(N, *shape)

    def unpack(F):
        cuts = np.cumsum([R * T * m, R * T * m * m, R * T * m, R * T])
        return (v_.reshape(N, R, T, *sh) for v_, sh in zip(np.split(np.asarray(F), cuts, axis=1), ((m,), (m, m), (m,), (), ())))

    if op == "kalman_smooth":
        # the backward recursion of de Jong / Durbin & Koopman: r and N gather what the later steps say about the state at t
        Z, Tm = full(args[0], R, T, m), full(args[1], m, m)
        apred, Ppred, _, vs, Fs = unpack(args[2])
        obs = full(args[3], R, T) != 0 if masked else np.ones((N, R, T), bool)
        r, Nm = np.zeros((N, R, m), dt), np.zeros((N, R, m, m), dt)
        mean, var = np.empty((N, R, T, m), dt), np.empty((N, R, T, m), dt)
        for t in range(T - 1, -1, -1):
            z, seen, a, P, v, Fv = Z[:, :, t], obs[:, :, t], apred[:, :, t], Ppred[:, :, t], vs[:, :, t], Fs[:, :, t]
            if t < T - 1:
                u, W = np.einsum("nik,nri->nrk", Tm, r), np.einsum("nli,nrlj,njk->nrik", Tm, Nm, Tm)
            else:
                u, W = np.zeros_like(r), np.zeros_like(Nm)
            K = np.einsum("nrij,nrj->nri", P, z) / Fv[..., None]
            e = v / Fv - np.einsum("nri,nri->nr", K, u)
            g, gt = np.einsum("nrij,nrj->nri", W, K), np.einsum("nrij,nri->nrj", W, K)
            D = 1.0 / Fv + np.einsum("nri,nri->nr", K, g)
            zz = z[..., :, None] * z[..., None, :]
            r = np.where(seen[..., None], u + e[..., None] * z, u)
            Nm = np.where(seen[..., None, None], W - z[..., :, None] * gt[..., None, :] - g[..., :, None] * z[..., None, :] + D[..., None, None] * zz, W)
            mean[:, :, t] = a + np.einsum("nrij,nrj->nri", P, r)
            var[:, :, t] = np.einsum("nrii->nri", P) - np.einsum("nrij,nrjk,nrik->nri", P, Nm, P)
        return np.concatenate([mean.reshape(N, -1), var.reshape(N, -1)], axis=1)
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
    apred, Ppred, _, vs, Fs = unpack(args[5])
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
    if n.op == "kalman_smooth":
        Z, Tm, F = n.args[:3]
        return f"    nphip_kalman::smooth<{shape}>({obs}, {name(Z)}, {name(Tm)}, {name(F)}, {name(n)}, lane);"
    y, Z, h, Tm, Q, F, vbar, Fbar = n.args[:8]
    return (f"    nphip_kalman::backward<{shape}>({name(y)}, {obs}, {name(Z)}, {name(h)}, {name(Tm)}, {name(Q)}, {name(F)}, {name(vbar)}, {name(Fbar)}, "
            f"{name(n)}, lane);")


def _section(n: Expr) -> str:
    return f"stage {n.op}<{', '.join(str(int(v)) for v in n.payload)}>"


def _includes(nodes) -> list[str]:
    """a source that runs the smoother (an expand function) includes its header beside the filter's"""
    return [FAMILY.header] + ([SMOOTHER_HEADER] if any(n.op == "kalman_smooth" for n in nodes) else [])


def _check(nodes, waves_per_chain):
    if max(n.payload[2] for n in nodes) > MAX_KALMAN_STATE:
        raise ValueError(f"a compiled density filters states of up to {MAX_KALMAN_STATE} dimensions (this model: {max(n.payload[2] for n in nodes)})")
    return waves_per_chain


def _series_lengths(payload) -> set[int]:
    R, T, m = payload[:3]
    return {R * T * m, R * T, T}


# ---- the torch side: what nutpie_amd.torch_trace asks through FAMILY.torch_rules (torch is imported inside the functions)
def _kalman_traced(it, y, design, obs_var, transition, state_cov, init_mean, init_cov, observed=None) -> _Sym:
    """nutpie_amd::kalman_marginal onto the IR's Kalman filter stage: the leading axes of ``y`` are the series"""
    ys, zs = it.sym(y), it.sym(design)
    if len(ys.shape) < 1 or len(zs.shape) < 2 or tuple(zs.shape[:-1]) != tuple(ys.shape):
        raise UnsupportedTorchOp("kalman_marginal: y is [..., T] and design [..., T, m]")
    T, m = ys.shape[-1], zs.shape[-1]
    R = _numel(ys.shape[:-1])
    on = lambda sym_, n: _bcast(sym_.expr, it.dim(n))      # noqa: E731  (a scalar for all elements, or the value on the dimension of n elements)
    mats = [it.sym(v) for v in (transition, state_cov, init_cov)]
    a0 = it.sym(init_mean)
    if any(_numel(v.shape) != m * m or tuple(v.shape[-2:]) != (m, m) for v in mats) or _numel(a0.shape) != m:
        raise UnsupportedTorchOp("kalman_marginal: one m x m transition, state_cov, init_cov and one init_mean per chain (a matrix per series or per step is not compiled)")
    hs = it.sym(obs_var)
    if _numel(hs.shape) not in (1, R * T):
        raise UnsupportedTorchOp("kalman_marginal: obs_var is a scalar or [..., T]")
    obs = None
    if observed is not None:
        o = it.sym(observed).expr
        if o.op == "const":
            if o.payload == 0.0:
                return _Sym(Expr.const(0.0), ys.shape[:-1])
        elif o.op != "data":
            raise UnsupportedTorchOp("kalman_marginal: observed is constant data")
        else:
            obs = _bcast(o, it.dim(R * T))
    Tm, Q, P0 = (on(v, m * m) for v in mats)
    F = _kalman_forward(on(ys, R * T), on(zs, R * T * m), on(hs, R * T), Tm, Q, on(a0, m), P0, obs, R, T, m, "kalman_marginal")
    terms = _kalman_terms(F)
    if R == 1:
        return _Sym(terms.sum(), ys.shape[:-1])
    return _Sym(_segsum(terms, it.index(np.arange(R * T) // T, R * T, R)), ys.shape[:-1])


_KALMAN_OP = None


def _kalman_marginal_op():
    """``nutpie_amd::kalman_marginal``: a torch custom op — one node of a ``make_fx`` trace, which the tracer maps onto the IR's Kalman
    filter stage — with a sequential eager implementation and the adjoint of the filter as its autograd"""
    global _KALMAN_OP
    if _KALMAN_OP is not None:
        return _KALMAN_OP
    import torch

    log_2pi = math.log(2.0 * math.pi)

    def flat(y, Z, h, Tm, Q, a0, P0, observed):
        """every operand with the leading axes of y, flattened into one"""
        lead, T, m = y.shape[:-1], y.shape[-1], Z.shape[-1]
        ex = lambda v, *tail: v.expand(*lead, *tail).reshape(-1, *tail)      # noqa: E731
        seen = torch.ones_like(y) if observed is None else (observed != 0).to(y.dtype)
        return ex(y, T), ex(Z, T, m), ex(h, T), ex(Tm, m, m), ex(Q, m, m), ex(a0, m), ex(P0, m, m), ex(seen, T)

    def filter_loop(y, Z, h, Tm, Q, a0, P0, seen):
        T = y.shape[-1]
        a, P = a0, P0
        apred, Ppred, vs, Fs = [], [], [], []
        for t in range(T):
            z, s_ = Z[:, t], seen[:, t]
            apred.append(a)
            Ppred.append(P)
            M = torch.einsum("bij,bj->bi", P, z)
            v = s_ * (y[:, t] - (z * a).sum(-1))
            F = torch.where(s_ != 0, h[:, t] + (z * M).sum(-1), torch.ones_like(v))
            K = s_[:, None] * M / F[:, None]
            af = a + K * v[:, None]
            Pf = P - K[:, :, None] * M[:, None, :]
            vs.append(v)
            Fs.append(F)
            a = torch.einsum("bik,bk->bi", Tm, af)
            P = Q + torch.einsum("bik,bkl,bjl->bij", Tm, Pf, Tm)
        return torch.stack(apred, 1), torch.stack(Ppred, 1), torch.stack(vs, 1), torch.stack(Fs, 1)

    @torch.library.custom_op("nutpie_amd::kalman_marginal", mutates_args=(),
                             schema="(Tensor y, Tensor design, Tensor obs_var, Tensor transition, Tensor state_cov, Tensor init_mean, Tensor init_cov, Tensor? observed) -> Tensor")
    def op(y, design, obs_var, transition, state_cov, init_mean, init_cov, observed):
        with torch.no_grad():
            ops = flat(y, design, obs_var, transition, state_cov, init_mean, init_cov, observed)
            _, _, v, F = filter_loop(*ops)
            return (-0.5 * ops[7] * (log_2pi + torch.log(F) + v * v / F)).sum(-1).reshape(y.shape[:-1])

    @op.register_fake
    def _(y, design, obs_var, transition, state_cov, init_mean, init_cov, observed):
        return y.new_empty(y.shape[:-1])

    def setup_context(ctx, inputs, output):
        ctx.save_for_backward(*[v for v in inputs if v is not None])
        ctx.masked = inputs[7] is not None

    def backward(ctx, g):
        saved = list(ctx.saved_tensors)
        raw = saved[:7] + [saved[7] if ctx.masked else None]
        y, Z, h, Tm, Q, a0, P0, seen = flat(*raw)
        apred, Ppred, vs, Fs = filter_loop(y, Z, h, Tm, Q, a0, P0, seen)
        T = y.shape[-1]
        gb = g.reshape(-1, 1)
        vbar = gb * seen * (-vs / Fs)
        Fbar = gb * seen * (-0.5) * (1.0 / Fs - vs * vs / (Fs * Fs))
        ybar, hbar, Zbar = torch.zeros_like(y), torch.zeros_like(h), torch.zeros_like(Z)
        Tb, Qb = torch.zeros_like(Tm), torch.zeros_like(Q)
        ab, Pb = torch.zeros_like(a0), torch.zeros_like(P0)
        for t in range(T - 1, -1, -1):
            z, s_, a, P, v, F = Z[:, t], seen[:, t], apred[:, t], Ppred[:, t], vs[:, t], Fs[:, t]
            M = torch.einsum("bij,bj->bi", P, z)
            K = s_[:, None] * M / F[:, None]
            af = a + K * v[:, None]
            Pf = P - K[:, :, None] * M[:, None, :]
            if t < T - 1:
                Qb = Qb + Pb
                Tb = Tb + torch.einsum("bij,bjl,bkl->bik", Pb, Tm, Pf) + torch.einsum("bji,bjl,blk->bik", Pb, Tm, Pf) + ab[:, :, None] * af[:, None, :]
                Pfb = torch.einsum("bli,blj,bjk->bik", Tm, Pb, Tm)
                afb = torch.einsum("bik,bi->bk", Tm, ab)
            else:
                Pfb, afb = torch.zeros_like(Pb), torch.zeros_like(ab)
            Kb = afb * v[:, None] - torch.einsum("bij,bj->bi", Pfb, M)
            vb = vbar[:, t] + (afb * K).sum(-1)
            Fb = Fbar[:, t] - (Kb * K).sum(-1) / F
            Mb = -torch.einsum("bij,bi->bj", Pfb, K) + Kb / F[:, None] + Fb[:, None] * z
            ybar[:, t], hbar[:, t] = s_ * vb, s_ * Fb
            Zbar[:, t] = s_[:, None] * (Fb[:, None] * M + torch.einsum("bik,bi->bk", P, Mb) - vb[:, None] * a)
            ab = afb - (s_ * vb)[:, None] * z
            Pb = Pfb + (s_[:, None] * Mb)[:, :, None] * z[:, None, :]
        lead = raw[0].shape[:-1]
        back = lambda v, like: v.reshape(*lead, *v.shape[1:]).sum_to_size(like.shape)      # noqa: E731
        return (back(ybar, raw[0]), back(Zbar, raw[1]), back(hbar, raw[2]), back(Tb, raw[3]), back(Qb, raw[4]), back(ab, raw[5]), back(Pb, raw[6]), None)

    op.register_autograd(backward, setup_context=setup_context)
    _KALMAN_OP = op
    return op


def kalman_marginal(y, design, obs_var, transition, state_cov, init_mean, init_cov, observed=None):
    """The log-likelihood of a linear Gaussian state-space model with the state summed out by a Kalman filter, one value per series:
    ``y[..., T]`` (every element of the leading axes its own series), ``design[..., T, m]`` or ``[m]`` (the same row at every step),
    ``obs_var[..., T]`` or one number, ``transition[m, m]``, ``state_cov[m, m]``, ``init_mean[m]``, ``init_cov[m, m]`` (the state at
    t = 0, before the first observation; these four may carry leading axes that broadcast against those of ``y``: the chains of a
    batched density), ``observed[..., T]`` constant, 0 where the observation is missing.  Returns ``[...]``; the caller sums over the
    series.  Eager: a sequential loop with the filter's adjoint as its autograd; traced (``torch_trace.trace``,
    ``from_torch_density(compile=True)``): the IR's Kalman filter stage, run on the GPU by ``csrc/chain_kalman.h`` (m <= 8, one
    transition matrix per chain).  A hand-written Python loop over t in a traced function is not recognised: it stays on the general
    path and unrolls into T m^3 terms."""
    import torch

    y = torch.as_tensor(y)
    kw = dict(dtype=y.dtype, device=y.device)
    design, obs_var = torch.as_tensor(design, **kw), torch.as_tensor(obs_var, **kw)
    m = design.shape[-1] if design.dim() else 1
    transition, state_cov, init_cov = (torch.as_tensor(v, **kw) for v in (transition, state_cov, init_cov))
    init_mean = torch.as_tensor(init_mean, **kw)
    if init_mean.dim() == 0:
        init_mean = init_mean.expand(m)
    if y.dim() < 1 or design.dim() < 1 or any(tuple(v.shape[-2:]) != (m, m) for v in (transition, state_cov, init_cov)) or init_mean.shape[-1] != m:
        raise ValueError(f"kalman_marginal: transition, state_cov, init_cov are [..., {m}, {m}] and init_mean [..., {m}] for design [..., {m}]")
    try:
        design = design.expand(*y.shape, m) if design.dim() > 1 else design.expand(*y.shape, m)
        obs_var = obs_var.expand(y.shape)
        if observed is not None:
            observed = torch.as_tensor(observed, **kw).expand(y.shape)
    except RuntimeError as e:
        raise ValueError(f"kalman_marginal: design is [..., T, m] or [m], obs_var and observed [..., T] or scalars for y [..., T] ({e})") from None
    return _kalman_marginal_op()(y, design, obs_var, transition, state_cov, init_mean, init_cov, observed)


def _torch_kalman_marginal(c):
    return _kalman_traced(c.it, *c.args[:8])


FAMILY = Family(name="kalman", ops=_KALOPS, readers=("kalman_part",), header="chain_kalman.h", header_deps=("chain_hmm.h",), call=_call,
                read=read_part, numpy=_numpy, adjoint={"kalman_part": _part_adjoint}, finish=_finish,
                refusal="second derivatives of the Kalman filter stages (kalman_filtered_state and kalman_smoothed_state carry no gradient)",
                more_headers=(SMOOTHER_HEADER,), includes=_includes,
                check=_check, section=_section, series_lengths=_series_lengths, torch_rules={"kalman_marginal": _torch_kalman_marginal})
