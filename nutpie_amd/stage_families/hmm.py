"""HMM stages: the scaled forward-backward algorithm (``csrc/chain_hmm.h``).

``hmm_fwd`` (args logE, P, pi) is the scaled forward algorithm, ``hmm_bwd`` (args logE, P, the forward result) the backward pass with the
adjoints of P and pi — what the gradient emits.  A stage has ONE stored result, so each packs its arrays on a dimension of its own:
[alpha: R T K | c: R T | m: R T] resp. [beta: R T K | w: R T K | Pbar: K K | pibar: K]; ``hmm_part`` (payload: the offset) reads one of
them as a value on the dimension it belongs to, ``hmm_ll`` the steps' log c_t + m_t — element-wise reads of the stored array, like
``rhscol``.  payload = (R, T, K)."""

from __future__ import annotations

import numpy as np

from nutpie_amd.expr import Dim, Expr, _bcast, _segsum
from nutpie_amd.stage_families import Family, np_part, read_part
from nutpie_amd.trace_values import UnsupportedTorchOp, _numel, _Sym

_HMMOPS = ("hmm_fwd", "hmm_bwd")
MAX_HMM_STATES = 16   # a lane keeps its column (row) of the transition matrix in registers, a group of up to 16 lanes owns a series


def _hmm_model(d: Dim, what: str):
    m = d._model() if d._model is not None else None
    if m is None:
        raise ValueError(f"{what}: log_emission lives on a dimension of no Model")
    return m


def _hmm_forward(logE, P, pi, R: int, T: int, K: int, steps: Dim, what: str = "hmm_marginal_lpdf") -> Expr:
    """the forward stage for ``logE`` on ANY fixed-size dimension of R T K elements (row-major), ``steps`` a dimension of R T elements —
    what a front end that keeps its tensors flat calls (the torch tracer); the public functions are this on a ``Model.product``"""
    logE, P, pi = Expr.wrap(logE), Expr.wrap(P), Expr.wrap(pi)
    d = logE.dim
    if d is None or d.size is None or d.size != R * T * K or steps.size != R * T:
        raise ValueError(f"{what}: log_emission is a value on a fixed-size dimension (R series of T steps of K states)")
    if P.dim is None or P.dim.size != K * K:
        raise ValueError(f"{what}: transition is a K x K value on a fixed-size dimension (K = {K}: the states of log_emission)")
    if pi.dim is not None and pi.dim.size != K:
        raise ValueError(f"{what}: initial is a scalar or a value on the {K} states of log_emission")
    m = _hmm_model(d, what)
    if pi.dim is None:
        pi = _bcast(pi, m.dim(f"{d.name}__hmm_k", K))
    packed = m.dim(f"{d.name}__hmm_f", R * T * K + 2 * R * T)
    F = Expr("hmm_fwd", (logE, P, pi), packed, (int(R), int(T), int(K)))
    packed._hmm_back = m.dim(f"{d.name}__hmm_b", 2 * R * T * K + K * K + K)      # (the backward stage's, should the gradient or a smoothed value need it)
    return F


def _hmm_backward(F: Expr) -> Expr:
    logE, P, _ = F.args
    return Expr("hmm_bwd", (logE, P, F), F.dim._hmm_back, F.payload)


def _hmm_part(X: Expr, offset: int, dim: Dim) -> Expr:
    return Expr("hmm_part", (X,), dim, int(offset))


def _hmm_lpdf(F: Expr, steps: Dim) -> Expr:
    """sum over the R T steps of log c_t + m_t: the IR's own reduction over ``steps``"""
    return Expr("hmm_ll", (F,), steps, F.payload).sum()


def _hmm_prob(F: Expr, smoothed: bool) -> Expr:
    d = F.args[0].dim
    alpha = _hmm_part(F, 0, d)
    return alpha * _hmm_part(_hmm_backward(F), 0, d) if smoothed else alpha


def _hmm_shape(log_emission, along, what: str):
    logE = Expr.wrap(log_emission)
    d = logE.dim
    if d is None or d.size is None or d.factors is None:
        raise ValueError(f"{what}: log_emission is a value on a Model.product(time, state) or product(product(series, time), state)")
    steps, state = d.factors
    if steps.size is None or state.size is None:
        raise ValueError(f"{what}: log_emission is a value on a dimension of fixed size")
    if along is None or (steps.factors is None and along == steps.name):
        return logE, 1, steps.size, state.size, steps
    if steps.factors is None:
        raise ValueError(f"{what}: along={along!r} names no axis of dimension {steps.name!r}")
    series, time = steps.factors
    if along == series.name and along != time.name:
        raise ValueError(f"{what}: {along!r} is the outer axis of {steps.name!r}; the time axis must be the inner (second) one")
    if along != time.name:
        raise ValueError(f"{what}: along={along!r} names no axis of dimension {steps.name!r}")
    return logE, series.size, time.size, state.size, steps


def hmm_marginal_lpdf(log_emission, transition, initial, along: str | None = None) -> Expr:
    """The log-likelihood of a hidden Markov model with its discrete state summed out (Stan's ``hmm_marginal``): ``sum_r log(pi^T
    diag(e_r0) P diag(e_r1) P ... diag(e_r,T-1) 1)`` with ``e = exp(log_emission)``, by the scaled forward algorithm.
    ``log_emission``: the log density of observation t under state k, a value on ``Model.product(time, state)`` — one series — or on
    ``product(product(series, time), state)`` with ``along`` naming the time axis: every series its own chain of states, the values
    summed.  ``transition``: K x K on a fixed-size dimension (row-major; row i the weights of the next state given state i —
    ``Model.transition_matrix``); ``initial``: a value on the K states, or one number for all.  The rows of ``transition`` and
    ``initial`` need not sum to one: the value is the general product above, and so is the gradient with respect to every element.
    K <= 16.  A ``log_emission`` of -inf is an impossible state; a step at which every state is impossible makes the density
    non-finite (a divergence); a NaN makes what depends on it NaN (not guarded)."""
    logE, R, T, K, steps = _hmm_shape(log_emission, along, "hmm_marginal_lpdf")
    return _hmm_lpdf(_hmm_forward(logE, transition, initial, R, T, K, steps), steps)


def hmm_state_prob(log_emission, transition, initial, along: str | None = None, smoothed: bool = True) -> Expr:
    """The probability of every state at every step given the observations (Stan's ``hmm_hidden_state_prob``), a value on the
    dimension of ``log_emission``: given all of the series' observations when ``smoothed`` (alpha_t beta_t of the forward-backward
    algorithm — the gradient of :func:`hmm_marginal_lpdf` with respect to ``log_emission``), given those up to the step otherwise
    (the filtered alpha_t).  Meant for ``Model.deterministic``: with the same arguments as the model's ``hmm_marginal_lpdf`` it reads
    the arrays the density computes anyway.  It carries no gradient."""
    logE, R, T, K, steps = _hmm_shape(log_emission, along, "hmm_state_prob")
    return _hmm_prob(_hmm_forward(logE, transition, initial, R, T, K, steps, "hmm_state_prob"), bool(smoothed))


# ---- reverse mode
def _ll_adjoint(n: Expr, g: Expr, ad):
    a = n.args[0]
    if g.dim is not None and g.op == "gather" and g.args[0].op == "bcast":
        g = g.args[0].args[0]      # (per-series values summed by the caller, as the torch op returns them: one scalar for every step)
    if g.dim is not None:
        raise NotImplementedError("the steps of an HMM likelihood carry one weight: their sum is what is differentiated")
    logE, P, pi = a.args
    R, T, K = n.payload
    back = _hmm_backward(a)
    ad.acc(logE, g * (_hmm_part(a, 0, logE.dim) * _hmm_part(back, 0, logE.dim)))      # alpha_t beta_t
    ad.acc(P, g * _hmm_part(back, 2 * R * T * K, P.dim))
    ad.acc(pi, g * _hmm_part(back, 2 * R * T * K + K * K, pi.dim))


# ---- host evaluation
def _np_hmm(op: str, args: list[np.ndarray], R: int, T: int, K: int, N: int) -> np.ndarray:
    """the packed result of the forward (``hmm_fwd``) or backward (``hmm_bwd``) stage by the plain scaled algorithm: the checker (the
    bitwise reference of the device routines is tests/fixtures/hmm_reference.c)"""
    def full(v, n):
        return np.broadcast_to(v[:, None] if v.ndim == 1 else v, (N, n))

    logE, P = full(args[0], R * T * K).reshape(N, R, T, K), full(args[1], K * K).reshape(N, K, K)
    if op == "hmm_fwd":
        pi = full(args[2], K)
        alpha, c = np.empty((N, R, T, K)), np.empty((N, R, T))
        m = logE.max(axis=3)
        e = np.exp(logE - m[..., None])
        for t in range(T):
            a = (pi[:, None, :] if t == 0 else np.einsum("nri,nij->nrj", alpha[:, :, t - 1], P)) * e[:, :, t]
            c[:, :, t] = a.sum(axis=2)
            alpha[:, :, t] = a / c[:, :, t, None]
        return np.concatenate([alpha.reshape(N, -1), c.reshape(N, -1), m.reshape(N, -1)], axis=1)
    F = args[2]
    alpha, c, m = F[:, :R * T * K].reshape(N, R, T, K), F[:, R * T * K:R * T * K + R * T].reshape(N, R, T), F[:, R * T * K + R * T:].reshape(N, R, T)
    e = np.exp(logE - m[..., None])
    beta, w = np.ones((N, R, T, K)), np.empty((N, R, T, K))
    for t in range(T - 1, -1, -1):
        w[:, :, t] = e[:, :, t] * beta[:, :, t] / c[:, :, t, None]
        if t:
            beta[:, :, t - 1] = np.einsum("nij,nrj->nri", P, w[:, :, t])
    Pbar = np.einsum("nrti,nrtj->nij", alpha[:, :, :-1], w[:, :, 1:])
    return np.concatenate([beta.reshape(N, -1), w.reshape(N, -1), Pbar.reshape(N, -1), w[:, :, 0].sum(axis=1)], axis=1)


def _numpy(n: Expr, args, data, N: int, dim_len) -> np.ndarray:
    if n.op == "hmm_part":
        return np_part(n, args, dim_len)
    if n.op == "hmm_ll":
        R, T, K = n.payload
        return np.log(args[0][:, R * T * K:R * T * K + R * T]) + args[0][:, R * T * K + R * T:]
    return _np_hmm(n.op, args, *n.payload, N)


# ---- generated code (every routine ends with the chain's barrier)
def _call(gen, n: Expr) -> str:
    R, T, K = n.payload
    args = ", ".join(gen.store_name[a.id] for a in n.args)
    out = gen.store_name[n.id]
    if n.op == "hmm_fwd":
        return f"    nphip_hmm::forward<{R}, {T}, {K}>({args}, {out}, lane);"
    call = f"    nphip_hmm::backward<{R}, {T}, {K}>({args}, {out}, lane);"
    if any(m.op == "hmm_part" and m.args[0] is n and m.payload >= 2 * R * T * K for m in gen.order):
        # (the adjoints of P and pi: the density's gradient reads them, the smoothed probabilities of the expand function do not)
        call += f" nphip_hmm::transition_adjoint<{R}, {T}, {K}>({gen.store_name[n.args[2].id]}, {out}, lane);"
    return call


def _read(n: Expr, name: str, array: str, j: str):
    if n.op == "hmm_part":
        return read_part(n, name, array, j)
    R, T, K = n.payload
    return ([f"        const double {name}_c = {array}[{R * T * K} + {j}], {name}_m = {array}[{R * T * K + R * T} + {j}];"],
            [f"        const double {name} = log({name}_c) + {name}_m;"])


def _check(nodes, waves_per_chain):
    if max(n.payload[2] for n in nodes) > MAX_HMM_STATES:
        raise ValueError(f"a compiled density sums out up to {MAX_HMM_STATES} hidden states (this model: {max(n.payload[2] for n in nodes)})")
    return waves_per_chain


def _series_lengths(payload) -> set[int]:
    R, T, K = payload
    return {R * T * K, R * T, T}


# ---- the torch side: what nutpie_amd.torch_trace asks through FAMILY.torch_rules (torch is imported inside the functions)
def _hmm_traced(it, log_emission, transition, initial) -> _Sym:
    """nutpie_amd::hmm_marginal onto the IR's HMM stage: the leading axes of ``log_emission`` are the series"""
    le = it.sym(log_emission)
    if len(le.shape) < 2:
        raise UnsupportedTorchOp("hmm_marginal: log_emission is [..., T, K]")
    T, K = le.shape[-2:]
    R = _numel(le.shape[:-2])
    P_s, pi_s = it.sym(transition), it.sym(initial)
    if _numel(P_s.shape) != K * K or tuple(P_s.shape[-2:]) != (K, K) or _numel(pi_s.shape) != K:
        raise UnsupportedTorchOp("hmm_marginal: one K x K transition matrix and K initial weights per chain (a matrix per series or per step is not compiled)")
    logE = _bcast(le.expr, it.dim(R * T * K))
    P = _bcast(P_s.expr, it.dim(K * K))
    pi = pi_s.expr if pi_s.expr.dim is None else _bcast(pi_s.expr, it.dim(K))
    steps = it.dim(R * T)
    F = _hmm_forward(logE, P, pi, R, T, K, steps, "hmm_marginal")
    if R == 1:
        return _Sym(_hmm_lpdf(F, steps), le.shape[:-2])
    per_step = Expr("hmm_ll", (F,), steps, F.payload)
    return _Sym(_segsum(per_step, it.index(np.arange(R * T) // T, R * T, R)), le.shape[:-2])


_HMM_OP = None


def _hmm_marginal_op():
    """``nutpie_amd::hmm_marginal(log_emission, transition, initial)`` (``transition`` and ``initial`` broadcast against the leading
    axes of ``log_emission``): a torch custom op — one node of a ``make_fx`` trace, which the tracer maps onto the IR's HMM stage —
    with a sequential eager implementation in log space and the forward-backward formulas as its autograd"""
    global _HMM_OP
    if _HMM_OP is not None:
        return _HMM_OP
    import torch

    def forward_loop(logE, P, pi):
        with torch.no_grad():
            lead, K = logE.shape[:-2], logE.shape[-1]
            P, pi = P.expand(*lead, K, K), pi.expand(*lead, K)
            logP = torch.log(P)
            la = [torch.log(pi) + logE[..., 0, :]]
            for t in range(1, logE.shape[-2]):
                la.append(torch.logsumexp(la[-1].unsqueeze(-1) + logP, dim=-2) + logE[..., t, :])
            return torch.stack(la, dim=-2)

    @torch.library.custom_op("nutpie_amd::hmm_marginal", mutates_args=(), schema="(Tensor log_emission, Tensor transition, Tensor initial) -> Tensor")
    def op(log_emission, transition, initial):
        return torch.logsumexp(forward_loop(log_emission, transition, initial)[..., -1, :], dim=-1)

    @op.register_fake
    def _(log_emission, transition, initial):
        return log_emission.new_empty(log_emission.shape[:-2])

    def setup_context(ctx, inputs, output):
        ctx.save_for_backward(*inputs, output)

    def backward(ctx, g):
        logE, P0, pi0, ll = ctx.saved_tensors
        la = forward_loop(logE, P0, pi0)
        T, K = logE.shape[-2:]
        P = P0.expand(*logE.shape[:-2], K, K)
        lb = [torch.zeros_like(la[..., 0, :])]          # log beta, last step first
        for t in range(T - 1, 0, -1):
            lb.append(torch.logsumexp(torch.log(P) + (logE[..., t, :] + lb[-1]).unsqueeze(-2), dim=-1))
        lb = torch.stack(lb[::-1], dim=-2)
        ll_ = ll[..., None, None]
        g_ = g[..., None, None]
        g_logE = g_ * torch.exp(la + lb - ll_)                                   # the smoothed state probabilities
        # d / d P[i][j] = sum_{t >= 1} alpha_{t-1}[i] e_t[j] beta_t[j] / likelihood (zero for T = 1); d / d pi[k] = e_0[k] beta_0[k] / likelihood
        pair = la[..., :-1, :, None] + (logE + lb)[..., 1:, None, :] - ll[..., None, None, None]
        g_P = g_ * torch.exp(pair).sum(dim=-3)
        g_pi = g[..., None] * torch.exp(logE[..., 0, :] + lb[..., 0, :] - ll[..., None])
        return g_logE, g_P.sum_to_size(P0.shape), g_pi.sum_to_size(pi0.shape)

    op.register_autograd(backward, setup_context=setup_context)
    _HMM_OP = op
    return op


def hmm_marginal(log_emission, transition, initial):
    """The log-likelihood of a hidden Markov model with the state summed out, one value per series: ``log_emission[..., T, K]`` the
    log density of observation t under state k (every element of the leading axes its own series), ``transition[K, K]`` with row i
    the weights of the next state given state i, ``initial[K]`` — both non-negative, neither has to sum to one, and both may carry
    leading axes that broadcast against those of ``log_emission`` (the chains of a batched density: ``transition[:, None]`` against
    ``log_emission[chains, series, T, K]``).  Returns ``[...]``; the caller sums over the series.  Eager: a sequential loop in log
    space with the forward-backward formulas as its autograd; traced (``torch_trace.trace``, ``from_torch_density(compile=True)``): the
    IR's HMM stage, run on the GPU by ``csrc/chain_hmm.h`` (K <= 16, one matrix per chain).  A hand-written Python loop over t in a
    traced function is not recognised: it stays on the general path and unrolls into T K^2 terms."""
    import torch

    log_emission = torch.as_tensor(log_emission)
    K = log_emission.shape[-1]
    transition = torch.as_tensor(transition, dtype=log_emission.dtype, device=log_emission.device)
    initial = torch.as_tensor(initial, dtype=log_emission.dtype, device=log_emission.device)
    if initial.dim() == 0:
        initial = initial.expand(K)
    if tuple(transition.shape[-2:]) != (K, K) or initial.shape[-1] != K:
        raise ValueError(f"hmm_marginal: transition is [..., {K}, {K}] and initial [..., {K}] for log_emission [..., T, {K}]")
    return _hmm_marginal_op()(log_emission, transition, initial)


def _torch_hmm_marginal(c):
    return _hmm_traced(c.it, c.args[0], c.args[1], c.args[2])


FAMILY = Family(name="hmm", ops=_HMMOPS, readers=("hmm_part", "hmm_ll"), header="chain_hmm.h", call=_call, read=_read, numpy=_numpy,
                adjoint={"hmm_ll": _ll_adjoint}, refusal="second derivatives of the HMM stages (hmm_state_prob carries no gradient)",
                check=_check, series_lengths=_series_lengths, torch_rules={"hmm_marginal": _torch_hmm_marginal})
