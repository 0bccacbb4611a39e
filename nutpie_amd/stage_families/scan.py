"""Scan stages: first-order linear recurrences (``csrc/chain_scan.h``).

x_t = a_t x_{t-1} + b_t over R rows of T elements, row-major on a fixed-size dimension, that one device routine runs between two loops.
``scan`` (args a, b, init) is the user's; ``rscan`` (args a, xbar) the adjoint the gradient emits: lambda_t = a_{t+1} lambda_{t+1} + xbar_t,
lambda_{T-1} = xbar_{T-1}.  ``a`` is a value on the dimension, a scalar, or the constant 1 (a prefix sum); ``init`` a scalar or a value on
the rows.  payload = (R, T)."""

from __future__ import annotations

import numpy as np

from nutpie_amd.expr import Dim, Expr, _bcast, _segsum, elem, select, where_lt
from nutpie_amd.stage_families import Family
from nutpie_amd.trace_values import _numel, _Sym

_SCANOPS = ("scan", "rscan")


def _scan(a, b, init, R: int, T: int, rows: Dim | None = None) -> Expr:
    a, b, init = Expr.wrap(a), Expr.wrap(b), Expr.wrap(init)
    d = b.dim
    if d is None or d.size is None or d.size != R * T:
        raise ValueError("linear_recurrence: b is a value on a fixed-size dimension (R rows of T elements)")
    if a.dim is not None and a.dim is not d:
        raise ValueError("linear_recurrence: a is a scalar or a value on the dimension of b")
    if init.dim is not None and (rows is None or init.dim is not rows):
        raise ValueError("linear_recurrence: init is a scalar or a value on the rows of b")
    if not (a.op == "const" and init.op == "const"):
        # the gradient with respect to a or init reads x_{t-1}: a constant gather, registered with the model now
        m = d._model() if d._model is not None else None
        if m is None:
            raise ValueError("linear_recurrence: b lives on a dimension of no Model")
        m._scan_aux(d, R, T, rows if init.dim is not None else None)
    return Expr("scan", (a, b, init), d, (int(R), int(T)))


def linear_recurrence(a, b, init=0.0, along: str | None = None) -> Expr:
    """``x_t = a_t x_{t-1} + b_t`` with ``x_{-1} = init``, along a dimension of fixed size.  ``b``: a value on it; ``a``: a scalar
    expression or a value on the same dimension.  ``along``: the time axis of a ``Model.product(rows, time)`` — every row is its own
    recurrence and ``init`` a scalar or a value on ``rows``; time must be the inner (second) axis.  Without ``along`` the whole
    dimension is one series.  A non-finite ``a`` or ``b`` makes the values that depend on it non-finite; ``|a| > 1`` grows
    geometrically and overflows on long series (not guarded)."""
    b = Expr.wrap(b)
    d = b.dim
    if d is None or d.size is None:
        raise ValueError("linear_recurrence: b is a value on a dimension of fixed size")
    if along is None or (d.factors is None and along == d.name):
        return _scan(a, b, init, 1, d.size)
    if d.factors is None:
        raise ValueError(f"linear_recurrence: along={along!r} names no axis of dimension {d.name!r}")
    rows, time = d.factors
    if along == rows.name and along != time.name:
        raise ValueError(f"linear_recurrence: {along!r} is the outer axis of {d.name!r}; the time axis must be the inner (second) one")
    if along != time.name:
        raise ValueError(f"linear_recurrence: along={along!r} names no axis of dimension {d.name!r}")
    return _scan(a, b, init, rows.size, time.size, rows)


def cumsum(x, along: str | None = None) -> Expr:
    """The prefix sum of ``x`` (``linear_recurrence(1.0, x, along=along)``)."""
    return linear_recurrence(1.0, x, 0.0, along)


def _scan_grads(n: Expr, lam: Expr) -> tuple[Expr | None, Expr | None]:
    """adjoints of ``a`` and ``init`` in x = scan(a, b, init), lam the adjoint of b: a-bar_t = lam_t x_{t-1} (x_{-1} = init),
    init-bar = a_0 lam_0 per row"""
    a, _, init = n.args
    R, T = n.payload
    d = n.dim
    if a.op == "const" and init.op == "const":
        return None, None
    prev, first, to_r = d._scan_aux[T]

    def at_first(v, w):     # v on the first element of every row, w on the others
        return where_lt(d, 1, v, w) if R == 1 else select(first, v, w)

    ga = gi = None
    if a.op != "const":
        ga = lam * at_first(init if init.dim is None else init[to_r], n[prev])
    if init.op != "const":
        if R == 1 and init.dim is None:
            gi = (a if a.dim is None else elem(a, 0)) * elem(lam, 0)
        else:
            first_terms = at_first(a * lam, 0.0)
            gi = first_terms.sum() if init.dim is None else _segsum(first_terms, to_r)
    return ga, gi


def _adjoint(n: Expr, g: Expr, ad):
    a, b, init = n.args
    lam = Expr("rscan", (a, _bcast(g, n.dim)), n.dim, n.payload)          # the adjoint recurrence, run backwards
    ad.acc(b, lam)
    ga, gi = _scan_grads(n, lam)
    if ga is not None:
        ad.acc(a, ad.reduce_to(ga, n.dim, a))
    if gi is not None:
        ad.acc(init, gi)


# ---- host evaluation
def _np_scan(op: str, args: list[np.ndarray], R: int, T: int, N: int) -> np.ndarray:
    """the recurrence (``scan``) or its adjoint (``rscan``) by a plain loop over time: the checker (the bitwise reference of the device routine is the CPU oracle's ``oracle_chain_scan``)"""
    def rows(v):
        return np.broadcast_to(v[:, None] if v.ndim == 1 else v, (N, R * T)).reshape(N, R, T)

    a, b = rows(args[0]), rows(args[1])
    out = np.empty((N, R, T))
    if op == "scan":
        prev = np.broadcast_to(args[2][:, None] if args[2].ndim == 1 else args[2], (N, R))
        for t in range(T):
            prev = a[:, :, t] * prev + b[:, :, t]
            out[:, :, t] = prev
    else:
        lam = b[:, :, T - 1]
        out[:, :, T - 1] = lam
        for t in range(T - 2, -1, -1):
            lam = a[:, :, t + 1] * lam + b[:, :, t]
            out[:, :, t] = lam
    return out.reshape(N, R * T)


def _numpy(n: Expr, args, data, N: int, dim_len) -> np.ndarray:
    return _np_scan(n.op, args, *n.payload, N)


# ---- the generated call (the routine ends with the chain's barrier)
def _call(gen, n: Expr) -> str:
    R, T = n.payload
    a, v = n.args[0], n.args[1]
    init = n.args[2] if n.op == "scan" else Expr.const(0.0)
    kind = "A_ONE" if a.is_const(1.0) else ("A_SCALAR" if a.dim is None else "A_ARRAY")
    none = "(const double*)nullptr"
    coef = gen.store_name[a.id] if a.dim is not None else none
    a_s = gen.sref(a) if a.dim is None else "1.0"
    irow = init.dim is not None
    i_arr = gen.store_name[init.id] if irow else none
    i_s = "0.0" if irow else gen.sref(init)
    rev = "true" if n.op == "rscan" else "false"
    return (f"    nphip_scan::linear_recurrence<{R}, {T}, nphip_scan::{kind}, {rev}, {'true' if irow else 'false'}>"
            f"({coef}, {a_s}, {gen.store_name[v.id]}, {i_arr}, {i_s}, {gen.store_name[n.id]}, lane);")


# ---- the torch side: what nutpie_amd.torch_trace asks through FAMILY.torch_rules (torch is imported inside the functions)
def _scan_traced(it, a, b: _Sym, init, ax: int) -> _Sym:
    """x_t = a_t x_{t-1} + b_t along axis ``ax`` of the traced ``b`` (``a``: broadcast against ``b``; ``init``: against ``b`` without
    that axis): the axis moved last, the elements of the other axes the rows of one scan stage, the result moved back"""
    shp = b.shape
    last = len(shp) - 1
    to_last = (lambda t: t.movedim(ax, -1)) if ax != last else None
    bm = it.move(b, to_last) if to_last else b
    T = bm.shape[-1] if bm.shape else 1
    R = _numel(bm.shape) // T
    P = it.dim(R * T)
    a_s = it.sym(a)
    if _numel(a_s.shape) == 1:
        a_e = a_s.expr if a_s.expr.dim is None else elem(a_s.expr, 0)
    else:
        if ax != last and len(a_s.shape) == len(shp):
            a_s = it.move(a_s, to_last)
        a_e = it.broadcast(a_s, bm.shape)
        a_e = a_e if a_e.dim is None else _bcast(a_e, P)
    i_s = it.sym(init)
    rows = None
    if _numel(i_s.shape) == 1:
        i_e = i_s.expr if i_s.expr.dim is None else elem(i_s.expr, 0)
    else:
        i_e = it.broadcast(i_s, bm.shape[:-1])
        if i_e.dim is not None:
            rows = it.dim(R)
            i_e = _bcast(i_e, rows)
    x = _Sym(_scan(a_e, _bcast(bm.expr, P), i_e, R, T, rows), bm.shape)
    return it.move(x, lambda t: t.movedim(-1, ax)) if to_last else x


_LR_OP = None


def _linear_recurrence_op():
    """``nutpie_amd::linear_recurrence(a, b, init)`` (time the last axis of ``b``; ``a`` broadcast against ``b``, ``init`` against
    ``b[..., 0]``): a torch custom op — one node of a ``make_fx`` trace, which the tracer maps onto the IR's scan stage — with a
    sequential eager implementation and its adjoint as the autograd formula"""
    global _LR_OP
    if _LR_OP is not None:
        return _LR_OP
    import torch

    def forward_loop(a, b, init):
        a = a.expand_as(b)
        prev = init.expand(b.shape[:-1])
        cols = []
        for t in range(b.shape[-1]):
            prev = a[..., t] * prev + b[..., t]
            cols.append(prev)
        return torch.stack(cols, dim=-1)

    @torch.library.custom_op("nutpie_amd::linear_recurrence", mutates_args=(), schema="(Tensor a, Tensor b, Tensor init) -> Tensor")
    def op(a, b, init):
        return forward_loop(a, b, init)

    @op.register_fake
    def _(a, b, init):
        return torch.empty_like(b)

    def setup_context(ctx, inputs, output):
        a, b, init = inputs
        ctx.save_for_backward(a, b, init, output)

    def backward(ctx, g):
        a, b, init, x = ctx.saved_tensors
        ae = a.expand_as(b)
        # lambda_t = a_{t+1} lambda_{t+1} + g_t (the adjoint recurrence, run backwards)
        shifted = torch.cat([ae[..., 1:], torch.zeros_like(ae[..., :1])], dim=-1)
        lam = forward_loop(shifted.flip(-1), g.flip(-1), torch.zeros((), dtype=g.dtype, device=g.device)).flip(-1)
        xprev = torch.cat([init.expand(b.shape[:-1]).unsqueeze(-1), x[..., :-1]], dim=-1)
        ga = (lam * xprev).sum_to_size(a.shape)
        gi = (ae[..., 0] * lam[..., 0]).sum_to_size(init.shape)
        return ga, lam.sum_to_size(b.shape), gi

    op.register_autograd(backward, setup_context=setup_context)
    _LR_OP = op
    return op


# (``nutpie_amd.torch_trace.linear_recurrence``: in this module that name is the expression front end's)
def torch_linear_recurrence(a, b, init=0.0, dim: int = -1):
    """``x_t = a_t x_{t-1} + b_t`` along axis ``dim`` of the tensor ``b``, with ``x_{-1} = init``: ``a`` a number or a tensor that
    broadcasts against ``b``, ``init`` a number or a tensor that broadcasts against ``b`` without that axis (every other element of
    ``b``'s other axes is its own series).  Eager: a sequential loop with its adjoint as the autograd formula; traced
    (``torch_trace.trace``, ``from_torch_density(compile=True)``): the IR's scan stage, run on the GPU by ``csrc/chain_scan.h``.
    Covers a cumulative sum (``a = 1``), an AR(1) path (``a = phi``), a GARCH(1, 1) variance filter and exponential smoothing."""
    import torch

    b = torch.as_tensor(b)
    a = torch.as_tensor(a, dtype=b.dtype, device=b.device)
    init = torch.as_tensor(init, dtype=b.dtype, device=b.device)
    d = dim % b.dim()
    if d != b.dim() - 1:
        b = b.movedim(d, -1)
        if a.dim() == b.dim():
            a = a.movedim(d, -1)
    x = _linear_recurrence_op()(a, b, init)
    return x.movedim(-1, d) if d != b.dim() - 1 else x


def _torch_cumsum(c):
    # a prefix sum of a traced value along a long axis: the scan stage with a = 1, the axis moved last and the others as rows (a
    # short axis, or a broadcast scalar, is the tracer's own rule)
    shp = c.args[0].shape
    ax = c.arg(1, "dim") % max(len(shp), 1)
    if (shp[ax] if shp else 1) <= 64:
        return NotImplemented
    v = c.it.sym(c.args[0])
    if v.expr.dim is None:
        return NotImplemented
    return _scan_traced(c.it, 1.0, v, 0.0, ax)


def _torch_linear_recurrence(c):
    # nutpie_amd::linear_recurrence (time is the last axis): the scan stage
    b = c.it.sym(c.args[1])
    return _scan_traced(c.it, c.args[0], b, c.args[2], len(b.shape) - 1)


FAMILY = Family(name="scan", ops=_SCANOPS, header="chain_scan.h", call=_call, numpy=_numpy, adjoint={"scan": _adjoint},
                refusal="second derivatives of the matrix and scan stages",
                torch_rules={"cumsum": _torch_cumsum, "linear_recurrence": _torch_linear_recurrence})
