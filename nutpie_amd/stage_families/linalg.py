"""Matrix stages: one chain's dense matrices (``csrc/chain_linalg.h``).

K x K (K <= 32) and K x N values, row-major on a fixed-size dimension (a ``Model.product``), that one device routine turns into another
between two loops.  ``chol`` / ``trsv`` are the user's; the other three are the adjoints the gradient emits.  payload = (K, N): N the
columns of the right-hand sides (K for the K x K stages).

Past 32 x 32, up to 128 x 128, the same ops run on the panel routines of ``csrc/wide_chain_linalg.h`` (``nphip_lw::``) when the model is
compiled with ``wide_matrices=True`` — the family's option, handed to ``_check``; ``_call`` and ``_includes`` go by the stage's K.  The
diagonal of such a factor is read through a gather (``_diagonal``), not element by element."""

from __future__ import annotations

import math

import numpy as np

from nutpie_amd.expr import _HALF_LOG_2PI, Expr, _bcast, elem, log
from nutpie_amd.stage_families import Family
from nutpie_amd.trace_values import UnsupportedTorchOp, _is_traced, _numel, _Sym

_MATOPS = ("chol", "trsv", "trsv_t", "trsv_gl", "chol_adj")
MAX_MATRIX = 32     # the largest K a compiled density factors (8 KB per matrix and chain)
MAX_WIDE = 128      # ... with Model.compile(wide_matrices=True): the panel routines of csrc/wide_chain_linalg.h (128 KB per matrix and chain)
WIDE_HEADER = "wide_chain_linalg.h"


def _side(e: Expr, what: str) -> int:
    if e.dim is None or e.dim.size is None:
        raise ValueError(f"{what}: a matrix lives on a fixed-size dimension (Model.product(rows, cols))")
    k = int(round(math.sqrt(e.dim.size)))
    if k * k != e.dim.size:
        raise ValueError(f"{what}: a square matrix has K * K elements, dimension {e.dim.name!r} has {e.dim.size}")
    return k


def cholesky(A) -> Expr:
    """``L`` with ``L L^T = A`` (K x K, row-major; the upper triangle of ``L`` is zero).  Only the lower triangle of ``A`` is read,
    as by ``torch.linalg.cholesky``, and the gradient is that of what is read: an ``A`` filled below the diagonal only is as valid as a
    symmetric one (for a symmetric ``A`` the parameter gradient is torch.autograd's).  A matrix that is not positive definite gives
    NaN everywhere (the log-density is NaN there: an impossible point)."""
    A = Expr.wrap(A)
    k = _side(A, "cholesky")
    return Expr("chol", (A,), A.dim, (k, k))


def solve_lower(L, B) -> Expr:
    """``L^-1 B`` for a lower-triangular K x K ``L`` (its upper triangle is not read) and a K x N ``B`` (row-major: element
    (i, n) at ``i N + n``, every COLUMN a right-hand side — a value on ``Model.product(k, n)``).  The result lives where ``B`` does."""
    L, B = Expr.wrap(L), Expr.wrap(B)
    k = _side(L, "solve_lower")
    if B.dim is None or B.dim.size is None or B.dim.size % k:
        raise ValueError(f"solve_lower: the right-hand sides are a K x N value on a fixed-size dimension (K = {k})")
    return Expr("trsv", (L, B), B.dim, (k, B.dim.size // k))


def _diagonal(L: Expr, k: int) -> Expr:
    """``diag(L)`` of a wide matrix as a value on a K-long dimension: a gather through the index ``i (K + 1)``, read in the loop over that
    dimension — and its adjoint a segment sum written by the loop over the K x K one: no line of source per element or row.  The index is
    registered once per matrix dimension with the model that declared it (its name holds a double underscore, which no user data can)."""
    kk = L.dim
    m = kk._model() if kk._model is not None else None
    if m is None:
        raise ValueError("the diagonal of a wide matrix: its dimension belongs to no Model")
    name = f"{kk.name}__diag"
    ix = m._indices.get(name)
    if ix is None:
        d = kk.factors[0] if kk.factors is not None and kk.factors[0].size == k else m.dim(f"{kk.name}_diag", k)
        ix = m._add_index(name, np.arange(k) * (k + 1), d.name, kk.name)
    return L[ix]


def log_det_chol(L) -> Expr:
    """``sum(log(diag(L)))``: half the log-determinant of ``L L^T``."""
    L = Expr.wrap(L)
    k = _side(L, "log_det_chol")
    if k > MAX_MATRIX:
        return log(_diagonal(L, k)).sum()
    total = None
    for i in range(k):
        t = log(elem(L, i * k + i))
        total = t if total is None else total + t
    return total


def mvnormal_lpdf(value, mu, *, cov=None, chol=None) -> Expr:
    """Sum over the N columns of the K x N ``value`` (element (i, n) at ``i N + n``: ``Model.product(k, n)``, every column one
    draw) of the multivariate normal log-density with mean ``mu`` (a scalar or a value on the same dimension: ``Model.broadcast``)
    and covariance ``cov`` (K x K) or its lower Cholesky factor ``chol``."""
    if (cov is None) == (chol is None):
        raise ValueError("mvnormal_lpdf: give cov= or chol=")
    value, mu = Expr.wrap(value), Expr.wrap(mu)
    L = cholesky(cov) if chol is None else Expr.wrap(chol)
    k = _side(L, "mvnormal_lpdf")
    if value.dim is None or value.dim.size is None or value.dim.size % k:
        raise ValueError(f"mvnormal_lpdf: value is a K x N value on a fixed-size dimension (K = {k})")
    n = value.dim.size // k
    z = solve_lower(L, value - mu)
    return -0.5 * (z * z).sum() - n * log_det_chol(L) - (n * k) * _HALF_LOG_2PI


def _lkj_log_norm(eta: float, k: int) -> float:
    """log of the LKJ(eta) normalising constant of K x K correlation matrices (Lewandowski, Kurowicka & Joe 2009, eq. 16)"""
    c = 0.0
    for i in range(1, k):
        b = eta + (k - i - 1) / 2.0
        c += (2.0 * eta - 2.0 + k - i) * (k - i) * math.log(2.0) + (k - i) * (2.0 * math.lgamma(b) - math.lgamma(2.0 * b))
    return -c


def lkj_corr_cholesky_lpdf(L, eta: float) -> Expr:
    """Log-density of the Cholesky factor ``L`` (K x K) of an LKJ(``eta``) correlation matrix, with respect to its strictly lower
    elements (Stan's ``lkj_corr_cholesky``): ``sum_{i >= 1} (K - i - 1 + 2 eta - 2) log L[i][i]`` + the normalising constant."""
    L = Expr.wrap(L)
    k = _side(L, "lkj_corr_cholesky_lpdf")
    total = Expr.const(_lkj_log_norm(float(eta), k))
    if k > MAX_MATRIX:      # the exponents as data on the diagonal's dimension (row 0 has none)
        diag = _diagonal(L, k)
        m = diag.dim._model()
        name = f"{L.dim.name}__lkj{sum(1 for f in m._data if f.startswith(L.dim.name + '__lkj'))}"
        m._data[name] = np.array([0.0] + [k - i - 1 + 2.0 * float(eta) - 2.0 for i in range(1, k)])
        m._data_fields.append((name, "double", diag.dim))
        return total + (Expr("data", (), diag.dim, name) * log(diag)).sum()
    for i in range(1, k):
        total = total + (k - i - 1 + 2.0 * float(eta) - 2.0) * log(elem(L, i * k + i))
    return total


# ---- host evaluation
def _np_chol(a: np.ndarray) -> np.ndarray:
    """[N, K, K] -> the lower Cholesky factors (lower triangles read; column by column as csrc/chain_linalg.h), NaN where a pivot fails"""
    N, K, _ = a.shape
    L = np.zeros_like(a)
    bad = np.zeros(N, dtype=bool)
    for j in range(K):
        s = a[:, j:, j] - np.einsum("nik,nk->ni", L[:, j:, :j], L[:, j, :j])
        d = s[:, 0]
        ok = (d > 0.0) & np.isfinite(d)
        bad |= ~ok
        r = np.sqrt(np.where(ok, d, 1.0))
        L[:, j, j] = r
        L[:, j + 1:, j] = s[:, 1:] / r[:, None]
    L[bad] = np.nan
    return L


def _np_solve_lower(L: np.ndarray, B: np.ndarray) -> np.ndarray:
    """L^-1 B: L [N, K, K] (lower triangle read), B [N, K, M]"""
    X = np.zeros(B.shape)
    for i in range(L.shape[1]):
        X[:, i] = (B[:, i] - np.einsum("nk,nkm->nm", L[:, i, :i], X[:, :i])) / L[:, i, i][:, None]
    return X


def _np_solve_lower_t(L: np.ndarray, G: np.ndarray) -> np.ndarray:
    """L^-T G"""
    Y = np.zeros(G.shape)
    for i in reversed(range(L.shape[1])):
        Y[:, i] = (G[:, i] - np.einsum("nk,nkm->nm", L[:, i + 1:, i], Y[:, i + 1:])) / L[:, i, i][:, None]
    return Y


def _np_matop(op: str, args: list[np.ndarray], k: int, m: int) -> np.ndarray:
    N = args[0].shape[0]
    mats = [v.reshape(N, k, -1) for v in args]
    if op == "chol":
        out = _np_chol(mats[0])
    elif op == "trsv":
        out = _np_solve_lower(mats[0], mats[1])
    elif op == "trsv_t":
        out = _np_solve_lower_t(mats[0], mats[1])
    elif op == "trsv_gl":
        out = -np.tril(np.einsum("nim,njm->nij", mats[0], mats[1]))
    else:   # chol_adj: G = L^-T P L^-1, P = Phi(L^T tril(L-bar)) symmetrised (torch.autograd's G), folded onto the lower triangle
        L, Lb = mats
        M = np.tril(np.einsum("nki,nkj->nij", L, np.tril(Lb)))
        P = 0.5 * (M + np.transpose(np.tril(M, -1), (0, 2, 1)))
        Y = _np_solve_lower_t(L, P)
        G = np.transpose(_np_solve_lower_t(L, np.transpose(Y, (0, 2, 1))), (0, 2, 1))
        out = np.tril(G) + np.tril(np.transpose(G, (0, 2, 1)), -1)
    return out.reshape(N, -1)


def _numpy(n: Expr, args, data, N: int, dim_len) -> np.ndarray:
    full = [np.broadcast_to(v[:, None] if v.ndim == 1 else v, (N, dim_len(x.dim))) for v, x in zip(args, n.args)]
    return _np_matop(n.op, full, *n.payload)


# ---- reverse mode
def _chol_adjoint(n: Expr, g: Expr, ad):
    a, = n.args
    ad.acc(a, Expr("chol_adj", (n, _bcast(g, n.dim)), a.dim, n.payload))


def _trsv_adjoint(n: Expr, g: Expr, ad):
    a, b = n.args
    gb = Expr("trsv_t", (a, _bcast(g, n.dim)), b.dim, n.payload)      # B-bar = L^-T X-bar
    ad.acc(b, gb)
    ad.acc(a, Expr("trsv_gl", (gb, n), a.dim, n.payload))            # L-bar = -tril(B-bar X^T)


# ---- the generated call (every routine ends with the wave's barrier)
def _call(gen, n: Expr) -> str:
    k, m = n.payload
    args = ", ".join(gen.store_name[a.id] for a in n.args)
    out = gen.store_name[n.id]
    fn = {"chol": f"cholesky<{k}>", "trsv": f"solve_lower<{k}, {m}>", "trsv_t": f"solve_lower_t<{k}, {m}, {m}, 1>",
          "trsv_gl": f"solve_lower_adj_l<{k}, {m}>", "chol_adj": f"cholesky_adj<{k}>"}[n.op]
    return f"    {'nphip_lw' if _is_wide(n) else 'nphip_la'}::{fn}({args}, {out}, lane);"


def _is_wide(n: Expr) -> bool:
    """a stage of a matrix past the narrow routines' limit: the panel routines run it (``_check`` has let it pass)"""
    return n.payload[0] > MAX_MATRIX


def _section(n: Expr):
    """``Model.profile`` times the wide stages one by one (the narrow ones stay inside their level's section, as they were)"""
    return f"{n.op}<{n.payload[0]}, {n.payload[1]}>" if _is_wide(n) else None


def _includes(nodes) -> list[str]:
    wide = [_is_wide(n) for n in nodes]
    return (["chain_linalg.h"] if not all(wide) else []) + ([WIDE_HEADER] if any(wide) else [])


def _check(nodes, waves_per_chain, wide_matrices=False):
    k = max(n.payload[0] for n in nodes)
    if not wide_matrices and k > MAX_MATRIX:
        raise ValueError(f"a compiled density factors matrices of up to {MAX_MATRIX} x {MAX_MATRIX} (this model: {k} x {k}); "
                         f"compile(wide_matrices=True) factors up to {MAX_WIDE} x {MAX_WIDE}")
    if k > MAX_WIDE:
        raise ValueError(f"a compiled density with wide_matrices=True factors matrices of up to {MAX_WIDE} x {MAX_WIDE} (this model: {k} x {k})")
    if all(_is_wide(n) for n in nodes):
        return waves_per_chain      # the panel routines run on all the chain's waves
    # one wavefront per chain runs the narrow matrix stages
    if waves_per_chain not in (None, 1):
        raise ValueError("a model with matrix stages (cholesky / solve_lower) runs with waves_per_chain=1")
    return 1


# ---- the torch side: what nutpie_amd.torch_trace asks through FAMILY.torch_rules (torch is imported inside the functions)
def _matrix(it, v, what: str) -> tuple[_Sym, int]:
    """a traced square matrix (leading axes of length one) as a K x K value on its own dimension"""
    v = it.sym(v)
    if len(v.shape) < 2 or v.shape[-1] != v.shape[-2] or _numel(v.shape) != v.shape[-1] ** 2:
        raise UnsupportedTorchOp(f"{what} of a traced matrix of shape {v.shape} (one K x K matrix per chain)")
    k = v.shape[-1]
    return _Sym(_bcast(v.expr, it.dim(k * k)), v.shape), k


def _traced_limit(it) -> int:
    """the largest traced matrix: ``trace(..., wide_matrices=True)`` sets the interpreter's ``wide_matrices``"""
    return MAX_WIDE if getattr(it, "wide_matrices", False) else MAX_MATRIX


def _cholesky(it, a) -> _Sym:
    A, k = _matrix(it, a, "cholesky")
    if k > _traced_limit(it):
        raise UnsupportedTorchOp(f"cholesky of a {k} x {k} traced matrix (compiled densities factor up to {_traced_limit(it)} x {_traced_limit(it)})")
    return _Sym(cholesky(A.expr), A.shape)


def _solve_triangular(it, a, b, upper: bool, left: bool) -> _Sym:
    """A X = B (``left``) or X A = B with a traced triangular A, as ``solve_lower`` of K x N right-hand sides"""
    if not left:        # X A = B  <=>  A^T X^T = B^T
        bt = it.move(it.sym(b), lambda t: t.transpose(-1, -2))
        at = it.move(it.sym(a), lambda t: t.transpose(-1, -2))
        return it.move(_solve_triangular(it, at, bt, not upper, True), lambda t: t.transpose(-1, -2))
    if upper:           # U^-1 B = R (R U R)^-1 R B with R the reversal: R U R is lower triangular
        ar = it.move(it.sym(a), lambda t: t.flip(-1, -2))
        br = it.move(it.sym(b), lambda t: t.flip(-2))
        return it.move(_solve_triangular(it, ar, br, False, True), lambda t: t.flip(-2))
    A, k = _matrix(it, a, "solve_triangular")
    if k > _traced_limit(it):
        raise UnsupportedTorchOp(f"solve_triangular with a {k} x {k} traced matrix (compiled densities solve up to {_traced_limit(it)} x {_traced_limit(it)})")
    B = it.sym(b)
    if len(B.shape) < 2 or B.shape[-2] != k:
        raise UnsupportedTorchOp(f"solve_triangular: right-hand sides of shape {B.shape} for a {k} x {k} matrix")
    bshape = B.shape
    batch, n = bshape[:-2], bshape[-1]
    m = _numel(batch) * n
    # the right-hand sides as K x (batch, N): every column one of them
    Bk = it.move(B, lambda t: t.movedim(-2, 0).reshape(k, m))
    X = _Sym(solve_lower(A.expr, _bcast(Bk.expr, it.dim(k * m))), (k, m))
    return it.move(X, lambda t: t.reshape(k, *batch, n).movedim(0, -2))


def _torch_cholesky(c):
    # a traced matrix: the Cholesky stage (one chain's K x K matrix)
    it = c.it
    L = _cholesky(it, c.args[0])
    if bool(c.arg(1, "upper", False)):
        L = it.move(L, lambda t: t.transpose(-1, -2))
    if c.base == "linalg_cholesky_ex":
        # (info: 0 — a matrix that is not positive definite makes the density NaN instead of raising)
        return (L, it.torch.zeros(L.shape[:-2], dtype=it.torch.int32))
    return L


def _torch_solve_triangular(c):
    # a traced triangular matrix: the triangular solve (lower, left) — other forms through transposes and reversals; a constant
    # matrix is the tracer's own rule
    if not _is_traced(c.args[0]):
        return NotImplemented
    if bool(c.kwargs.get("unitriangular", False)):
        raise UnsupportedTorchOp(f"{c.name} with unitriangular=True and a traced matrix")
    return _solve_triangular(c.it, c.args[0], c.args[1], bool(c.kwargs.get("upper", False)), bool(c.kwargs.get("left", True)))


FAMILY = Family(name="linalg", ops=_MATOPS, header="chain_linalg.h", call=_call, numpy=_numpy,
                adjoint={"chol": _chol_adjoint, "trsv": _trsv_adjoint}, refusal="second derivatives of the matrix and scan stages",
                check=_check, options=("wide_matrices",), more_headers=(WIDE_HEADER,), includes=_includes, long_results=_is_wide,
                section=_section,
                torch_rules={"linalg_cholesky_ex": _torch_cholesky, "linalg_cholesky": _torch_cholesky, "cholesky": _torch_cholesky,
                             "linalg_solve_triangular": _torch_solve_triangular})
