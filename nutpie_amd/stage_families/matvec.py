"""Data-matrix stages: products with a design matrix read from L2 (``csrc/chain_matvec.h``).

``matvec`` E = X B (arg B on the matrix's columns, result on its rows) and ``matvec_t`` C = X^T G, each the other's adjoint.
payload = (name of the matrix, K columns, R right-hand sides).  With them ``Matrix`` (what ``Model.matrix`` returns) and the two
functions that take a value on ``product(rows, rhs)`` apart into its columns and back."""

from __future__ import annotations

import numpy as np

from nutpie_amd.expr import Dim, Expr, _bcast, elem
from nutpie_amd.stage_families import Family
from nutpie_amd.trace_values import _is_traced, _numel, _Sym, _X

_MVOPS = ("matvec", "matvec_t")
MAX_RHS = 16        # the right-hand sides of one product: that many accumulators per row block of a lane


class Matrix:
    """Float data with one row per element of ``dim`` and one column per element of ``cols`` (a design matrix).  ``X @ v`` with ``v``
    on ``cols`` is the linear predictor on ``dim``.  With up to ``STAGE_ABOVE`` columns it is a sum over the columns of (column
    x element of v), so that its transpose — the gradient with respect to ``v`` — is one wave-wide sum per column; with more (or
    ``Model.matrix(..., stage=True)``) it is a stage between loops that one device routine runs (``csrc/chain_matvec.h``, DESIGN.md
    §11.7), and ``X.T @ g`` with ``g`` on ``dim`` the transposed product."""

    #: the automatic lowering keeps the sum over the columns up to this many columns: the stage from 64 on, the smallest measured
    #: width where it samples faster (logistic regression, n = 2000, 512 chains: 1.46 against 0.91 M leapfrogs/s; at 32 columns 1.64
    #: against 5.46 — profiles/matvec_wide_regression.txt)
    STAGE_ABOVE = 63

    def __init__(self, name: str, dim: Dim, cols: Dim, stage: bool | None = None, model=None):
        self.name, self.dim, self.cols, self.stage = name, dim, cols, stage
        self._model = model               # (weak) the Model that holds the data: a stage registers the transposed copy there

    def column(self, c: int) -> "Expr":
        return Expr("datacol", (), self.dim, (self.name, int(c), self.cols.size))

    @property
    def T(self) -> "_MatrixT":
        """The transposed matrix: ``X.T @ g`` with ``g`` on the rows' dimension is a value on ``cols``."""
        return _MatrixT(self)

    def _staged_product(self) -> bool:
        return self.stage if self.stage is not None else self.cols.size > Matrix.STAGE_ABOVE

    def _register_stage(self):
        m = self._model() if self._model is not None else None
        if m is None:
            raise ValueError(f"matrix {self.name!r} belongs to no Model")
        m._matrix_stage(self)

    def _rhs(self, v, outer: Dim, what: str) -> Dim | None:
        """the dimension of the right-hand sides when ``v`` lives on a ``Model.product(outer, rhs)``, None when it lives on ``outer``"""
        if isinstance(v, Expr) and v.dim is outer:
            return None
        if not isinstance(v, Expr) or v.dim is None or v.dim.factors is None or v.dim.factors[0] is not outer:
            raise ValueError(f"matrix {self.name!r}{what} multiplies a vector on dimension {outer.name!r} (or a value on a product({outer.name!r}, right-hand sides))")
        rhs = v.dim.factors[1]
        if rhs.size > MAX_RHS:
            raise ValueError(f"matrix {self.name!r}{what} multiplies up to {MAX_RHS} right-hand sides at once ({rhs.name!r} has {rhs.size})")
        return rhs

    def _product_dim(self, outer: Dim, rhs: Dim) -> Dim:
        return self._model().product(outer.name, rhs.name)

    def times(self, B: "Expr", out: Dim, R: int) -> "Expr":
        """``X B`` for ``B`` on ANY fixed-size dimension of K x R elements (row-major), the n x R result on ``out`` (n x R elements) —
        what a front end that keeps its tensors flat calls (the torch tracer); ``X @ B`` is this on a ``Model.product``."""
        K = self.cols.size
        if not isinstance(B, Expr) or B.dim is None or B.dim.size != K * R or not 1 <= R <= MAX_RHS or out.len_py(self._model()._data) != self.dim.len_py(self._model()._data) * R:
            raise ValueError(f"matrix {self.name!r} times a K x R value: K = {K}, up to {MAX_RHS} right-hand sides, the result n x R")
        self._register_stage()
        return Expr("matvec", (B,), out, (self.name, K, int(R)))

    def __matmul__(self, v) -> "Expr":
        rhs = self._rhs(v, self.cols, "")
        if rhs is not None:       # K x R coefficients: always the stage, the result n x R on product(rows, right-hand sides)
            self._register_stage()
            return Expr("matvec", (v,), self._product_dim(self.dim, rhs), (self.name, self.cols.size, rhs.size))
        if self._staged_product():
            self._register_stage()
            return Expr("matvec", (v,), self.dim, (self.name, self.cols.size, 1))
        total = None
        for c in range(self.cols.size):
            term = self.column(c) * elem(v, c)
            total = term if total is None else total + term
        return total


class _MatrixT:
    """``X.T``: what ``X.T @ g`` multiplies with (always the stage: the transposed product has no other form)."""

    def __init__(self, matrix: Matrix):
        self.matrix = matrix

    def __matmul__(self, g) -> "Expr":
        X = self.matrix
        rhs = X._rhs(g, X.dim, " transposed")
        X._register_stage()
        if rhs is not None:
            return Expr("matvec_t", (g,), X._product_dim(X.cols, rhs), (X.name, X.cols.size, rhs.size))
        return Expr("matvec_t", (g,), X.cols, (X.name, X.cols.size, 1))


# A value on ``product(rows, rhs)`` (row-major, R = rhs.size values per row) and the R values on ``rows`` that are its columns:
# ``column(E, r)`` reads column r (like a gather: from the stored array, in a loop over the rows), ``pack_columns([g_0 .. g_{R-1}],
# dim)`` is the value whose columns the g_r are (stored by the loop over the rows that computes them) — each the other's adjoint.
# What is element-wise ALONG the right-hand sides (a softmax over the classes) is written with these two, on the rows' loop.
def column(E, r: int) -> Expr:
    """Column ``r`` of a value on a ``Model.product(rows, rhs)``: a value on ``rows``."""
    E = Expr.wrap(E)
    if E.dim is None or E.dim.factors is None or not 0 <= int(r) < E.dim.factors[1].size:
        raise ValueError("column(): a value on a Model.product(rows, rhs) and a column inside it")
    if E.op == "rowpack":
        return E.args[int(r)]
    return Expr("rhscol", (E,), E.dim.factors[0], int(r))


def pack_columns(columns, dim: Dim) -> Expr:
    """The value on ``dim`` = ``Model.product(rows, rhs)`` whose columns are the given values on ``rows`` (or scalars)."""
    columns = [Expr.wrap(c) for c in columns]
    if dim.factors is None or len(columns) != dim.factors[1].size or any(c.dim is not None and c.dim is not dim.factors[0] for c in columns):
        raise ValueError("pack_columns(): one value on the rows (or scalar) per column of a Model.product(rows, rhs)")
    if all(c.is_const(0.0) for c in columns):
        return Expr.const(0.0)
    return Expr("rowpack", tuple(columns), dim, None)


def _adjoint(n: Expr, g: Expr, ad):
    a, = n.args
    ad.acc(a, Expr("matvec_t" if n.op == "matvec" else "matvec", (_bcast(g, n.dim),), a.dim, n.payload))   # B-bar = X^T E-bar, G-bar = X C-bar


def _numpy(n: Expr, args, data, N: int, dim_len) -> np.ndarray:
    name, K, R = n.payload
    X = np.asarray(data[name], dtype=np.float64).reshape(-1, K)
    arg = np.broadcast_to(args[0][:, None] if args[0].ndim == 1 else args[0], (N, dim_len(n.args[0].dim)))
    if n.op == "matvec":      # [N, K, R] -> [N, n, R]
        return np.einsum("ik,nkr->nir", X, arg.reshape(N, K, R)).reshape(N, -1)
    return np.einsum("ik,nir->nkr", X, arg.reshape(N, -1, R)).reshape(N, -1)      # [N, n, R] -> [N, K, R]


# ---- the generated call (the routine ends with the chain's barrier)
def _call(gen, n: Expr) -> str:
    name, K, R = n.payload
    arg, out = gen.store_name[n.args[0].id], gen.store_name[n.id]
    rows = gen.m._matrix_t[name].dim          # (the length the routines take is the matrix's rows, whatever R)
    # the routines read the matrix from device memory — also a matrix that the loops of a sum over its columns read from the
    # workgroup's staged copy in LDS (a narrow matrix with `X @ beta` unrolled and `X.T @ g` beside it)
    if n.op == "matvec":
        return f"    nphip_mv::times<{K}, {R}>(data.{name}__t, {arg}, {out}, n_{rows.name}, lane);"
    return f"    nphip_mv::times_t<{K}, {R}>(data.{name}, {arg}, {out}, n_{rows.name}, lane);"


def _section(n: Expr) -> str:
    return f"stage {n.op}<{n.payload[1]}, {n.payload[2]}> of {n.payload[0]}"


# ---- the torch side: what nutpie_amd.torch_trace's matmul asks through FAMILY.torch_matmul
def _data_matrix_product(it, mat, vec, out_shape, original):
    torch = it.torch
    rows, k = int(mat.shape[0]), int(mat.shape[1])
    # (up to Matrix.STAGE_ABOVE columns the IR unrolls the product over the columns; beyond, `Matrix @` is the data-matrix stage
    #  of csrc/chain_matvec.h: the matrix is read as data, never expanded into an n k-element product)
    if not (k > 1 and rows > 1) or isinstance(vec, _X) and not it.whole:
        return None
    bv = it.sym(vec)
    if bv.expr.dim is None or not bool(torch.isfinite(mat).all()):
        return None
    name = it.fresh_name(original)
    m = it.m.matrix(name, mat.to(torch.float64).contiguous().cpu().numpy(), dim=it.dim(rows).name, cols=it.dim(k).name)
    return _Sym(m @ bv.expr, out_shape)


def _torch_matmul(it, a, b, sa, sb):
    torch = it.torch
    ca, cb = not _is_traced(a), not _is_traced(b)
    # a data matrix times a traced vector: the IR's design-matrix form (few columns: one wave-wide sum per column in the gradient;
    # many: the data-matrix stage); `v @ M` with M[k, n] data is the same product with the transposed matrix
    if cb and len(sb) == 2 and len(sa) in (1, 2) and _numel(sa) == sb[0] and not ca:
        r = _data_matrix_product(it, b.t(), a, (sb[1],) if len(sa) == 1 else (1, sb[1]), None)
        if r is not None:
            return r
    if ca and len(sa) == 2 and len(sb) in (1, 2) and _numel(sb) == sa[1] and not cb:
        r = _data_matrix_product(it, a, b, (sa[0],) if len(sb) == 1 else (sa[0], 1), a)
        if r is not None:
            return r
    # a data matrix times a traced k x R matrix (the classes of a softmax regression; leading axes of length one are the batch's):
    # one product with R right-hand sides, the n x R result row-major as torch has it
    if (ca and len(sa) >= 2 and len(sb) >= 2 and sb[-2] == sa[-1] and 2 <= sb[-1] <= MAX_RHS and _numel(sa[:-2]) == 1
            and _numel(sb[:-2]) == 1 and sa[-2] > 1 and sa[-1] > 1 and not cb and not (isinstance(b, _X) and not it.whole)):
        bv = it.sym(b)
        n, k, R = sa[-2], sa[-1], sb[-1]
        if bv.expr.dim is not None and bool(torch.isfinite(a).all()):
            m = it.m.matrix(it.fresh_name(a), a.reshape(n, k).to(torch.float64).contiguous().cpu().numpy(), dim=it.dim(n).name, cols=it.dim(k).name)
            return _Sym(m.times(bv.expr, it.dim(n * R), R), (1,) * (max(len(sa), len(sb)) - 2) + (n, R))
    return NotImplemented


FAMILY = Family(name="matvec", ops=_MVOPS, header="chain_matvec.h", call=_call, numpy=_numpy, adjoint={"matvec": _adjoint, "matvec_t": _adjoint},
                refusal="second derivatives of the matrix and scan stages", section=_section, torch_matmul=_torch_matmul)
