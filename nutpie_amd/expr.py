"""The expression graph of the model front end (``nutpie_amd.symbolic``): dimensions, index data, hash-consed nodes, the element-wise
functions and the handful of structural nodes (``select`` / ``pad`` / ``trunc`` / ``elem`` / ``stack``, broadcasts, segment sums).  What a
stage family (``nutpie_amd.stage_families``) needs in order to build nodes of its own; ``nutpie_amd.symbolic`` re-exports all of it."""

from __future__ import annotations

import math
import weakref
from typing import Any

import numpy as np

_HALF_LOG_2PI = 0.5 * math.log(2.0 * math.pi)


class Dim:
    """A named coordinate of the model: the range one wave-wide loop runs over."""

    def __init__(self, name: str, size, runtime_len: str | None = None, runtime_div: int = 1, runtime_mul: int = 1):
        self.name = name
        self.size = size                  # int, or None for a data dimension whose length comes from the data block
        self.runtime_len = runtime_len    # the data array whose length is the dimension's (times runtime_div: a matrix's rows)
        self.runtime_div = runtime_div
        self.runtime_mul = runtime_mul    # (the product of a data dimension with a fixed-size one: that many values per element)
        self.factors: tuple[Dim, Dim] | None = None   # (rows, cols) of a Model.product
        self._model = None                # (weak) the Model that declared it: where a scan's gradient registers its shifted read
        self._scan_aux: dict[int, tuple] = {}   # row length T -> (index of element t - 1, "first element of a row" data or None)

    def len_c(self) -> str:
        if self.size is not None:
            return str(self.size)
        return f"data.n_{self.runtime_len}" + (f" / {self.runtime_div}" if self.runtime_div != 1 else "") + (f" * {self.runtime_mul}" if self.runtime_mul != 1 else "")

    def len_py(self, data) -> int:
        return self.size if self.size is not None else int(np.asarray(data[self.runtime_len]).size) // self.runtime_div * self.runtime_mul

    def __repr__(self):
        return f"Dim({self.name})"


class Index:
    """Integer data: for every element of ``dim`` the element of ``into`` it refers to."""

    def __init__(self, name: str, dim: Dim, into: Dim):
        self.name, self.dim, self.into = name, dim, into


class Expr:
    """A node of the expression graph.  ``dim`` is None for scalars.  Nodes are hash-consed by ``Model``-independent structural
    keys, so that the gradient graph shares its sub-expressions with the forward graph."""

    _table: "weakref.WeakValueDictionary[tuple, Expr]" = None   # (weak: the nodes of a discarded model are collected with it)
    _count = 0
    __array_ufunc__ = None     # numpy scalars defer to the operators below

    def __new__(cls, op: str, args: tuple = (), dim: Dim | None = None, payload: Any = None):
        key = (op, tuple(id(a) for a in args), id(dim) if dim is not None else None, payload if not isinstance(payload, (Index, Dim)) else id(payload))
        if Expr._table is None:
            Expr._table = weakref.WeakValueDictionary()
        hit = Expr._table.get(key)
        if hit is not None:
            return hit
        self = object.__new__(cls)
        self.op, self.args, self.dim, self.payload = op, tuple(args), dim, payload
        self.id = Expr._count
        Expr._count += 1
        Expr._table[key] = self
        return self

    # ---- construction helpers
    @staticmethod
    def const(v) -> "Expr":
        return Expr("const", (), None, float(v))

    @staticmethod
    def wrap(v) -> "Expr":
        return v if isinstance(v, Expr) else Expr.const(v)

    def is_const(self, v=None):
        return self.op == "const" and (v is None or self.payload == v)

    def _bin(self, op, other, swap=False):
        a, b = Expr.wrap(self), Expr.wrap(other)
        if swap:
            a, b = b, a
        return _binary(op, a, b)

    __add__ = lambda s, o: s._bin("add", o)           # noqa: E731
    __radd__ = lambda s, o: s._bin("add", o, True)    # noqa: E731
    __sub__ = lambda s, o: s._bin("sub", o)           # noqa: E731
    __rsub__ = lambda s, o: s._bin("sub", o, True)    # noqa: E731
    __mul__ = lambda s, o: s._bin("mul", o)           # noqa: E731
    __rmul__ = lambda s, o: s._bin("mul", o, True)    # noqa: E731
    __truediv__ = lambda s, o: s._bin("div", o)       # noqa: E731
    __rtruediv__ = lambda s, o: s._bin("div", o, True)  # noqa: E731

    def __neg__(self):
        return _unary("neg", self)

    def __pow__(self, k):
        if k == 2:
            return self * self
        raise TypeError("only `** 2` is supported: write other powers with exp / log")

    def __getitem__(self, index: Index) -> "Expr":
        if not isinstance(index, Index):
            raise TypeError("an expression is indexed with a Model.index(...) array")
        if self.dim is not index.into:
            raise ValueError(f"index {index.name!r} points into dimension {index.into.name!r}, the expression lives on {self.dim.name if self.dim else 'no dimension'!r}")
        return Expr("gather", (self,), index.dim, index)

    def sum(self) -> "Expr":
        if self.dim is None:
            raise ValueError("sum() of a scalar")
        return Expr("sum", (self,), None, None)

    def max(self, constant: bool = False) -> "Expr":
        """The largest element.  ``constant``: a value the result does not depend on in exact arithmetic (the shift of a softmax or a
        log-sum-exp) — no gradient flows through it; otherwise the gradient goes to the element(s) that attain it."""
        if self.dim is None:
            return self
        return Expr("max", (self,), None, "constant" if constant else None)

    def __repr__(self):
        return f"<{self.op}#{self.id}{'@' + self.dim.name if self.dim else ''}>"


def _join(a: Expr, b: Expr) -> Dim | None:
    if a.dim is None:
        return b.dim
    if b.dim is None or a.dim is b.dim:
        return a.dim
    raise ValueError(f"operands live on different dimensions ({a.dim.name!r}, {b.dim.name!r}): index one into the other")


def _binary(op: str, a: Expr, b: Expr) -> Expr:
    # constant folding and the identities the gradient graph is full of
    if a.op == "const" and b.op == "const":
        x, y = a.payload, b.payload
        return Expr.const({"add": x + y, "sub": x - y, "mul": x * y, "div": x / y if y != 0.0 else math.copysign(math.inf, x)}[op])
    if op == "mul" and b.op == "const" and a.op != "const":
        a, b = b, a                                   # constants first
    if op == "add":
        if a.is_const(0.0):
            return b
        if b.is_const(0.0):
            return a
        if a.op == "rowpack" and b.op == "rowpack" and a.dim is b.dim:     # (the adjoints of the columns of one value, collected)
            return Expr("rowpack", tuple(_binary("add", x, y) for x, y in zip(a.args, b.args)), a.dim, None)
        if a is b:
            return _binary("mul", Expr.const(2.0), a)
    elif op == "sub":
        if b.is_const(0.0):
            return a
        if a.is_const(0.0):
            return _unary("neg", b)
    elif op == "mul":
        if a.is_const(1.0):
            return b
        if b.is_const(1.0):
            return a
        if a.is_const(0.0) or b.is_const(0.0):
            return Expr.const(0.0)
        if a.is_const(-1.0):
            return _unary("neg", b)
        if a.op == "const" and b.op == "mul" and b.args[0].op == "const":
            return _binary("mul", Expr.const(a.payload * b.args[0].payload), b.args[1])     # c1 (c2 x) = (c1 c2) x
        if a.op == "const" and b.op == "neg":
            return _binary("mul", Expr.const(-a.payload), b.args[0])
    elif op == "div":
        if b.is_const(1.0):
            return a
        if a.is_const(0.0):
            return a
        if b.op == "const" and b.payload != 0.0:
            return _binary("mul", a, Expr.const(1.0 / b.payload))     # (the numpy evaluation follows the same graph)
        if a.dim is not None and b.dim is None:
            # one division per evaluation instead of one per element
            return _binary("mul", a, _binary("div", Expr.const(1.0), b))
    return Expr(op, (a, b), _join(a, b))


def _digamma_py(x: float) -> float:
    """psi(x) the way the generated device code computes it (recurrence up to 10, then the asymptotic series)"""
    if x <= 0.0:
        if x == math.floor(x):
            return math.nan
        return _digamma_py(1.0 - x) - math.pi / math.tan(math.pi * x)
    r = 0.0
    while x < 10.0:
        r -= 1.0 / x
        x += 1.0
    f = 1.0 / (x * x)
    return r + math.log(x) - 0.5 / x - f * (1.0 / 12 - f * (1.0 / 120 - f * (1.0 / 252 - f * (1.0 / 240 - f * (1.0 / 132 - f * (691.0 / 32760 - f / 12))))))


_UNARY_FOLD = {"neg": lambda v: -v, "exp": math.exp, "log": math.log, "log1p": math.log1p, "sqrt": math.sqrt,
               "softplus": lambda v: max(v, 0.0) + math.log1p(math.exp(-abs(v))), "sigmoid": lambda v: 1.0 / (1.0 + math.exp(-v)),
               "tanh": math.tanh, "expm1": math.expm1, "erf": math.erf, "erfc": math.erfc, "sin": math.sin, "cos": math.cos, "atan": math.atan,
               "lgamma": math.lgamma, "digamma": _digamma_py, "abs": abs, "sign": lambda v: float((v > 0) - (v < 0))}


def _unary(op: str, a) -> Expr:
    a = Expr.wrap(a)
    if a.op == "const":
        return Expr.const(_UNARY_FOLD[op](a.payload))
    if op == "neg" and a.op == "neg":
        return a.args[0]
    if op == "neg" and a.op == "mul" and a.args[0].op == "const":
        return _binary("mul", Expr.const(-a.args[0].payload), a.args[1])
    if op == "log" and a.op == "exp":      # log sigma of a log-transformed sigma: the raw parameter
        return a.args[0]
    return Expr(op, (a,), a.dim)


def exp(a):
    return _unary("exp", a)


def log(a):
    return _unary("log", a)


def log1p(a):
    return _unary("log1p", a)


def sqrt(a):
    return _unary("sqrt", a)


def softplus(a):
    """log(1 + e^a), evaluated as max(a, 0) + log1p(e^-|a|)."""
    return _unary("softplus", a)


def sigmoid(a):
    return _unary("sigmoid", a)


def tanh(a):
    return _unary("tanh", a)


def expm1(a):
    return _unary("expm1", a)


def erf(a):
    return _unary("erf", a)


def erfc(a):
    return _unary("erfc", a)


def sin(a):
    return _unary("sin", a)


def cos(a):
    return _unary("cos", a)


def atan(a):
    return _unary("atan", a)


def lgamma(a):
    return _unary("lgamma", a)


def digamma(a):
    return _unary("digamma", a)


def absolute(a):
    return _unary("abs", a)


def sign(a):
    return _unary("sign", a)


def _join3(c: Expr, a: Expr, b: Expr) -> Dim | None:
    d = None
    for v in (c, a, b):
        if v.dim is not None:
            if d is not None and v.dim is not d:
                raise ValueError(f"operands live on different dimensions ({d.name!r}, {v.dim.name!r})")
            d = v.dim
    return d


def select(c, a, b, strict: bool = True) -> Expr:
    """``a`` where ``c > 0`` (``strict``) resp. ``c >= 0``, else ``b`` — element-wise; the condition carries no gradient."""
    c, a, b = Expr.wrap(c), Expr.wrap(a), Expr.wrap(b)
    if c.op == "const":
        return a if (c.payload > 0.0 if strict else c.payload >= 0.0) else b
    if a is b:
        return a
    return Expr("sel_gt" if strict else "sel_ge", (c, a, b), _join3(c, a, b))


def pad(v: Expr, dim: Dim) -> Expr:
    """``v`` (on a shorter dimension of fixed size) on the first elements of ``dim``, zero on the rest."""
    v = Expr.wrap(v)
    if v.dim is None or v.dim is dim:
        return v
    if v.dim.size is None or dim.size is None or v.dim.size > dim.size:
        raise ValueError("pad() goes from a fixed-size dimension to a longer fixed-size dimension")
    return Expr("pad", (v,), dim, None)


def trunc(v: Expr, dim: Dim) -> Expr:
    """The first ``dim.size`` elements of ``v`` (on a longer dimension of fixed size), as a value on ``dim``."""
    v = Expr.wrap(v)
    if v.dim is None or v.dim is dim:
        return v
    if v.dim.size is None or dim.size is None or v.dim.size < dim.size:
        raise ValueError("trunc() goes from a fixed-size dimension to a shorter fixed-size dimension")
    if v.op == "pad" and v.args[0].dim is dim:
        return v.args[0]
    return Expr("trunc", (v,), dim, None)


def where_lt(dim: Dim, k: int, a, b) -> Expr:
    """``a`` on the first ``k`` elements of ``dim``, ``b`` on the rest."""
    a, b = Expr.wrap(a), Expr.wrap(b)
    for v in (a, b):
        if v.dim is not None and v.dim is not dim:
            raise ValueError("where_lt: operands must be scalars or live on `dim`")
    return Expr("where_lt", (a, b), dim, int(k))


def _bcast(a: Expr, dim: Dim) -> Expr:
    return a if a.dim is dim else Expr("bcast", (a,), dim, None)


def _dim_len(dim: Dim) -> Expr:
    return Expr.const(dim.size) if dim.size is not None else Expr("dimlen", (), None, dim)


def _segsum(e: Expr, index: Index) -> Expr:
    if e.is_const(0.0):
        return e
    return Expr("segsum", (_bcast(e, index.dim),), index.into, index)


def elem(v: Expr, c: int) -> Expr:
    """Element ``c`` of a vector on a fixed-size dimension, as a scalar."""
    if v.dim is None:
        return v
    if v.dim.size is None or not 0 <= c < v.dim.size:
        raise ValueError("elem() needs a vector on a fixed-size dimension and an index inside it")
    if v.op == "vparam" and c >= v.payload[1]:
        return Expr.const(0.0)            # the padding element of a zero-sum parameter
    if v.op == "stack":
        return v.args[c]
    if v.op == "bcast":
        return v.args[0]
    return Expr("elem", (v,), None, int(c))


def stack(scalars, dim: Dim) -> Expr:
    """The vector on ``dim`` whose elements are the given scalars."""
    scalars = [Expr.wrap(v) for v in scalars]
    if dim.size is None or len(scalars) != dim.size or any(v.dim is not None for v in scalars):
        raise ValueError("stack() needs one scalar per element of a fixed-size dimension")
    if all(v.is_const(0.0) for v in scalars):
        return Expr.const(0.0)
    return Expr("stack", tuple(scalars), dim, None)


def _topo(roots) -> list[Expr]:
    seen, order = set(), []
    stack = [(r, False) for r in roots]
    while stack:
        n, done = stack.pop()
        if done:
            order.append(n)
            continue
        if n.id in seen:
            continue
        seen.add(n.id)
        stack.append((n, True))
        for a in n.args:
            if a.id not in seen:
                stack.append((a, False))
    return order
