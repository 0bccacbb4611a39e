"""The values of a torch trace (:mod:`nutpie_amd.torch_trace`) and its two exceptions: what the tracer's rules and the stage families'
torch rules (``Family.torch_rules``) both handle.  Imports neither torch nor the tracer, so that the family modules can use it."""

from __future__ import annotations

import numpy as np


class UnsupportedTorchOp(NotImplementedError):
    """The traced function uses an operation (or a form of one) the IR has no counterpart for."""


class _NeedWholeVector(Exception):
    """the position vector is used in a way the partition into parameters cannot express: trace again with x as ONE parameter"""


def _numel(shape) -> int:
    return int(np.prod(shape, dtype=np.int64)) if len(shape) else 1


class _Sym:
    """a traced float tensor: ``expr`` on the dimension of ``numel(shape)`` elements (row-major), or a scalar for all of them"""

    __slots__ = ("expr", "shape")

    def __init__(self, expr, shape):
        self.expr, self.shape = expr, tuple(int(v) for v in shape)


class _Bool:
    """a traced boolean tensor: a tree of comparisons of traced values (``gt`` / ``ge`` of an expression against zero, ``not``,
    ``and``, ``or``)"""

    __slots__ = ("tree", "shape")

    def __init__(self, tree, shape):
        self.tree, self.shape = tree, tuple(int(v) for v in shape)


class _X:
    """the position vector (or a view of it that keeps all of its elements in order)"""

    __slots__ = ("shape",)

    def __init__(self, shape):
        self.shape = tuple(int(v) for v in shape)


def _is_traced(v) -> bool:
    """a value that depends on the position vector (anything else is a constant of the trace)"""
    return isinstance(v, (_Sym, _Bool, _X))
