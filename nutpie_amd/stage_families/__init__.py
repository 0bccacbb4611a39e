"""Stage families of the compiled-density front end: the device routines that run between two generated loops.

One :class:`Family` record per family, in its own module next to the functions that build its nodes; ``FAMILIES`` is the table the front
end (``nutpie_amd.symbolic``: the generator, ``gradient``, ``evaluate``, ``Model.compile``) and the library cache (``nutpie_amd.density``)
and the torch tracer (``nutpie_amd.torch_trace``) ask instead of naming a family.  Adding a family = one module with one record, and one
entry in ``FAMILIES``."""

from __future__ import annotations

import dataclasses
from typing import Callable


def _nothing(*_):
    return None


def _no_lengths(payload) -> set[int]:
    return set()


def _no_limit(nodes, waves_per_chain):
    return waves_per_chain


def _declines(*_):
    return NotImplemented


def _own_header(nodes):
    return None


@dataclasses.dataclass(frozen=True)
class Family:
    name: str
    #: the stage ops: nodes whose value one call of a routine of ``header`` stores between two loops
    ops: tuple[str, ...]
    #: the chain header of ``csrc/`` that holds the routines ...
    header: str
    #: ``call(gen, node) -> str``: the line of generated source that runs the stage (``gen`` the generator: ``store_name``, ``sref``, ``order``, ``m``)
    call: Callable
    #: ``numpy(node, args, data, N, dim_len) -> array``: the host evaluation of a stage op or a reader for ``N`` positions (``args``: the values
    #: of ``node.args``, ``[N]`` or ``[N, len]``; ``dim_len(dim)`` the length of a dimension under ``data``)
    numpy: Callable
    #: op -> ``rule(node, g, ad)``: the reverse-mode rule of the ops and readers that have one.  ``g`` is the node's adjoint; ``ad.acc(target, e)``
    #: adds to a target's, ``ad.reduce_to(e, from_dim, target)`` folds a contribution onto the target's dimension, ``ad.pending(stage)`` is the
    #: dict in which readers leave adjoints for ``finish`` (below).  A rule returns False for a node it does not differentiate.
    adjoint: dict[str, Callable]
    #: what ``gradient`` says of an op or reader without a rule
    refusal: str
    #: ``check(nodes, waves_per_chain, **options) -> waves_per_chain``: the family's limits on the model's stage nodes (a ``ValueError``),
    #: and the waves per chain it forces (returned; otherwise the argument)
    check: Callable = _no_limit
    #: the keywords of ``Model.compile`` that ``check`` is given by name (a switch that belongs to the family)
    options: tuple[str, ...] = ()
    #: further headers of ``csrc/`` with routines of the family (hashed into a library's cache key when the source includes them) ...
    more_headers: tuple[str, ...] = ()
    #: ... and ``includes(nodes) -> [header] | None``: which of ``header`` and ``more_headers`` a source with these stage nodes includes
    #: (None: ``header``)
    includes: Callable = _own_header
    #: ops that read a stored stage result element-wise, in the loop over their own dimension
    readers: tuple[str, ...] = ()
    #: ... and the other chain headers that header includes (hashed with it into a library's cache key)
    header_deps: tuple[str, ...] = ()
    #: ``read(node, name, array, j) -> (loads, arithmetic)``: the generated lines that define ``const double <name>`` for a reader, element ``j``
    #: of its dimension, from the stage's stored ``array``
    read: Callable = _nothing
    #: ``finish(stage, pending, ad)``: called when the reverse traversal reaches a stage node for which readers left adjoints — a family
    #: whose adjoint is ONE node built from all of them (the Kalman filter's backward stage)
    finish: Callable = _nothing
    #: ``section(node) -> str | None``: the label under which ``Model.profile`` times the stage on its own
    section: Callable = _nothing
    #: ``series_lengths(payload) -> set[int]``: lengths of the dimensions a stage's series live on (their loops are unrolled alike whatever the length)
    series_lengths: Callable = _no_lengths
    #: results may be too long for the LDS of the generated expand function (``Model._finish`` then checks, and expands on the host);
    #: or ``long_results(node) -> bool``: which of the family's stages are
    long_results: bool | Callable = True
    #: base name of a torch op (``cumsum``, ``linalg_cholesky``, the family's own ``nutpie_amd::`` custom ops) -> ``rule(c)``: the lowering
    #: the torch tracer asks BEFORE its own table, the families in table order.  ``c`` is the tracer's rule context (``c.it`` the
    #: interpreter, ``c.args`` / ``c.kwargs`` the node's evaluated arguments, ``c.name`` / ``c.base`` the op's names); a rule returns the
    #: node's value, or ``NotImplemented`` to decline, and the tracer goes on to the next rule of that name (``cumsum`` along a short
    #: axis).  A rule uses of the interpreter ``it.sym``, ``it.move``, ``it.dim``, ``it.index``, ``it.broadcast``, ``it.m``,
    #: ``it.fresh_name`` and the attributes ``it.torch`` and ``it.whole``, and the values of ``nutpie_amd.trace_values``.
    torch_rules: dict[str, Callable] = dataclasses.field(default_factory=dict)
    #: ``torch_matmul(it, a, b, sa, sb) -> value | NotImplemented``: a product ``a @ b`` (shapes ``sa``, ``sb``, at least one operand
    #: traced) the family has a stage for; the tracer asks before it multiplies element-wise and sums
    torch_matmul: Callable = _declines


def read_part(n, name: str, array: str, j: str):
    """``Family.read`` of a reader whose payload is an offset into the stage's packed result"""
    return [f"        const double {name} = {array}[{n.payload} + {j}];"], []


def np_part(n, args, dim_len):
    """``Family.numpy`` of such a reader"""
    return args[0][:, n.payload:n.payload + dim_len(n.dim)]


from nutpie_amd.stage_families import hmm, kalman, linalg, matvec, scan  # noqa: E402  (the family modules import Family from here)

#: in the order of the ``#include`` lines of a generated source
FAMILIES: tuple[Family, ...] = (linalg.FAMILY, scan.FAMILY, matvec.FAMILY, hmm.FAMILY, kalman.FAMILY)

_STAGES: tuple[str, ...] = tuple(op for f in FAMILIES for op in f.ops)
_READERS: tuple[str, ...] = tuple(op for f in FAMILIES for op in f.readers)
_FAMILY_OF: dict[str, Family] = {op: f for f in FAMILIES for op in f.ops + f.readers}


def family_of(op: str) -> Family | None:
    """the family of a stage op or a reader op, None for any other op"""
    return _FAMILY_OF.get(op)


def chain_headers(source: str) -> list[str]:
    """the chain headers a generated source compiles with, in the order a library's cache key hashes them: for every family whose
    ``#include`` line is in ``source``, its header and then the headers that one includes; then the families' further headers"""
    return ([h for f in FAMILIES if f'#include "{f.header}"' in source for h in (f.header,) + f.header_deps]
            + [h for f in FAMILIES for h in f.more_headers if f'#include "{h}"' in source])


def has_long_results(n) -> bool:
    """a stage node whose result may not fit the LDS of the generated expand function (``Family.long_results``)"""
    long = family_of(n.op).long_results
    return bool(long(n)) if callable(long) else bool(long)
