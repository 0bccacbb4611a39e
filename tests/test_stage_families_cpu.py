"""The table of stage families (nutpie_amd/stage_families: Family, FAMILIES) against what it describes: the chain headers of
nutpie_amd/csrc, their #include lines, the ops of the families and the header list a library's cache key hashes.  DESIGN.md §11.5."""
import glob
import os
import re

from nutpie_amd import density, stage_families as SF
from nutpie_amd import symbolic as S

CSRC = os.path.join(os.path.dirname(os.path.abspath(S.__file__)), "csrc")


def chain_includes(header):
    """the chain headers a header of csrc/ includes"""
    with open(os.path.join(CSRC, header)) as f:
        return set(re.findall(r'^\s*#\s*include\s+"(chain_\w+\.h)"', f.read(), flags=re.M))


def test_the_table_is_in_the_order_of_the_include_lines():
    assert [f.name for f in SF.FAMILIES] == ["linalg", "scan", "matvec", "hmm", "kalman"]


def test_every_header_exists_and_every_chain_header_belongs_to_exactly_one_family():
    for f in SF.FAMILIES:
        assert os.path.isfile(os.path.join(CSRC, f.header)), f.header
    on_disk = sorted(os.path.basename(p) for p in glob.glob(os.path.join(CSRC, "chain_*.h")))
    assert on_disk == sorted(f.header for f in SF.FAMILIES)      # (sorted lists: a header named by two families is one too many)


def test_header_deps_are_the_chain_headers_the_header_includes():
    for f in SF.FAMILIES:
        assert len(set(f.header_deps)) == len(f.header_deps)
        assert set(f.header_deps) == chain_includes(f.header), f.header
    assert SF.family_of("kalman_fwd").header_deps == ("chain_hmm.h",)


def test_ops_and_readers_are_disjoint_and_map_back_to_their_family():
    names = [op for f in SF.FAMILIES for op in f.ops + f.readers]
    assert len(names) == len(set(names))
    assert SF._STAGES == tuple(op for f in SF.FAMILIES for op in f.ops) == S._STAGES
    assert SF._STAGES == S._MATOPS + S._SCANOPS + S._MVOPS + S._HMMOPS + S._KALOPS
    assert set(SF._READERS) == {"hmm_part", "hmm_ll", "kalman_part"}
    for f in SF.FAMILIES:
        for op in f.ops + f.readers:
            assert SF.family_of(op) is f
        assert set(f.adjoint) <= set(f.ops + f.readers)
    assert SF.family_of("add") is None and SF.family_of("rhscol") is None


def test_the_hashed_header_list_is_the_header_followed_by_its_deps():
    assert density.chain_headers is SF.chain_headers      # (what compile_density appends to the files it hashes)
    assert SF.chain_headers('#include "chain_kalman.h"\n') == ["chain_kalman.h", "chain_hmm.h"]
    assert SF.chain_headers('#include "chain_scan.h"\n') == ["chain_scan.h"]
    assert SF.chain_headers("__device__ double nphip_density() { return 0.0; }") == []
    for f in SF.FAMILIES:
        assert SF.chain_headers(f'#include "{f.header}"') == [f.header, *f.header_deps]
    # several families: table order, whatever the order in the source (a model with an HMM and a Kalman stage hashes chain_hmm.h twice)
    both = '#include "chain_kalman.h"\n#include "chain_hmm.h"\n#include "chain_linalg.h"\n'
    assert SF.chain_headers(both) == ["chain_linalg.h", "chain_hmm.h", "chain_kalman.h", "chain_hmm.h"]


# ---- the torch side: Family.torch_rules and the torch tracer's own table (nutpie_amd/torch_trace.py: _RULES, _lower)
FAMILY_STRINGS = ("hmm", "kalman", "linear_recurrence", "cholesky", "solve_lower")
#: a family rule of these names may decline (return NotImplemented); the tracer's own rule of the same name is then asked
DECLINING_PAIRS = {"cumsum", "linalg_solve_triangular"}


def test_no_torch_op_is_claimed_by_two_families():
    names = [name for f in SF.FAMILIES for name in f.torch_rules]
    assert len(names) == len(set(names))
    assert set(SF.family_of("chol").torch_rules) == {"linalg_cholesky_ex", "linalg_cholesky", "cholesky", "linalg_solve_triangular"}
    assert set(SF.family_of("scan").torch_rules) == {"cumsum", "linear_recurrence"}
    assert set(SF.family_of("hmm_fwd").torch_rules) == {"hmm_marginal"} and set(SF.family_of("kalman_fwd").torch_rules) == {"kalman_marginal"}
    assert SF.family_of("matvec").torch_rules == {}
    # the products are reached through the record's hook: of the families only matvec has one
    assert [f.name for f in SF.FAMILIES if f.torch_matmul is not SF._declines] == ["matvec"]


def test_a_name_in_a_family_and_in_the_general_table_is_a_documented_declining_pair():
    from nutpie_amd import torch_trace as TT

    shared = {name for f in SF.FAMILIES for name in f.torch_rules} & set(TT._RULES)
    assert shared == DECLINING_PAIRS


def test_every_custom_op_a_family_module_registers_has_a_rule_in_that_family():
    import inspect
    import sys

    found = 0
    for f in SF.FAMILIES:
        source = inspect.getsource(sys.modules[f"nutpie_amd.stage_families.{f.name}"])
        for op in re.findall(r'custom_op\(\s*"nutpie_amd::(\w+)"', source):
            assert op in f.torch_rules, (f.name, op)
            found += 1
    assert found == 3      # linear_recurrence, hmm_marginal, kalman_marginal
    with open(os.path.join(os.path.dirname(CSRC), "torch_trace.py")) as fh:
        assert "custom_op(" not in fh.read()


def _registered_names(TT):
    """the names handed to ``@_rule(...)`` in torch_trace.py, one entry per registration (``*TABLE`` registers the table's keys)"""
    import ast
    import inspect

    names = []
    for fn in ast.parse(inspect.getsource(TT)).body:
        for dec in getattr(fn, "decorator_list", []):
            if isinstance(dec, ast.Call) and getattr(dec.func, "id", None) == "_rule":
                for a in dec.args:
                    names += list(getattr(TT, a.value.id)) if isinstance(a, ast.Starred) else [a.value]
    return names


def test_the_general_table_registers_each_name_once():
    import pytest

    from nutpie_amd import torch_trace as TT

    names = _registered_names(TT)
    assert len(names) == len(set(names)) == len(TT._RULES) and set(names) == set(TT._RULES)
    before = dict(TT._RULES)
    with pytest.raises(AssertionError, match="two rules for add"):
        TT._rule("add")(lambda c: None)
    assert TT._RULES == before


def test_the_names_the_ladder_listed_twice_keep_the_arm_that_was_reachable():
    """In the parent's ``_run`` ladder (after the block for a partitioned x) ``alias`` stood in the data-movement arm — ``it.move(a0,
    lambda t: tgt(t, ...))``, now ``_move`` — and again, unreachably, in the arm of the conversions ``clone`` / ``to`` / ``double``.
    ``clone``, ``detach``, ``contiguous``, ``_to_copy`` and ``lift_fresh_copy`` stood in no ladder arm but the conversions' — ``it.sym(a0)``
    unless a ``_Bool`` stays one, now ``_convert``; their other listing was in the block for a partitioned x, which came first and
    still does (``_x_rule``: an ``_X`` that keeps all elements stays an ``_X``)."""
    from nutpie_amd import torch_trace as TT

    assert TT._RULES["alias"] is TT._move
    for name in ("clone", "detach", "contiguous", "_to_copy", "lift_fresh_copy"):
        assert TT._RULES[name] is TT._convert, name
    for name in ("alias", "clone", "detach", "contiguous", "_to_copy", "lift_fresh_copy"):
        assert not any(name in f.torch_rules for f in SF.FAMILIES)
    # the _copy suffix rule of _run leaves _to_copy and lift_fresh_copy their names: both are keys of the table as they are
    assert "_to" not in TT._RULES and "lift_fresh" in TT._RULES
    # the partitioned x first: clone of x stays the position vector, whatever the tables say
    it = TT._Interp(4, False, [])
    import torch

    x = TT._X((1, 4))
    got = TT._x_rule(TT._Ctx(it, None, torch.ops.aten.clone.default, "clone.default", "clone", (x,), {}))
    assert isinstance(got, TT._X) and got.shape == (1, 4)


def test_importing_the_front_end_does_not_import_torch():
    import subprocess
    import sys

    code = ("import sys; import nutpie_amd.symbolic, nutpie_amd.stage_families, nutpie_amd.trace_values; "
            "assert 'torch' not in sys.modules, 'torch was imported'; "
            "assert all(isinstance(f.torch_rules, dict) for f in nutpie_amd.stage_families.FAMILIES)")
    root = os.path.dirname(os.path.dirname(CSRC))
    r = subprocess.run([sys.executable, "-c", code], cwd=root, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_the_tracer_names_no_family():
    import ast

    path = os.path.join(os.path.dirname(CSRC), "torch_trace.py")
    with open(path) as fh:
        text = fh.read()
    doc = ast.get_docstring(ast.parse(text), clean=False)
    assert doc and text.count(doc) == 1
    text = text.replace(doc, "")
    begin, end = text.index("# ---- re-exports"), text.index("# ---- end of the re-exports")
    reexports, rest = text[begin:end], text[:begin] + text[end:]
    for name in ("linear_recurrence", "hmm_marginal", "kalman_marginal"):
        assert name in reexports
    for s in FAMILY_STRINGS:
        assert s not in rest, s
    for call in ("S._scan", "S._hmm_", "S._kalman_", "S.cholesky", "S.solve_lower", "m.matrix"):
        assert call not in rest, call
    from nutpie_amd import torch_trace as TT

    assert TT.__all__ == ["trace", "traced_model", "UnsupportedTorchOp", "TraceResult", "linear_recurrence", "hmm_marginal", "kalman_marginal"]
    from nutpie_amd.torch_trace import UnsupportedTorchOp, hmm_marginal, kalman_marginal, linear_recurrence  # noqa: F401
    from nutpie_amd import trace_values

    assert TT._Sym is trace_values._Sym and TT.UnsupportedTorchOp is trace_values.UnsupportedTorchOp


def test_a_declined_family_rule_falls_through_to_the_general_rule():
    """``torch.cumsum`` of traced values: along 8 elements the scan family declines and the gather / segment-sum rule builds the sum
    (no stage node); along 65 the family takes it (one scan stage).  Looked up in the model's nodes, nothing is compiled."""
    import torch

    from nutpie_amd.torch_trace import trace

    def stages(n):
        tr = trace(lambda x: -0.5 * (torch.cumsum(x, dim=-1) ** 2).sum(-1), n)
        return [node.op for node in S._topo([tr.model.logp_expr()]) if node.op in SF._STAGES]

    assert stages(8) == []
    assert stages(65) == ["scan"]
