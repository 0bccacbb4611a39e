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
