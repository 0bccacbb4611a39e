"""Probe cases for the wide matrix routines (csrc/wide_chain_linalg.h), on the probes of tests/chain_stage_probes.py: one probe per number
of waves per chain, and a small one for the containment test.  tests/test_gpu_matrix_wide.py compares the outputs with the CPU restatement of
the order contract (``oracle.chain_*``: K is a run-time argument there) bit for bit."""
from __future__ import annotations

import functools

import numpy as np

from chain_stage_probes import Case, Probe, spd, with_lds

HEADER = "wide_chain_linalg.h"
#: on and beside the panel width (32), the row block of one wave (64) and the limit (128)
WIDE_K = {1: [1, 17, 32, 33, 63, 64, 65, 100, 127, 128], 2: [33, 65, 128], 4: [33, 65, 128]}
ALL_K = WIDE_K[1]
WIDE_N = [1, 2, 63, 64, 65, 129]


def right_hand_sides(K: int) -> list[int]:
    """The thinning rule: a K >= 33 takes two N of the list, by its position among those K — every N meets a K <= 65 and a K >= 100 (the
    same pairs at every W)."""
    j = [k for k in ALL_K if k >= 33].index(K)
    return [WIDE_N[(j + m) % len(WIDE_N)] for m in (0, 3)]


def _cholesky_case(name, K, A):
    import oracle

    return Case(name, f"nphip_lw::cholesky<{K}>(P1, PO, lane);", np.zeros(0), A, np.zeros(0), K * K,
                lambda p0, p1, p2: oracle.chain_cholesky(p1)[0], poison=((K // 2) * (K + 1), 1))


def wide_cases(W: int):
    """``cholesky`` and ``cholesky_adj`` at every K of the probe with a random SPD matrix and one of condition 1e12 (the same
    instantiation, other data; ``cholesky_adj`` with a non-symmetric ``Lbar``); the routines with right-hand sides at every K >= 33 with
    the two N of ``right_hand_sides``, ``solve_lower_t`` in both layouts.  Device memory, and LDS where the arrays fit."""
    import oracle

    rng = np.random.default_rng(500)      # (the same operands at every W: the result is no function of W)
    cases = []
    none = np.zeros(0)
    for K in ALL_K:
        mine = []
        for cond in (None, 1e12):
            A = spd(rng, K, cond)
            L = oracle.chain_cholesky(A)[0]
            assert np.isfinite(L).all()
            tag = f"K={K} cond={cond or 'random'}"
            mine.append(_cholesky_case(f"cholesky {tag}", K, A))
            Lbar = rng.normal(size=(K, K))      # not symmetric, and with an upper triangle that must not count
            mine.append(Case(f"cholesky_adj {tag}", f"nphip_lw::cholesky_adj<{K}>(P0, P1, PO, lane);", L, Lbar, none, K * K,
                             lambda p0, p1, p2: oracle.chain_cholesky_adj(p0, p1)))
        for m, N in enumerate(right_hand_sides(K) if K >= 33 else []):
            L = oracle.chain_cholesky(spd(rng, K, 1e12 if m == 1 else None))[0]
            B, G2 = rng.normal(size=(K, N)), rng.normal(size=(K, N))
            tag = f"K={K} N={N}"
            mine.append(Case(f"solve_lower {tag}", f"nphip_lw::solve_lower<{K}, {N}>(P0, P1, PO, lane);", L, B, none, K * N,
                             lambda p0, p1, p2: oracle.chain_solve_lower(p0, p1)))
            mine.append(Case(f"solve_lower_t columns {tag}", f"nphip_lw::solve_lower_t<{K}, {N}, {N}, 1>(P0, P1, PO, lane);", L, B, none, K * N,
                             lambda p0, p1, p2: oracle.chain_solve_lower_t(p0, p1)))
            mine.append(Case(f"solve_lower_t rows {tag}", f"nphip_lw::solve_lower_t<{K}, {N}, 1, {K}>(P0, P1, PO, lane);", L, np.ascontiguousarray(B.T), none, K * N,
                             lambda p0, p1, p2: oracle.chain_solve_lower_t(p0, p1, by_rows=True)))
            mine.append(Case(f"solve_lower_adj_l {tag}", f"nphip_lw::solve_lower_adj_l<{K}, {N}>(P1, P2, PO, lane);", none, B, G2, K * K,
                             lambda p0, p1, p2: oracle.chain_solve_lower_adj_l(p1, p2)))
        if K in WIDE_K[W]:
            cases += mine
    return with_lds(cases)


def containment_cases():
    """the middle pivot of a random SPD matrix (every poison value fails it: earlier columns are subtracted from it) and of a diagonal
    one (the pivot is the value itself: a positive subnormal factors), at K = 128 and K = 33"""
    rng = np.random.default_rng(501)
    cases = []
    for K in (128, 33):
        cases.append(_cholesky_case(f"cholesky K={K} random", K, spd(rng, K)))
        cases.append(_cholesky_case(f"cholesky diagonal K={K}", K, np.diag(rng.uniform(0.5, 2.0, K))))
    return with_lds(cases)


@functools.lru_cache(maxsize=None)
def probe(W: int) -> Probe:
    return Probe(f"wide linalg W={W}", W, [HEADER], wide_cases(W))


@functools.lru_cache(maxsize=None)
def containment_probe() -> Probe:
    return Probe("wide linalg containment", 1, [HEADER], containment_cases())
