"""Probe densities that reach the chain stages (csrc/chain_scan.h, chain_matvec.h, chain_linalg.h) directly.

A probe is a density given as HIP source (``nutpie_amd.from_density_source``): its ``nphip_density`` copies a case's operands from the
data into the chain's scratch — LDS, or the chain's block of device memory: the routines are instantiated separately for either pointer
type —, calls ONE stage, copies the stage's output out, and goes on to the next case; it returns a constant.  It is compiled by the
project's own JIT path with its flags, and ``logp_and_grad(points, return_data=True)`` hands the raw outputs back for every chain of
the launch.  ``tests/test_gpu_chain_stages.py`` compares them with the CPU restatement of the contracts (``oracle.chain_*``) bit for bit.

Where the outputs go: into the data array ``out`` (one block per chain, ``NPHIP_CHAIN_SLOT``), not into ``grad``.  A gradient has as many
elements as the density has dimensions, and a library is always built with its resident kernel for that many dimensions; one probe
holds dozens of cases with outputs of up to 100 003 doubles.  The densities have three dimensions: the chain's parameters.

How chains differ: the operands are data, shared by all chains; ``x[0]`` scales the "scaled" operands (one exact multiplication that
numpy repeats), so every chain computes different numbers.  ``x[2] != 0`` poisons the chain: the elements ``i`` of the scaled operand
with ``i // poison_group == poison_index`` become ``x[1]`` (a NaN, an infinity, a zero ...) — values fed in as data, in one chain of a
launch; nothing here provokes a fault.

One probe per (family, waves per chain): every compilation builds the whole engine kernel around the density, the cases of a probe share
it.  Each distinct (routine instantiation, memory) is a function of its own (not inlined: the density stays small), called once per case.
"""
from __future__ import annotations

import functools
from dataclasses import dataclass, field
from typing import Callable

import numpy as np

LDS_DOUBLES = 4096      # LDS scratch per chain: four chains of a workgroup at one wave per chain take 128 KB of the 160 KB
N_CHAINS = 64
POISONED_CHAIN = 5      # (at one wave per chain, chains 4 .. 7 share a workgroup)


@dataclass
class Case:
    name: str
    call: str                       # C++: the stage call on P0, P1, P2 (inputs), PO (output), MX (the data matrix), n (its rows)
    p0: np.ndarray                  # operand taken as it is
    p1: np.ndarray                  # operand scaled by x[0]; the one that can be poisoned
    p2: np.ndarray                  # second scaled operand
    n_out: int
    oracle: Callable                # (p0, p1, p2) -> the expected output (any shape, n_out elements)
    mem: str = "dev"                # "lds" or "dev"
    poison: tuple = (0, 1)          # (index, group)
    matrix: str = ""                # "X" / "Xt": which copy of the data matrix MX points into
    X: np.ndarray | None = None     # the n x K matrix
    # filled by Probe
    offs: dict = field(default_factory=dict)

    @property
    def doubles(self):
        return self.p0.size + self.p1.size + self.p2.size + self.n_out


def _f(v: float) -> str:
    return float(v).hex()


PRELUDE = r"""
template <class P> __device__ __forceinline__ void probe_load(P dst, const double* src, int n, double s, int p, int pr, double pv, int lane) {
    for (int i = lane; i < n; i += NPHIP_CHAIN_THREADS) dst[i] = (p >= 0 && i / pr == p) ? pv : src[i] * s;
}
template <class P> __device__ __forceinline__ void probe_store(double* dst, P src, int n, int lane) {
    for (int i = lane; i < n; i += NPHIP_CHAIN_THREADS) dst[i] = src[i];
}
"""


class Probe:
    def __init__(self, name: str, waves: int, includes: list[str], cases: list[Case]):
        self.name, self.waves, self.cases = name, waves, cases
        pools = {"a": [np.zeros(1)], "b": [np.zeros(1)], "X": [np.zeros(1)], "Xt": [np.zeros(1)]}
        size = {k: 1 for k in pools}

        def put(pool, arr):
            arr = np.ascontiguousarray(arr, dtype=np.float64).reshape(-1)
            off = size[pool]
            if arr.size:
                pools[pool].append(arr)
                size[pool] += arr.size
            return off

        fns: dict[tuple, str] = {}
        body, defs = [], []
        out_off = 0
        self.scratch = max([c.doubles for c in cases if c.mem == "dev"] + [1])
        for k, c in enumerate(cases):
            assert c.mem == "dev" or c.doubles <= LDS_DOUBLES, c.name
            c.offs = {"p0": put("a", c.p0), "p1": put("b", c.p1), "p2": put("b", c.p2), "out": out_off}
            ox = 0
            if c.matrix:
                ox = put("X", c.X) if c.matrix == "X" else put("Xt", c.X.T)
            out_off += c.n_out
            key = (c.call, c.mem)
            if key not in fns:
                fns[key] = f"probe_fn{len(fns)}"
                base = "NPHIP_LDS_PTR(double, lds)" if c.mem == "lds" else "dev"
                defs.append(f"""
__device__ __noinline__ void {fns[key]}(const NphipData& data, double s, double pv, int p, int pr, int o0, int n0, int o1, int n1, int o2, int n2,
                                        int no, int ox, int n, double* out, double* lds, double* dev, int lane) {{
    const auto P0 = {base};
    const auto P1 = P0 + n0;
    const auto P2 = P1 + n1;
    const auto PO = P2 + n2;
    const double* const MX = data.{c.matrix or 'X'} + ox;
    probe_load(P0, data.a + o0, n0, 1.0, -1, 1, 0.0, lane);
    probe_load(P1, data.b + o1, n1, s, p, pr, pv, lane);
    probe_load(P2, data.b + o2, n2, s, -1, 1, 0.0, lane);
    nphip_chain_barrier();
    {c.call}
    probe_store(out, PO, no, lane);
    nphip_chain_barrier();
    (void)MX; (void)n;
}}""")
            n_rows = c.X.shape[0] if c.X is not None else 0
            body.append(f"    {fns[key]}(data, s, pv, flag ? {c.poison[0]} : -1, {c.poison[1]}, {c.offs['p0']}, {c.p0.size}, {c.offs['p1']}, {c.p1.size}, "
                        f"{c.offs['p2']}, {c.p2.size}, {c.n_out}, {ox}, {n_rows}, out + {c.offs['out']}, lds, dev, lane);   // {k}: {c.name} [{c.mem}]")
        self.n_out = max(out_off, 1)
        self.data = {k: np.concatenate(v) for k, v in pools.items()}
        self.data["out"] = np.zeros(N_CHAINS * self.n_out)
        self.source = "\n".join([*(f'#include "{h}"' for h in includes), PRELUDE, *defs, f"""
__device__ double nphip_density(const NphipData& data, int dim, const double* x, double* grad, double* lds, const double* shared, int lane) {{
    const double s = x[0], pv = x[1];
    const bool flag = x[2] != 0.0;
    const int chain = NPHIP_CHAIN_SLOT;
    double* const dev = (double*)data.scratch__ + (size_t)chain * {self.scratch};
    double* const out = (double*)data.out + (size_t)chain * {self.n_out};
""", *body, """    if (lane < dim) grad[lane] = 0.0;
    return 0.0;
}
"""])

    @functools.cached_property
    def model(self):
        from nutpie_amd import from_density_source

        return from_density_source(3, self.source, self.data, lds_doubles_per_chain=LDS_DOUBLES, scratch_doubles_per_chain=self.scratch,
                                   waves_per_chain=self.waves)

    def run(self, points):
        """the raw outputs [N_CHAINS, n_out] of one launch"""
        points = np.asarray(points, dtype=np.float64)
        assert points.shape == (N_CHAINS, 3)
        _, _, data = self.model.logp_and_grad(points, return_data=True)
        return data["out"].reshape(N_CHAINS, self.n_out)

    def operands(self, case: Case, point):
        s, pv, flag = point
        p1 = case.p1.reshape(-1) * s
        if flag != 0.0:
            p1[np.arange(p1.size) // case.poison[1] == case.poison[0]] = pv
        return case.p0.copy(), p1.reshape(case.p1.shape), case.p2 * s

    def expected(self, case: Case, point):
        return np.asarray(case.oracle(*self.operands(case, point)), dtype=np.float64).reshape(-1)

    def got(self, out, case: Case, chain: int):
        return out[chain, case.offs["out"]:case.offs["out"] + case.n_out]


def clean_points(seed=0):
    rng = np.random.default_rng(seed)
    x = np.zeros((N_CHAINS, 3))
    x[:, 0] = rng.uniform(0.5, 1.5, N_CHAINS)
    x[0, 0] = 1.0
    return x


def poisoned_points(value, seed=0):
    x = clean_points(seed)
    x[POISONED_CHAIN, 1:] = value, 1.0
    return x


def with_lds(cases):
    """every case in device memory, and again in LDS where its arrays fit"""
    out = []
    for c in cases:
        out.append(c)
        if c.doubles <= LDS_DOUBLES:
            out.append(Case(**{**{f: getattr(c, f) for f in ("name", "call", "p0", "p1", "p2", "n_out", "oracle", "poison", "matrix", "X")}, "mem": "lds"}))
    return out


# --------------------------------------------------------------------------- scan
def scan_lengths(W):
    S = 64 * W   # a segment; four segments run side by side; the two sets of wave totals alternate per group of four
    return sorted({1, 2, 63, 64, 65, S - 1, S, S + 1, 4 * S - 1, 4 * S, 4 * S + 1, 8 * S + 1, 2000, 20000, 100003})


def coefficients(rng, kind, n):
    if kind == "tanh":
        return np.tanh(rng.normal(size=n))
    if kind == "sprinkled":     # exact 0 (a reset: what came before must not show) and +-1 among ordinary values
        a = np.tanh(rng.normal(size=n))
        pick = rng.uniform(size=n)
        a[pick < 0.06] = 0.0
        a[(pick >= 0.06) & (pick < 0.10)] = 1.0
        a[(pick >= 0.10) & (pick < 0.14)] = -1.0
        return a
    if kind == "negative":
        return -rng.uniform(0.2, 0.999, size=n)
    assert kind == "above_one"  # short rows only: 1.3 ** 65 is still a small number
    return rng.uniform(1.0, 1.3, size=n) * rng.choice([-1.0, 1.0], size=n)


def scan_cases(W):
    """The thinning rule.  Every length of ``scan_lengths`` runs all six (a kind) x (forward, reversed).  What rotates, with the length's
    position in the list and the case: the rows (1, 3, 8; several rows only up to R T = 8200), the init kind (constant, scalar, per row;
    the reversed routine has none) and the coefficient set (tanh of normals, sprinkled 0 / +-1, negative, |a| above 1 up to T = 65).
    Three rows of 8 * 64 W + 1 elements are added by name (four cases).  Each case runs in device memory, and in LDS when its arrays fit."""
    import oracle

    rng = np.random.default_rng(100 + W)
    cases = []
    sets = ["tanh", "sprinkled", "negative", "above_one"]
    def add(R, T, ak, rev, init_kind, cs):
        a = coefficients(rng, cs, R * T).reshape(R, T) if ak == "A_ARRAY" else np.zeros(0)
        a_s = {"A_SCALAR": float(coefficients(rng, cs, 1)[0]), "A_ARRAY": 1.0, "A_ONE": 1.0}[ak]
        b = rng.normal(size=(R, T))
        b[rng.uniform(size=(R, T)) < 0.02] = -0.0      # (a negative zero: the identity composition is not a no-op on it)
        init = rng.normal(size={"row": R, "scalar": 1, "const": 0}[init_kind])     # (a scalar init is scaled with the chain like the rows')
        i_expr = {"const": _f(0.25), "scalar": "(double)P2[0]", "row": "0.0"}[init_kind]
        call = (f"nphip_scan::linear_recurrence<{R}, {T}, nphip_scan::{ak}, {'true' if rev else 'false'}, {'true' if init_kind == 'row' else 'false'}>"
                f"(P0, {_f(a_s)}, P1, P2, {i_expr}, PO, lane);")

        def run(p0, p1, p2):
            aa = p0 if ak == "A_ARRAY" else (1 if ak == "A_ONE" else a_s)
            ii = {"const": 0.25, "scalar": float(p2[0]) if p2.size else 0.0, "row": p2}[init_kind]
            return oracle.chain_scan(p1, aa, ii, waves=W, rev=rev)

        cases.append(Case(f"scan R={R} T={T} {ak} rev={rev} init={init_kind} a={cs}", call, a, b, init, R * T, run, poison=((R * T) // 2, 1)))

    for idx, T in enumerate(scan_lengths(W)):
        for j, (ak, rev) in enumerate([(ak, rev) for ak in ("A_ARRAY", "A_SCALAR", "A_ONE") for rev in (False, True)]):
            R = [1, 3, 8][(idx + j) % 3]
            if R * T > 8200:
                R = 1
            init_kind = "const" if rev else ["const", "scalar", "row"][(idx + 2 * j) % 3]
            cs = sets[(idx + j) % 4]
            if cs == "above_one" and T > 65:
                cs = "tanh"
            add(R, T, ak, rev, init_kind, cs)
    # named, not left to the rotation: several rows of more than two groups of four segments each — the carry starts again and the set of
    # wave totals in use carries over at every change of row
    for ak, rev, init_kind in (("A_ARRAY", False, "row"), ("A_ARRAY", True, "const"), ("A_ONE", False, "scalar"), ("A_SCALAR", True, "const")):
        add(3, 8 * 64 * W + 1, ak, rev, init_kind, "sprinkled")
    return with_lds(cases)


# --------------------------------------------------------------------------- data-matrix products
def matvec_shapes(W):
    """The thinning rule.  Every K of the list gets two R in rotation through (1, 2, 3, 4, 15, 16) — so that every R meets a small, a
    boundary and a large K — plus R = 16 at K = 9 and at K = 256 W + 1; the instantiation <K, R> runs with three n
    of the list in rotation (n is a run-time argument), dropping an n where n K > 1 300 000 (the matrix and its copy are data) or
    n R > 40 000 (the output of 64 chains is read back).  Both routines for every (n, K, R), in device memory, and in LDS where the
    operands fit."""
    S = 64 * W
    Ns = sorted({1, 63, 64, 65, 4 * S - 1, 4 * S, 4 * S + 1, 2000, 20000})
    Ks = sorted({1, 7, 8, 9, 63, 64, 65, S - 1, S, S + 1, 200, 4 * S, 4 * S + 1, 600})
    Rs = [1, 2, 3, 4, 15, 16]
    pairs = [(K, Rs[(j + W + h) % 6]) for j, K in enumerate(Ks) for h in (0, 3)]
    pairs += [kr for kr in [(9, 16), (4 * S + 1, 16)] if kr not in pairs]
    shapes = []
    for j, (K, R) in enumerate(pairs):
        for m in range(3):
            n = Ns[(j + 3 * m) % len(Ns)]
            if n * K <= 1_300_000 and n * R <= 40_000:
                shapes.append((n, K, R))
    # the longest matrix and the widest one with the most rows the caps allow are named, not left to the rotation
    for extra in [(20000, 64, 1), (2000, 600, min(R for K, R in pairs if K == 600))]:
        if extra not in shapes:
            shapes.append(extra)
    return shapes


def matvec_cases(W):
    import oracle

    rng = np.random.default_rng(200 + W)
    pool = rng.normal(size=1_300_000)
    pool[rng.uniform(size=pool.size) < 0.01] = 0.0
    pool[[0, 2]] = 0.0      # (every matrix is the head of the pool: with one row, the outputs of columns 0 and 2 are sums of signed zeros
    #                          only — an accumulator that does not start from +0.0 gives -0.0 there)
    cases = []
    none = np.zeros(0)
    for n, K, R in matvec_shapes(W):
        X = pool[:n * K].reshape(n, K)
        B, G = rng.normal(size=(K, R)), rng.normal(size=(n, R))
        cases.append(Case(f"times n={n} K={K} R={R}", f"nphip_mv::times<{K}, {R}>(MX, P1, PO, n, lane);", none, B, none, n * R,
                          lambda p0, p1, p2, X=X: oracle.chain_times(X, p1), poison=(K // 2, R), matrix="Xt", X=X))
        cases.append(Case(f"times_t n={n} K={K} R={R}", f"nphip_mv::times_t<{K}, {R}>(MX, P1, PO, n, lane);", none, G, none, K * R,
                          lambda p0, p1, p2, X=X: oracle.chain_times_t(X, p1), poison=(n // 2, R), matrix="X", X=X))
    return with_lds(cases)


# --------------------------------------------------------------------------- Cholesky and substitutions
LINALG_K = [1, 2, 3, 4, 5, 8, 15, 16, 17, 31, 32]
LINALG_N = [1, 2, 63, 64, 65, 85, 128, 129]


def spd(rng, K, cond=None):
    if cond is None:
        M = rng.normal(size=(K, K + 3))
        return M @ M.T / K + 0.5 * np.eye(K)
    Q, _ = np.linalg.qr(rng.normal(size=(K, K)))
    A = (Q * np.logspace(0, -np.log10(cond), K)) @ Q.T
    return (A + A.T) / 2


def linalg_cases():
    """The thinning rule.  ``cholesky`` and ``cholesky_adj`` run at every K with a random SPD matrix and one of condition 1e12 (the same
    instantiation, other data); the three routines with right-hand sides run at every K with three N of the list in rotation — every N
    meets a K <= 5 and a K >= 17 —, ``solve_lower_t`` in both of its layouts.  Device memory, and LDS where the arrays fit."""
    import oracle

    rng = np.random.default_rng(300)
    cases = []
    none = np.zeros(0)
    for j, K in enumerate(LINALG_K):
        for cond in (None, 1e12):
            A = spd(rng, K, cond)
            L = oracle.chain_cholesky(A)[0]
            assert np.isfinite(L).all()
            tag = f"K={K} cond={cond or 'random'}"
            cases.append(Case(f"cholesky {tag}", f"nphip_la::cholesky<{K}>(P1, PO, lane);", none, A, none, K * K,
                              lambda p0, p1, p2: oracle.chain_cholesky(p1)[0], poison=((K // 2) * (K + 1), 1)))
            Lbar = rng.normal(size=(K, K))      # not symmetric, and with an upper triangle that must not count
            cases.append(Case(f"cholesky_adj {tag}", f"nphip_la::cholesky_adj<{K}>(P0, P1, PO, lane);", L, Lbar, none, K * K,
                              lambda p0, p1, p2: oracle.chain_cholesky_adj(p0, p1)))
        if K in (5, 17):     # a diagonal matrix: the poisoned pivot is the value itself, so a subnormal positive one factors
            cases.append(Case(f"cholesky diagonal K={K}", f"nphip_la::cholesky<{K}>(P1, PO, lane);", none, np.diag(rng.uniform(0.5, 2.0, K)), none, K * K,
                              lambda p0, p1, p2: oracle.chain_cholesky(p1)[0], poison=((K // 2) * (K + 1), 1)))
        for m in (0, 3, 5):
            N = LINALG_N[(j + m) % len(LINALG_N)]
            L = oracle.chain_cholesky(spd(rng, K, 1e12 if m == 3 else None))[0]
            B, G2 = rng.normal(size=(K, N)), rng.normal(size=(K, N))
            tag = f"K={K} N={N}"
            cases.append(Case(f"solve_lower {tag}", f"nphip_la::solve_lower<{K}, {N}>(P0, P1, PO, lane);", L, B, none, K * N,
                              lambda p0, p1, p2: oracle.chain_solve_lower(p0, p1)))
            cases.append(Case(f"solve_lower_t columns {tag}", f"nphip_la::solve_lower_t<{K}, {N}, {N}, 1>(P0, P1, PO, lane);", L, B, none, K * N,
                              lambda p0, p1, p2: oracle.chain_solve_lower_t(p0, p1)))
            cases.append(Case(f"solve_lower_t rows {tag}", f"nphip_la::solve_lower_t<{K}, {N}, 1, {K}>(P0, P1, PO, lane);", L, np.ascontiguousarray(B.T), none, K * N,
                              lambda p0, p1, p2: oracle.chain_solve_lower_t(p0, p1, by_rows=True)))
            cases.append(Case(f"solve_lower_adj_l {tag}", f"nphip_la::solve_lower_adj_l<{K}, {N}>(P1, P2, PO, lane);", none, B, G2, K * K,
                              lambda p0, p1, p2: oracle.chain_solve_lower_adj_l(p1, p2)))
    return with_lds(cases)


# --------------------------------------------------------------------------- the probes
@functools.lru_cache(maxsize=None)
def probe(family: str, W: int) -> Probe:
    if family == "scan":
        return Probe(f"scan W={W}", W, ["chain_scan.h"], scan_cases(W))
    if family == "matvec":
        return Probe(f"matvec W={W}", W, ["chain_matvec.h"], matvec_cases(W))
    assert family == "linalg" and W == 1
    return Probe("linalg", 1, ["chain_linalg.h"], linalg_cases())


PROBES = [("scan", 1), ("scan", 2), ("scan", 4), ("matvec", 1), ("matvec", 2), ("matvec", 4), ("linalg", 1)]


# --------------------------------------------------------------------------- the forward scan through the expand step
EXPAND_T = 300


def expand_probe():
    """A standard normal in EXPAND_T dimensions whose expand step (``nphip_expand``: a separate instantiation of the routine, launched by
    the engine over the stored draws) reports x and the recurrence x_t' = a_t x_{t-1}' + x_t with the data coefficients a."""
    from nutpie_amd import from_density_source

    T = EXPAND_T
    a = coefficients(np.random.default_rng(400), "sprinkled", T)
    src = f"""
#include "chain_scan.h"
__device__ double nphip_density(const NphipData& data, int dim, const double* x, double* grad, double* lds, const double* shared, int lane) {{
    double acc = 0.0;
    for (int i = lane; i < dim; i += NPHIP_CHAIN_THREADS) {{
        acc = __builtin_fma(x[i], x[i], acc);
        grad[i] = -x[i];
    }}
    return -0.5 * nphip_chain_sum(acc);
}}
__device__ double nphip_expand(const NphipData& data, int dim, const double* x, double* out, double* lds, const double* shared, int lane) {{
    const auto A = NPHIP_LDS_PTR(double, lds), B = A + {T}, X = B + {T};
    for (int i = lane; i < {T}; i += NPHIP_CHAIN_THREADS) {{
        A[i] = data.a[i];
        B[i] = x[i];
        out[i] = x[i];
    }}
    nphip_chain_barrier();
    nphip_scan::linear_recurrence<1, {T}, nphip_scan::A_ARRAY, false, false>(A, 1.0, B, (const double*)nullptr, 0.5, X, lane);
    for (int i = lane; i < {T}; i += NPHIP_CHAIN_THREADS) out[{T} + i] = X[i];
    return 0.0;
}}
"""
    model = from_density_source(T, src, {"a": a}, expanded_names=["x", "path"], expanded_shapes=[(T,), (T,)], expand_lds_doubles=3 * T)
    return model, a
