"""Probe models for the wave-wide loops that ``nutpie_amd.symbolic`` generates (``_Gen.loop``, ``seg_cap``, ``unroll``), and the table
of shapes and index layouts they are compiled at.  Plain data and fixed seeds; of the code under test only ``nutpie_amd.symbolic`` is
imported.  The high-precision restatement of every variant is tests/loop_edge_reference.py.

One hierarchical regression, small enough to restate by hand:

    mu, b ~ N(0, 1);  sg = exp(sg_log__), sig = exp(sig_log__), each with the density exp(-v^2 / 2) / sqrt(2 pi) and its Jacobian
    a[group] ~ N(0, 1)
    y[obs] ~ N(eta, sig),   eta = mu + b x + (a sg)[gi]  (+ the variant's terms)

Variants (what each adds to ``eta``, each new vector with a N(0, 1) prior; every model reports ``eff = a sg + mu`` on ``group``):

    base     nothing
    crossed  c[hi]: a second index of ``obs`` into ``group`` — the loop over ``group`` holds two segment dictionaries
    three    a2[gi] x + a3[gi] w: three segment sums share gi's ranges — the batch is capped at 64 // 3 = 21
    zs       zs[gi], zs a zero-sum vector on ``group`` (one free value fewer than elements: partial parameter reads)
    p2d      B[pi], B a parameter on product(group, k), k = 2, pi = 2 gi + i % 2; ``Bt = B sg`` is reported with its axes turned
             (a ``perm`` output of the generated expand)

Data magnitudes lie in [0.5, 1.5] with random signs, position magnitudes in [0.3, 0.9]: no element is negligible.  Every y[i] is drawn
again until its residual is at least 2e-3 at each of the case's positions (tests/test_loop_edges_cpu.py holds 1e-3 against the
reference), so that dropping or doubling one observation moves the outputs far beyond their rounding bounds.

The table (``cases(W)``, T = 64 W).  The full cross product of 12 lengths of ``obs``, 9 (5 for W = 2, 4) of ``group`` and 7 range profiles is
thinned to the rows of ``ROWS``: row k takes the k-th length of ``obs``; the lengths of ``group`` cycle through {1, T - 1, T, T + 1, 4T + 1}
and the profiles through (a) ... (f), each moved to the nearest row where profile and lengths are compatible (one observation per group
needs equal lengths, a longest range of L needs obs <= L groups, different caps per slot need more than T groups ...); W = 1 has four
more rows for the lengths of ``group`` that only it keeps (2, 2T + 1, 3T + 1, 4T).  tests/test_loop_edges_cpu.py pins that every length
and every profile occurs at every W, and what the generated sources of the table contain.
"""
import functools

import numpy as np

from nutpie_amd import symbolic as S

VARIANTS = ("base", "crossed", "three", "zs", "p2d")
WAVES = (1, 2, 4)
N_POS = 5          # a full workgroup of four one-wave chains and a ragged one
K2 = 2             # columns of the two-dimensional parameter

OBS_CLASSES = ("1", "2", "T-1", "T", "T+1", "2*T", "2*T+1", "3*T+1", "4*T-1", "4*T", "4*T+1", "8*T+1")
GROUP_CLASSES = {1: ("1", "2", "T-1", "T", "T+1", "2*T+1", "3*T+1", "4*T", "4*T+1"), 2: ("1", "T-1", "T", "T+1", "4*T+1"), 4: ("1", "T-1", "T", "T+1", "4*T+1")}
PROFILES = ("a", "b", "c2", "c3", "d", "e", "f")

# (variant, obs, group, profile, shuffled)
ROWS = (
    ("base", "1", "1", "b", False),
    ("base", "2", "T-1", "a", True),
    ("zs", "T-1", "T-1", "b", True),
    ("base", "T", "T", "c2", True),
    ("base", "T+1", "1", "a", False),
    ("three", "2*T", "T+1", "d", False),
    ("base", "2*T+1", "4*T+1", "d", True),
    ("crossed", "3*T+1", "4*T+1", "e", False),
    ("base", "4*T-1", "4*T+1", "c3", False),
    ("p2d", "4*T", "T-1", "f", False),
    ("base", "4*T+1", "T", "f", True),
    ("base", "8*T+1", "4*T+1", "e", True),
)
ROWS_W1 = (
    ("zs", "2*T+1", "2*T+1", "b", False),
    ("crossed", "2", "2", "b", False),
    ("three", "3*T+1", "3*T+1", "c3", True),
    ("p2d", "4*T+1", "4*T", "f", False),
)


def _size(text: str, T: int) -> int:
    return int(eval(text, {"__builtins__": {}}, {"T": T}))      # (the size classes above: arithmetic in T)


def mag(rng, n, lo=0.5, hi=1.5):
    return rng.uniform(lo, hi, n) * rng.choice([-1.0, 1.0], n)


# --------------------------------------------------------------------------- range profiles
def _spread(counts, free, n, cap):
    """n further observations over the groups ``free``, at most ``cap`` in each, one at a time round the groups"""
    assert n <= cap * len(free), (n, cap, len(free))
    k = 0
    while n > 0:
        g = free[k % len(free)]
        if counts[g] < cap:
            counts[g] += 1
            n -= 1
        k += 1


def profile_counts(profile: str, N: int, G: int, T: int, three: bool = False) -> np.ndarray:
    """observations per group (the lengths of the index's ranges)"""
    counts = np.zeros(G, dtype=np.int64)
    every = list(range(G))
    if profile == "a":        # every observation in one group; the first and last groups empty (where there are three)
        counts[G // 2] = N
    elif profile == "b":      # exactly one observation per group
        assert N == G
        counts[:] = 1
    elif profile in ("c2", "c3"):   # the longest range 2, and 3: either side of the threshold of the capped batch
        L = int(profile[1])
        assert N >= L
        counts[G // 3] = L
        _spread(counts, [g for g in every if g != G // 3], N - L, L - 1 if N - L <= (L - 1) * (G - 1) else L)
    elif profile == "d":      # ranges either side of the cap: 31, 32, 33 (three accumulators: 20, 21, 22)
        lens = (20, 21, 22) if three else (31, 32, 33)
        at = (1, G // 2, G - 2)
        assert G >= 5 and len(set(at)) == 3
        for g, n in zip(at, lens):
            counts[g] = n
        _spread(counts, [g for g in every if g not in at], N - sum(lens), 2)
    elif profile == "e":      # the only long range in a group of the loop's last unrolled slot: the slots get different caps
        U = max(1, min(4, -(-G // T)))
        assert U >= 2
        g = min(G, U * T) - 1
        assert (g % (T * U)) // T == U - 1
        counts[g] = 10
        _spread(counts, [h for h in every if h != g], N - 10, 2)
    elif profile == "f":      # a run of empty groups in the middle, a range of 40 straight after it
        lo, hi = G // 3, G // 3 + max(2, G // 8)
        counts[hi] = 40
        free = [g for g in every if not lo <= g <= hi]
        _spread(counts, free, N - 40, -(-(N - 40) // len(free)))
    else:
        raise ValueError(profile)
    assert counts.sum() == N
    return counts


def index_from_counts(counts, shuffled: bool, rng) -> np.ndarray:
    gi = np.repeat(np.arange(counts.size), counts)
    return rng.permutation(gi) if shuffled else gi


# --------------------------------------------------------------------------- the model
def n_dim(variant: str, G: int) -> int:
    return 4 + G + {"base": 0, "crossed": G, "three": 2 * G, "zs": G - 1, "p2d": K2 * G}[variant]


def eta_numpy(variant, pos, data, G):
    """the linear predictor in plain numpy: what the data generator needs to keep the residuals away from 0 (not a reference)"""
    mu, b, sg = pos[:, 0:1], pos[:, 1:2], np.exp(pos[:, 2:3])
    a = pos[:, 4:4 + G]
    gi, x = data["gi"], data["x"]
    eta = mu + b * x + (a * sg)[:, gi]
    rest = pos[:, 4 + G:]
    if variant == "crossed":
        eta = eta + rest[:, data["hi"]]
    elif variant == "three":
        eta = eta + rest[:, :G][:, gi] * x + rest[:, G:][:, gi] * data["w"]
    elif variant == "zs":
        n = G
        s = rest.sum(axis=1, keepdims=True)
        v = np.concatenate([rest - s * (1.0 / (np.sqrt(n) + n)), -s * (1.0 / np.sqrt(n))], axis=1)
        eta = eta + v[:, gi]
    elif variant == "p2d":
        eta = eta + rest[:, data["pi"]]
    return eta


def make_data(variant: str, gi: np.ndarray, G: int, seed: int, pos: np.ndarray) -> dict:
    """the data of one case for the index ``gi``; y keeps every residual at least 2e-3 away from 0 at the positions ``pos``"""
    rng = np.random.default_rng(seed)
    N = gi.size
    data = {"x": mag(rng, N), "gi": gi.astype(np.int32)}
    if variant == "crossed":
        data["hi"] = rng.integers(0, G, N).astype(np.int32)
    if variant == "three":
        data["w"] = mag(rng, N)
    if variant == "p2d":
        data["pi"] = (K2 * gi + np.arange(N) % K2).astype(np.int32)
    eta = eta_numpy(variant, pos, data, G)
    y = mag(rng, N)
    for _ in range(100):
        bad = (np.abs(y[None, :] - eta) < 2e-3).any(axis=0)
        if not bad.any():
            break
        y[bad] = mag(rng, int(bad.sum()))
    else:
        raise AssertionError("no y keeps the residuals away from 0")
    data["y"] = y
    return data


def positions(variant: str, G: int, seed: int, n: int = N_POS) -> np.ndarray:
    return mag(np.random.default_rng(seed), n * n_dim(variant, G), 0.3, 0.9).reshape(n, -1)


def build(variant: str, G: int, data: dict) -> S.Model:
    m = S.Model()
    m.dim("group", G)
    mu = m.param("mu")
    b = m.param("b")
    sg = m.param("sg", lower=0.0)
    sig = m.param("sig", lower=0.0)
    a = m.param("a", dim="group")
    x = m.data("x", data["x"], dim="obs")
    y = m.data("y", data["y"], dim="obs")
    gi = m.index("gi", data["gi"], dim="obs", into="group")
    for v in (mu, b, sg, sig):
        m.add_logp(S.normal_lpdf(v, 0.0, 1.0))
    m.add_logp(S.normal_lpdf(a, 0.0, 1.0).sum())
    eta = mu + b * x + (a * sg)[gi]
    if variant == "crossed":
        c = m.param("c", dim="group")
        hi = m.index("hi", data["hi"], dim="obs", into="group")
        m.add_logp(S.normal_lpdf(c, 0.0, 1.0).sum())
        eta = eta + c[hi]
    elif variant == "three":
        a2 = m.param("a2", dim="group")
        a3 = m.param("a3", dim="group")
        w = m.data("w", data["w"], dim="obs")
        m.add_logp(S.normal_lpdf(a2, 0.0, 1.0).sum())
        m.add_logp(S.normal_lpdf(a3, 0.0, 1.0).sum())
        eta = eta + a2[gi] * x + a3[gi] * w
    elif variant == "zs":
        zs = m.param("zs", dim="group", zero_sum=True)
        m.add_logp(S.normal_lpdf(zs, 0.0, 1.0).sum())
        eta = eta + zs[gi]
    elif variant == "p2d":
        m.dim("k", K2)
        B = m.param("B", dims=("group", "k"))
        pi = m.index("pi", data["pi"], dim="obs", into="group_x_k")
        m.add_logp(S.normal_lpdf(B, 0.0, 1.0).sum())
        m.deterministic("Bt", B * sg, dims=("k", "group"))
        eta = eta + B[pi]
    elif variant != "base":
        raise ValueError(variant)
    m.add_logp(S.normal_lpdf(y, eta, sig).sum())
    m.deterministic("eff", a * sg + mu)
    return m


# --------------------------------------------------------------------------- the case table
class Case:
    """One compiled shape: ``front`` is the Model, ``compile(**kw)`` its compiled form (cached per keyword set)."""

    def __init__(self, variant, W, N, G, profile, shuffled, seed, obs_class="", group_class=""):
        self.variant, self.W, self.N, self.G, self.profile, self.shuffled, self.seed = variant, W, N, G, profile, shuffled, seed
        self.obs_class, self.group_class = obs_class, group_class
        self.T = 64 * W
        rng = np.random.default_rng(seed)
        self.counts = profile_counts(profile, N, G, self.T, three=variant == "three")
        self.pos = positions(variant, G, seed + 1)
        self.data = make_data(variant, index_from_counts(self.counts, shuffled, rng), G, seed + 2, self.pos)
        self.name = f"{variant} W={W} obs={N} group={G} {profile}{' shuffled' if shuffled else ''}"
        self._compiled = {}

    @property
    def front(self):
        return build(self.variant, self.G, self.data)

    def compile(self, **kw):
        key = tuple(sorted(kw.items()))
        if key not in self._compiled:
            self._compiled[key] = self.front.compile(waves_per_chain=self.W, **kw)
        return self._compiled[key]

    def updates(self):
        """what ``with_data`` takes to put this case's data into a model of the same variant and number of groups"""
        return {k: v for k, v in self.data.items()}

    def __repr__(self):
        return self.name


@functools.lru_cache(maxsize=None)
def cases(W: int) -> tuple:
    T = 64 * W
    out = []
    for k, (variant, o, g, profile, shuffled) in enumerate(ROWS + (ROWS_W1 if W == 1 else ())):
        out.append(Case(variant, W, _size(o, T), _size(g, T), profile, shuffled, seed=1000 * W + 10 * k, obs_class=o, group_class=g))
    return tuple(out)


def case(W: int, variant: str, obs_class: str, profile: str) -> Case:
    return next(c for c in cases(W) if (c.variant, c.obs_class, c.profile) == (variant, obs_class, profile))


# ---- with_data on the specialised form at unchanged lengths: the caps stay those of the data the model was compiled with
def _given(like: "Case", counts, shuffled, seed, name) -> "Case":
    """a case of ``like``'s variant, lengths and positions with other ranges"""
    c = Case.__new__(Case)
    c.__dict__.update(like.__dict__)
    c.counts, c.shuffled, c.seed, c.profile = counts, shuffled, seed, name
    c.data = make_data(like.variant, index_from_counts(counts, shuffled, np.random.default_rng(seed)), like.G, seed + 2, like.pos)
    c.name = f"{like.variant} W={like.W} obs={like.N} group={like.G} {name}"
    c._compiled = {}
    return c


@functools.lru_cache(maxsize=None)
def swap_cases(W: int) -> tuple:
    """[(compiled-with, given)], both rows of the table: the (c, longest 3) row given (f) — ranges beyond every cap of the source, which
    the rest loop has to take —, and the (d) row given one observation per group with the other groups empty — caps of 31 and 32 over
    ranges of 1 and 0, where every read past a range's end is dropped by a select."""
    T = 64 * W
    c3 = case(W, "base", "4*T-1", "c3")
    d = case(W, "base", "2*T+1", "d")
    f = _given(c3, profile_counts("f", c3.N, c3.G, T), False, 1000 * W + 510, "f")
    counts = np.zeros(d.G, dtype=np.int64)
    counts[np.random.default_rng(1000 * W + 520).permutation(d.G)[:d.N]] = 1
    sparse = _given(d, counts, True, 1000 * W + 520, "b with empty groups")
    return ((c3, f), (d, sparse))


# ---- one specialize=False library per W and variant takes every length of obs and every profile through with_data
SWEEP_PROFILES = ("a", "c2", "c3", "c2", "b", "d", "e", "f", "a", "f", "f", "f")      # per length of obs, with T + 1 groups


@functools.lru_cache(maxsize=None)
def sweep(W: int, variant: str) -> tuple:
    """(the case the unspecialised library is compiled with, the cases it is then given): T + 1 groups throughout (a parameter's
    dimension is fixed), every length of ``obs`` with a profile that fits it, sorted and shuffled in turn.  The library is compiled with
    the longest data: ``with_data`` refuses data that outgrow the LDS plan of the data a model was compiled with."""
    T = 64 * W
    G = T + 1
    given = tuple(Case(variant, W, _size(o, T), G, profile, bool(k % 2), seed=2000 * W + 10 * k + VARIANTS.index(variant), obs_class=o)
                  for k, (o, profile) in enumerate(zip(OBS_CLASSES, SWEEP_PROFILES)))
    return given[-1], given


# ---- the smallest model that spills an adjoint array to device memory (data.scratch__) with four chains per workgroup
# (tests/test_loop_edges_cpu.py pins that one observation fewer does not spill)
SPILL_N, SPILL_G = 4097, 7


@functools.lru_cache(maxsize=None)
def spill_case(N: int = SPILL_N) -> Case:
    return Case("base", 1, N, SPILL_G, "f", True, seed=4242)


def spilled_doubles(compiled) -> int:
    s = compiled._scratch
    return int(s(compiled._data) if callable(s) else s)
