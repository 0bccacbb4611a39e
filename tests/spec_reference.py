"""The edge table of the numerics contract (include/nphip_spec.h) and its exact reference — TEST INFRASTRUCTURE.

``CASES[name]`` is the argument table of one function, ``[n, n_in]`` float64 in the record layout of ``nphip_test_spec`` (include/nutpie_hip.h;
integers travel as doubles).  It is plain data, built with numpy from fixed seeds: importing this module does not import ``mpmath``.
:func:`reference` evaluates a table in ``mpmath`` at 50 digits on the float64 arguments taken as exact; it runs once, in
tests/golden/make_spec_reference.py, and the tests read ``tests/golden/spec_reference.npz``.  The points are the places where such functions go wrong
(each builder below says which), a few thousand per function at the most.

What the fixture holds per table ``t``: ``t.x`` (the arguments; tables of 32-bit words as uint32) and the reference —
  exp, log, log1p, logaddexp, div, sqrt, u01, normal_pair: ``t.ref``, the correctly rounded float64 of the exact value (subnormals, 0 and inf included;
      NaN where the contract says NaN).  ``exp`` beyond its cut-offs, ``log`` of 0 / negatives / inf follow the contract's special cases, which are
      also the correctly rounded values.  normal_pair: ``[n, 3]`` = z0, z1 and the radius sqrt(-2 ln u1), with u1, u2 the float64 values ``u01`` gives.
  sincos2pi: ``t.ref`` ``[n, 2]`` and ``t.lo`` (float32): sin, cos as double-double pairs, exact - ref to 24 more bits.
  exp_parts: e^x = (``t.ref`` + ``t.lo``) * 2^``t.e`` with ``t.ref`` in [1, 2).
  philox: the four output words (Random123's known answers, and a from-the-paper Python restatement for the rest: :func:`philox`).
  weights: see :func:`weight_sequences`.

The fixture is capped by the largest file already in tests/golden (about 190 kB), and a float64 of full entropy costs 7 bytes compressed.  That is why each
reduction boundary of ``exp`` gets one point within 1e-15 relative and one within 1e-3 absolute, on opposite sides, the sides alternating with k — and
not both sides of both at every k —, why those points and the weight sequences are float32-valued numbers, why the binade points of ``log1p`` below 2^-60 have 8-bit mantissas, and why one of a merge's two uniforms is a multiple of 2^-9.
"""
from __future__ import annotations

import ctypes
import functools
import math
import os
import subprocess

import numpy as np

from oracle import SPEC_FNS

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
FIXTURE = os.path.join(GOLDEN, "spec_reference.npz")
DPS = 50

INF, NAN = math.inf, math.nan
DBL_MAX, DBL_MIN, DENORM_MIN = 1.7976931348623157e308, 2.2250738585072014e-308, 5e-324
EXP_HI, EXP_LO = 709.782712893384, -745.2            # the cut-offs of nphip_exp
LN2 = 0.6931471805599453
SWITCH = float.fromhex("0x1.6a09e667f3bcdp+0")       # the sqrt(2) switch of nphip_log
# fn -> (n_in, n_out) and fn -> code: the record table of nphip_test_spec, as the oracle's front-end restates it
SHAPES = {fn: (n_in, n_out) for fn, (_, n_in, n_out) in SPEC_FNS.items()}
SPEC_CODES = {fn: code for fn, (code, _, _) in SPEC_FNS.items()}


def _next(x, steps=1):
    x = np.float64(x)
    for _ in range(abs(steps)):
        x = np.nextafter(x, np.float64(INF if steps > 0 else -INF))
    return float(x)


def _around(x):
    return [_next(x, -1), float(x), _next(x, 1)]


def _cat(*parts):
    return np.concatenate([np.atleast_1d(np.asarray(p, dtype=np.float64)).ravel() for p in parts])


# ---- the tables --------------------------------------------------------------------------------------------------------------------------------------------


def _exp_table():
    rng = np.random.default_rng(101)
    k = np.arange(-1074, 1025, dtype=np.float64)
    b = (k + 0.5) * LN2                                   # the reduction boundaries: |r| is largest beside them
    side = np.where(k.astype(np.int64) % 2 == 0, 1.0, -1.0)
    near = b * (1.0 + side * 1e-15)                       # a few ulp from the boundary, on either side of it
    off = (b - side * rng.uniform(2e-4, 8e-4, k.size)).astype(np.float32).astype(np.float64)   # within 1e-3, on the other side (float32-valued: see the docstring)
    # x * (1 / ln2) an exact half-integer: the argument of rint is a tie (to even: down for even j, up for odd j)
    inv = float.fromhex("0x1.71547652b82fep+0")
    ties = []
    for j in list(range(-1075, 1024, 9)) + [-3, -2, -1, 0, 1, 2]:
        x0 = (j + 0.5) / inv
        for c in [x0] + [_next(x0, s) for s in (-3, -2, -1, 1, 2, 3)]:
            if c * inv == j + 0.5:
                ties.append(c)
                break
    sub = rng.uniform(-745.2, -708.39, 400)              # subnormal results: the second scaling step rounds
    small = _cat(rng.uniform(-1e-8, 1e-8, 60), [s * 10.0 ** -e for e in range(9, 20) for s in (1, -1)])
    edges = _cat([0.0, -0.0, 1e-300, -1e-300], _around(EXP_HI), _around(EXP_LO), [-745.13, -745.14, -745.1332191019412], [709.0, 710.0, -746.0, 1e9, -1e9, 1e300, -1e300],
                 [NAN, INF, -INF])
    return _cat(near, off, ties, sub, small, edges)


def _log_table():
    rng = np.random.default_rng(102)
    one = _cat([1 - 2.0 ** -53, 1 + 2.0 ** -52, 1 - 2.0 ** -52, 1.0], 1 + np.arange(-16, 17) * 2.0 ** -40, 1 + rng.integers(-2 ** 20, 2 ** 20, 31) * 2.0 ** -40)
    window = rng.uniform(1 - 1e-3, 1 + 1e-3, 200)
    e = np.array(sorted(set(range(-1074, 1024, 13)) | {-1074, -1073, -1023, -1022, -1021, -2, -1, 0, 1, 1022, 1023}))
    m = np.concatenate([SWITCH * (1 + 1e-12) * np.ones(e.size), SWITCH * (1 - 1e-12) * np.ones(e.size)])
    binades = np.ldexp(m, np.concatenate([e, e]).astype(np.int32))   # (subnormal results lose mantissa bits: they are still arguments)
    binades = binades[np.isfinite(binades) & (binades > 0)]
    cancel = rng.uniform(0.69, 0.72, 400)                 # e = -1 cancels against log m; the worst case known, 0x1.644e12f22e5f1p-1, lies here
    edges = _cat(_around(SWITCH), _around(SWITCH / 2), [float.fromhex("0x1.644e12f22e5f1p-1")], [DENORM_MIN, 1e-310, DBL_MIN, _next(DBL_MIN, -1), DBL_MAX, 2.0, 0.5, 1e-300, 1e300],
                 [0.0, -0.0, -1.0, -DENORM_MIN, -INF, INF, NAN])
    wide = np.exp(rng.uniform(-740, 709, 100))
    return _cat(one, window, binades, cancel, edges, wide)


def _log1p_table():
    rng = np.random.default_rng(103)
    e = np.arange(-1074, 0)
    # 2^e [1, 2): below 2^-53 the u == 1 branch returns y whatever the mantissa (multiples of 2^-8 there: see the docstring), above it every bit counts
    mant = np.where(e < -60, 1 + rng.integers(0, 256, e.size) / 256.0, 1 + rng.uniform(0, 1, e.size))
    binades = np.ldexp(mant, e.astype(np.int32))
    edges = _cat(_around(2.0 ** -53), [2.0 ** -52, _next(2.0 ** -52, 1), 2.0 ** -54, 1.0, _next(1.0, -1), 0.0, DENORM_MIN, DBL_MIN, 0.5, 1e-8, 1e-16, 1.5e-16])
    return _cat(rng.uniform(0, 1, 300), binades, edges)


def _sincos_table():
    rng = np.random.default_rng(104)
    oct_ = [v for j in range(8) for v in (j / 8 - 2.0 ** -54, j / 8, j / 8 + 2.0 ** -54) if v >= 0]     # (below 1/2 the +- 2^-54 are distinct doubles; above, ties)
    near = [v for j in range(1, 8) for v in _around(j / 8)] + [v for j in range(8) for v in _around(j / 8 + 1 / 16)]   # f beside 0 / 1 and beside the swap at 1/2
    return _cat(rng.uniform(0, 1, 300), oct_, near, [_next(1.0, -1), 2.0 ** -54, DENORM_MIN, 1e-300, 2.0 ** -53, 1 / 3, 0.1])


QUARTERS = {0.0: (0.0, 1.0), 0.25: (1.0, 0.0), 0.5: (0.0, -1.0), 0.75: (-1.0, 0.0)}     # the exact values (tests/test_spec.py)


def _logaddexp_table():
    rng = np.random.default_rng(105)
    a = rng.uniform(-50, 50, 200)
    pairs = [np.stack([a, a + rng.uniform(-800, 800, 200)], 1)]
    a2 = rng.uniform(-50, 50, 66)
    d = 2.0 ** np.arange(-60, 6)
    pairs += [np.stack([a2, a2 + d], 1), np.stack([a2, a2 - d], 1)]
    a3 = rng.uniform(-0.75, -0.6, 30)                     # the sum near 0: a and the log1p term cancel, the error is large in ulp of the result
    pairs += [np.stack([a3, a3 + rng.uniform(-0.2, 0.2, 30)], 1)]
    pairs += [np.array([[1.5, 1.5], [0.0, 0.0], [-700.0, -700.0], [1e300, 1e300], [-INF, 2.0], [0.0, -INF], [-INF, -INF], [INF, 1.0], [1.0, INF], [INF, INF],
                        [NAN, 1.0], [1.0, NAN], [NAN, NAN], [0.0, -745.0], [0.0, -746.0], [3.0, 3.0 + 2.0 ** -51], [-0.0, 0.0]])]
    return np.concatenate(pairs)


def _exp_parts_table():
    rng = np.random.default_rng(106)
    x = _cat(rng.uniform(-1e9, 1e9, 120), rng.uniform(-1e4, 1e4, 80), rng.uniform(-2, 2, 60), [1e9, -1e9, _next(1e9, -1), _next(-1e9, 1), 0.0, -0.0, 0.5 * LN2, -0.5 * LN2],
             (np.arange(-40, 41, 8) * 2.0 ** 24 + 0.5) * LN2)
    return x


def _div_table():
    rng = np.random.default_rng(107)
    n = 100
    sub = lambda: rng.integers(1, 2 ** 52, n).astype(np.float64) * DENORM_MIN      # noqa: E731
    norm = lambda lo, hi: np.exp(rng.uniform(lo, hi, n)) * rng.choice([-1.0, 1.0], n)   # noqa: E731
    b1 = norm(-30, 30)
    q = sub()
    b3 = norm(-300, 300)
    rows = [np.stack([sub(), b1], 1), np.stack([norm(-30, 30), sub()], 1), np.stack([q * b3, b3], 1),                       # subnormal a; subnormal b; subnormal a / b
            np.stack([DBL_MAX * rng.uniform(0.5, 1.0, n) * (b4 := rng.uniform(1e-3, 1.0, n)), b4], 1),                      # quotients near DBL_MAX (some overflow)
            np.stack([norm(-700, 700), norm(-700, 700)], 1), np.stack([np.ones(n), norm(-600, 600)], 1),
            np.array([[DENORM_MIN, 2.0], [3 * DENORM_MIN, 2.0], [DBL_MIN, 2.0], [DBL_MAX, 0.5], [DBL_MAX, 1 - 2.0 ** -53], [1.0, 3.0], [2.0, 3.0], [1.0, DENORM_MIN], [DENORM_MIN, DENORM_MIN],
                      [0.0, 1.0], [-0.0, 1.0], [1.0, INF], [1.0, 0.0], [-1.0, 0.0], [0.0, 0.0], [INF, INF], [NAN, 1.0], [DBL_MIN, DBL_MAX], [1.0, -INF]])]
    return np.concatenate(rows)


def _sqrt_table():
    rng = np.random.default_rng(108)
    return _cat(rng.integers(1, 2 ** 52, 40).astype(np.float64) * DENORM_MIN, [DENORM_MIN, 2 * DENORM_MIN, 3 * DENORM_MIN, DBL_MIN, _next(DBL_MIN, -1), DBL_MAX, _next(DBL_MAX, -1)],
                np.exp(rng.uniform(-700, 700, 60)), [0.0, -0.0, 1.0, 2.0, 4.0, _next(1.0, -1), _next(1.0, 1), INF, -1.0, NAN])


def philox(seed, c0, c1, c2, c3):
    """Philox4x32-10 written from the paper (Salmon et al., SC'11) in Python integers: a third statement of it, beside the header's and the oracle's."""
    k0, k1 = seed & 0xFFFFFFFF, seed >> 32
    c = [c0, c1, c2, c3]
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c[0], 0xCD9E8D57 * c[2]
        c = [(p1 >> 32) ^ c[1] ^ k0, p1 & 0xFFFFFFFF, (p0 >> 32) ^ c[3] ^ k1, p0 & 0xFFFFFFFF]
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return tuple(c)


# Random123's kat_vectors for philox4x32-10: (seed, counter words) -> output words (the three of tests/test_spec.py)
PHILOX_KAT = [((0, 0, 0, 0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
              ((0xFFFFFFFFFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF), (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
              ((0x299F31D0A4093822, 0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1))]


def _philox_inputs():
    rng = np.random.default_rng(109)
    rows = [k for k, _ in PHILOX_KAT] + [(int(rng.integers(0, 2 ** 63)) * 2 + int(rng.integers(0, 2)), *(int(v) for v in rng.integers(0, 2 ** 32, 4))) for _ in range(40)]
    rows += [(7, j, 3, 5, 1) for j in range(200)]        # a momentum stream (c0 = pair index, c1 = chain, c2 = draw, c3 = purpose): the blocks of the normal_pair table
    return rows


def _philox_table():
    return np.array([[s & 0xFFFFFFFF, s >> 32, c0, c1, c2, c3] for s, c0, c1, c2, c3 in _philox_inputs()], dtype=np.float64)


def _words_of_k(k):
    """(hi, lo) whose top 53 bits are k."""
    x = k << 11
    return x >> 32, x & 0xFFFFFFFF


_K_TOP = 2 ** 53 - 1
# k of u01 = (k + 0.5) 2^-53: the smallest and the largest, the last k whose k + 0.5 is a float64 (2^52 - 1) and the first that rounds to even
_U01_K = [0, 1, 2, _K_TOP, _K_TOP - 1, _K_TOP - 2, 2 ** 52 - 1, 2 ** 52, 2 ** 52 + 1, 2 ** 52 + 2, 2 ** 51, 12345678901234]


def _u01_table():
    rng = np.random.default_rng(110)
    rows = [_words_of_k(k) for k in _U01_K] + [(0, 0x7FF), (0, 0x800), (0xFFFFFFFF, 0xFFFFF7FF)] + [tuple(int(v) for v in rng.integers(0, 2 ** 32, 2)) for _ in range(40)]
    return np.array(rows, dtype=np.float64)


def _normal_pair_table():
    rows = []
    mid = _words_of_k(2 ** 52 // 3)
    # u1 the smallest, the largest (k = 2^53 - 1 rounds to 1.0: the radius is 0), mid-range; u2 mid-octant
    for k1 in (0, 1, _K_TOP, _K_TOP - 1, _K_TOP - 3, 2 ** 52, 2 ** 52 // 3, 2 ** 40):
        rows.append((*_words_of_k(k1), *_words_of_k(2 ** 53 // 16 + 5)))
    # u2 at and beside each octant boundary j / 8 (k + 0.5 = j 2^50: the boundary lies between k = j 2^50 - 1 and j 2^50; from 1/2 on, ties to even land on it)
    for j in range(0, 8):
        for dk in (-2, -1, 0, 1):
            k2 = j * 2 ** 50 + dk
            if 0 <= k2 <= _K_TOP:
                rows.append((*mid, *_words_of_k(k2)))
    rows.append((*mid, *_words_of_k(_K_TOP - 1)))          # the largest u2 inside [0, 1)
    rows += [philox(*inp) for inp in _philox_inputs()[-200:]]
    return np.array(rows, dtype=np.float64)


# u2 = 1.0 (k = 2^53 - 1, probability 2^-53 per draw) is outside the domain of nphip_sincos2pi: what the contract gives there is pinned by the tests, not bounded
NORMAL_PAIR_U2_ONE = np.array([[*_words_of_k(2 ** 52 // 3), *_words_of_k(_K_TOP)]], dtype=np.float64)


# ---- tree weights ------------------------------------------------------------------------------------------------------------------------------------------

WEIGHT_LENGTHS, WEIGHT_SCALES = (2, 8, 64, 1024), (0.5, 30.0, 3000.0)


def weight_sequences():
    """``[(name, x[n])]``: -energy_error of the leaves of a sequence, in merge order — float32-valued, drawn as scale * normal; then the clamps at +-1e9."""
    rng = np.random.default_rng(111)
    out = [("n%d_s%g" % (n, s), (s * rng.normal(size=n)).astype(np.float32).astype(np.float64)) for s in WEIGHT_SCALES for n in WEIGHT_LENGTHS]
    out.append(("clamp", np.array([2e9, 1e9, INF, -2e9, 1e9 - 64, -INF, 1e9 - 512], dtype=np.float64)))
    return out


def weight_offsets():
    """name -> (first, end) of a sequence's leaves in the concatenated ``weights.x``."""
    o, out = 0, {}
    for name, x in weight_sequences():
        out[name] = (o, o + len(x))
        o += len(x)
    return out


def _weights_table():
    return np.concatenate([x for _, x in weight_sequences()])


def _w_rel_table():
    """(m, e, E): pairs whose exponents differ by 998 .. 1001 (d = 999 is kept, d = 1000 dropped) and nearer ones."""
    rng = np.random.default_rng(112)
    rows = []
    for d in (0, 1, 2, 52, 53, 54, 500, 997, 998, 999, 1000, 1001, 1002, 2000, 10 ** 6, 2 * 10 ** 9):
        for e in (0, -1074, 1024, -(10 ** 9), 10 ** 9 - d if d < 10 ** 9 else -(10 ** 9)):
            rows.append((float(rng.uniform(0.70, 1.42)), e, e + d))
    rows += [(1.0, 0, 999), (1.0, 0, 1000), (1.4142135623730951, -5, 994), (1.4142135623730951, -5, 995), (700.0, 3, 1002), (700.0, 3, 1003)]
    return np.array(rows, dtype=np.float64)


def _w_add_table():
    """(m1, e1, m2, e2), both orders of the pairs of the w_rel table and sums of sums (mantissas up to 2n)."""
    rng = np.random.default_rng(113)
    rows = []
    for m, e, E in _w_rel_table():
        m2 = float(rng.uniform(0.70, 1.42)) * float(rng.choice([1.0, 8.0, 1000.0]))
        rows += [(m, e, m2, E), (m2, E, m, e)]
    return np.array(rows, dtype=np.float64)


_BUILDERS = {"exp": _exp_table, "log": _log_table, "log1p": _log1p_table, "sincos2pi": _sincos_table, "logaddexp": _logaddexp_table, "exp_parts": _exp_parts_table,
             "div": _div_table, "sqrt": _sqrt_table, "philox": _philox_table, "u01": _u01_table, "normal_pair": _normal_pair_table, "weights": _weights_table,
             "w_rel": _w_rel_table, "w_add": _w_add_table}
CASES = {name: np.ascontiguousarray(build(), dtype=np.float64) for name, build in _BUILDERS.items()}
TABLES = list(CASES)


# ---- the reference (mpmath; never at import) ---------------------------------------------------------------------------------------------------------------


def _exact(mp, v):
    """The float64 ``v`` (finite) as an mpf, exactly."""
    m, e = math.frexp(float(v))
    return mp.mpf(int(m * 2 ** 53)) * mp.mpf(2) ** (e - 53)


def _round(mp, v):
    """The correctly rounded float64 of the mpf ``v``, subnormals included (through an exact fraction: one rounding), inf on overflow."""
    from fractions import Fraction

    if v == 0:
        return 0.0
    sign, man, exp, _ = v._mpf_
    fr = Fraction(man) * (Fraction(2) ** exp)
    try:
        out = float(fr)          # int / int true division: correctly rounded, gradual underflow
    except OverflowError:
        out = INF
    return -out if sign else out


def _dd(mp, v):
    hi = _round(mp, v)
    return hi, float(np.float32(float(v - _exact(mp, hi)))) if math.isfinite(hi) else 0.0


def _mant(mp, v):
    """v > 0 as (hi, lo, e): v = (hi + lo) 2^e, hi in [1, 2) a float64, lo a float32."""
    e = int(mp.floor(mp.log(v, 2)))
    m = v / mp.mpf(2) ** e
    if m >= 2:
        m, e = m / 2, e + 1
    if m < 1:
        m, e = m * 2, e - 1
    hi, lo = _dd(mp, m)
    return hi, lo, e


def _clamp(x):
    return min(max(x, -1e9), 1e9)


def reference(name, rows=None):
    """The reference of table ``name`` (of the rows ``rows`` of it: an index array) as a dict of arrays, in mpmath at :data:`DPS` digits."""
    import mpmath as mp

    x = CASES[name] if rows is None else CASES[name][np.asarray(rows)]
    x = x.reshape(len(x), -1)
    with mp.workdps(DPS):
        f = lambda v: _exact(mp, v)    # noqa: E731
        if name == "exp":
            def one(v):
                if v != v:
                    return NAN
                if v == INF or v > 1e6:
                    return INF
                if v == -INF or v < -1e6:
                    return 0.0
                return _round(mp, mp.exp(f(v)))
            return {"ref": np.array([one(v) for v in x[:, 0]])}
        if name == "log":
            def one(v):
                if v != v or v < 0:
                    return NAN
                if v == 0:
                    return -INF
                return INF if v == INF else _round(mp, mp.log(f(v)))
            return {"ref": np.array([one(v) for v in x[:, 0]])}
        if name == "log1p":
            return {"ref": np.array([_round(mp, mp.log1p(f(v))) for v in x[:, 0]])}
        if name == "sqrt":
            return {"ref": np.array([NAN if (v != v or v < 0) else (v if v in (0.0, INF) else _round(mp, mp.sqrt(f(v)))) for v in x[:, 0]])}
        if name == "div":
            from fractions import Fraction

            def one(a, b):
                if a != a or b != b or (a == 0 and b == 0) or (abs(a) == INF and abs(b) == INF):
                    return NAN
                neg = (math.copysign(1, a) < 0) != (math.copysign(1, b) < 0)
                if b == 0 or abs(a) == INF:
                    return -INF if neg else INF
                if abs(b) == INF or a == 0:
                    return -0.0 if neg else 0.0
                try:
                    return float(Fraction(a) / Fraction(b))      # exact quotient, one rounding
                except OverflowError:
                    return -INF if neg else INF
            return {"ref": np.array([one(float(a), float(b)) for a, b in x])}
        if name == "sincos2pi":
            ref, lo = [], []
            for v in x[:, 0]:
                if float(v) in QUARTERS:
                    s, c = (mp.mpf(t) for t in QUARTERS[float(v)])
                else:
                    ang = 2 * mp.pi * f(v)
                    s, c = mp.sin(ang), mp.cos(ang)
                (sh, sl), (ch, cl) = _dd(mp, s), _dd(mp, c)
                ref.append((sh, ch))
                lo.append((sl, cl))
            return {"ref": np.array(ref), "lo": np.array(lo, dtype=np.float32)}
        if name == "logaddexp":
            def one(a, b):
                if a != a or b != b:
                    return NAN
                if a == INF or b == INF:
                    return INF
                if a == -INF:
                    return b
                if b == -INF:
                    return a
                hi, lo = max(a, b), min(a, b)
                return _round(mp, f(hi) + mp.log1p(mp.exp(f(lo) - f(hi))))
            return {"ref": np.array([one(float(a), float(b)) for a, b in x])}
        if name == "exp_parts":
            out = [_mant(mp, mp.exp(f(v))) for v in x[:, 0]]
            return {"ref": np.array([o[0] for o in out]), "lo": np.array([o[1] for o in out], dtype=np.float32), "e": np.array([o[2] for o in out], dtype=np.int64)}
        if name == "philox":
            kat = {k: v for k, v in PHILOX_KAT}
            ref = []
            for r in x:
                key = (int(r[0]) | (int(r[1]) << 32), *(int(v) for v in r[2:]))
                ref.append(kat.get(key) or philox(*key))
            return {"ref": np.array(ref, dtype=np.uint32)}
        if name == "u01":
            def one(hi, lo):
                k = ((int(hi) << 32) | int(lo)) >> 11
                return _round(mp, (mp.mpf(k) + mp.mpf("0.5")) * mp.mpf(2) ** -53)
            return {"ref": np.array([one(hi, lo) for hi, lo in x])}
        if name == "normal_pair":
            return reference_normal_pair(rows)
        if name == "w_rel":
            # the contract: m 2^(e - E), exact, for E - e < 1000; 0 from there on
            return {"ref": np.array([0.0 if E - e >= 1000 else _round(mp, f(m) * mp.mpf(2) ** int(e - E)) for m, e, E in x])}
        if name == "w_add":
            def one(m1, e1, m2, e2):
                E = max(e1, e2)
                t = [mp.mpf(0) if E - e >= 1000 else f(m) * mp.mpf(2) ** int(e - E) for m, e in ((m1, e1), (m2, e2))]
                return _round(mp, t[0] + t[1]), E
            out = [one(*r) for r in x]
            return {"ref": np.array([o[0] for o in out]), "e": np.array([o[1] for o in out], dtype=np.int64)}
    raise KeyError(name)


def u01_value(hi, lo):
    """u01 as the contract defines it, in Python's float arithmetic (one rounding of k + 0.5, exact scaling)."""
    return ((((int(hi) << 32) | int(lo)) >> 11) + 0.5) * 2.0 ** -53


def reference_normal_pair(rows=None):
    """normal_pair on the float64 uniforms ``u01`` gives: ``[n, 3]`` = z0, z1, sqrt(-2 ln u1), correctly rounded."""
    import mpmath as mp

    x = CASES["normal_pair"] if rows is None else CASES["normal_pair"][np.asarray(rows)]
    ref = []
    with mp.workdps(DPS):
        for w in x:
            u1, u2 = _exact(mp, u01_value(w[0], w[1])), _exact(mp, u01_value(w[2], w[3]))
            rad = mp.sqrt(-2 * mp.log(u1))
            ref.append((_round(mp, rad * mp.cos(2 * mp.pi * u2)), _round(mp, rad * mp.sin(2 * mp.pi * u2)), _round(mp, rad)))
    return {"ref": np.array(ref)}


def reference_weights(names=None):
    """Per sequence: the exact sum of exp(clamped x_i) after the prefixes in ``checkpoints(n)`` as (hi, lo, e), and per merge step i >= 1 the exact
    probability P_i = exp(x_i) / sum_{j <= i} exp(x_j) that the merge takes the new leaf — as two uniforms (``u[:, 0]`` a multiple of 2^-9 drawn at random,
    ``u[:, 1]`` a float64 at c n 2^-51 from P_i, c in [2, 32], where that lies inside (0, 1), else random), the exact decisions ``u < P_i`` and ``keep``: whether
    |u - P_i| > n 2^-51 (n the sequence's length), the rule under which the computed decision must equal the exact one."""
    import mpmath as mp

    rng = np.random.default_rng(114)
    out = {}
    with mp.workdps(DPS):
        for name, xs in weight_sequences():
            n = len(xs)
            # (random numbers are drawn for every sequence, so that a subset reproduces the fixture's)
            u0 = (rng.integers(0, 512, n) + 0.5) / 512.0
            c = rng.uniform(2, 32, n) * rng.choice([-1.0, 1.0], n)
            alt = rng.uniform(0, 1, n)
            if names is not None and name not in names:
                continue
            terms = [mp.exp(_exact(mp, _clamp(float(v)))) for v in xs]
            tot, sums, u, dec, keep = mp.mpf(0), [], np.zeros((n, 2)), np.zeros((n, 2), dtype=bool), np.zeros((n, 2), dtype=bool)
            cps = checkpoints(n)
            tol = mp.mpf(n) * mp.mpf(2) ** -51
            for i, t in enumerate(terms):
                tot += t
                if i + 1 in cps:
                    sums.append(_mant(mp, tot))
                if i == 0:
                    continue
                P = t / tot
                u1 = float(P) + c[i] * n * 2.0 ** -51
                u[i] = (u0[i] if i else 0.0), (u1 if 0.0 < u1 < 1.0 else alt[i])
                for j in range(2):
                    uj = _exact(mp, u[i, j])
                    dec[i, j] = bool(uj < P)
                    keep[i, j] = bool(abs(uj - P) > tol)
            out[name] = {"sum_hi": np.array([s[0] for s in sums]), "sum_lo": np.array([s[1] for s in sums], dtype=np.float32),
                         "sum_e": np.array([s[2] for s in sums], dtype=np.int64), "u": u, "decision": dec, "keep": keep}
    return out


def pack_weights(ref):
    """The per-sequence reference of every sequence as the fixture's few concatenated arrays (sequence order; :func:`unpack_weights` undoes it)."""
    cat = lambda k: np.concatenate([ref[name][k] for name, _ in weight_sequences()])    # noqa: E731
    u = cat("u")
    return {"weights.sum_hi": cat("sum_hi"), "weights.sum_lo": cat("sum_lo"), "weights.sum_e": cat("sum_e"), "weights.u0": np.round(u[:, 0] * 512 - 0.5).astype(np.uint16),
            "weights.u1": u[:, 1].copy(), "weights.decision": np.packbits(cat("decision"), axis=None), "weights.keep": np.packbits(cat("keep"), axis=None)}


def unpack_weights(fix):
    """name -> the dict :func:`reference_weights` gives, from the fixture's arrays."""
    n_all = len(CASES["weights"])
    u = np.stack([(fix["weights.u0"].astype(np.float64) + 0.5) / 512.0, fix["weights.u1"]], 1)
    u[np.concatenate([[o] for o, _ in weight_offsets().values()])] = 0.0      # (a sequence's first leaf has no merge)
    dec = np.unpackbits(fix["weights.decision"])[:2 * n_all].reshape(n_all, 2).astype(bool)
    keep = np.unpackbits(fix["weights.keep"])[:2 * n_all].reshape(n_all, 2).astype(bool)
    out, c = {}, 0
    for name, (lo, hi) in weight_offsets().items():
        nc = len(checkpoints(hi - lo))
        out[name] = {"sum_hi": fix["weights.sum_hi"][c:c + nc], "sum_lo": fix["weights.sum_lo"][c:c + nc], "sum_e": fix["weights.sum_e"][c:c + nc],
                     "u": u[lo:hi], "decision": dec[lo:hi], "keep": keep[lo:hi]}
        c += nc
    return out


def checkpoints(n):
    """The prefix lengths of a sequence of n leaves at which the exact sum is stored."""
    return sorted(c for c in {1, 2, 3, n} | {2 ** j for j in range(1, 11)} if c <= n)


# ---- the fixture -------------------------------------------------------------------------------------------------------------------------------------------


def load():
    with np.load(FIXTURE) as z:
        return {k: z[k] for k in z.files}


def args_of(fix, name):
    """The argument table ``[n, n_in]`` of ``name`` as the fixture stores it."""
    return np.ascontiguousarray(fix[name + ".x"], dtype=np.float64).reshape(len(CASES[name]), -1)


# ---- the header on the host (tests/fixtures/spec_header.c) -----------------------------------------------------------------------------------------------


@functools.lru_cache(maxsize=None)
def header_lib():
    src, out = os.path.join(HERE, "fixtures", "spec_header.c"), os.path.join(HERE, "fixtures", "libspec_header.so")
    hdr = os.path.join(HERE, "..", "include", "nphip_spec.h")
    if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(src), os.path.getmtime(hdr)):
        subprocess.run(["gcc", "-O2", "-fPIC", "-shared", "-ffp-contract=off", "-o", out, src, "-lm"], check=True)
    so = ctypes.CDLL(out)
    so.spec_header.argtypes = [ctypes.c_int, ctypes.c_uint64, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
    return so


def header(fn, x):
    """include/nphip_spec.h's ``fn`` as gcc compiles it, on the rows of ``x[n, n_in]``: ``y[n, n_out]``."""
    n_in, n_out = SHAPES[fn]
    x = np.ascontiguousarray(x, dtype=np.float64).reshape(-1, n_in)
    y = np.empty((x.shape[0], n_out))
    rc = header_lib().spec_header(SPEC_CODES[fn], x.shape[0], n_in, x.ctypes.data, n_out, y.ctypes.data)
    assert rc == 0, (fn, rc)
    return y


def run_sequence(call, xs):
    """A weight sequence through ``call(fn, rows)`` (header, oracle or device): leaves by w_leaf, merged left to right by w_add.  Returns
    (leaf[n, 2], total[n, 2], add_in[n - 1, 4]): the leaves' (m, e), the running total after each leaf, and the w_add records that produced it."""
    leaf = call("w_leaf", xs)
    tot, rec = [leaf[0]], []
    for i in range(1, len(xs)):
        r = np.array([tot[-1][0], tot[-1][1], leaf[i][0], leaf[i][1]])
        rec.append(r)
        tot.append(call("w_add", r[None])[0])
    return leaf, np.array(tot), np.array(rec).reshape(-1, 4)


# ---- comparing ---------------------------------------------------------------------------------------------------------------------------------------------


def same_bits(a, b):
    """Element-wise: the same float64 bits (so -0.0 != 0.0), or both NaN."""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return (a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))


def _ordinal(a):
    """float64 -> int64 ordered like the reals (-0.0 and 0.0 both 0; inf one step past DBL_MAX)."""
    b = np.ascontiguousarray(a, dtype=np.float64).view(np.int64)
    return np.where(b < 0, np.int64(-2 ** 63) - b, b)


def ulp_distance(got, ref):
    """How many float64 steps ``got`` is from the correctly rounded ``ref`` (NaN against NaN: 0; NaN against a number: inf)."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    og, orf = _ordinal(got), _ordinal(ref)
    same = (og >= 0) == (orf >= 0)          # (the difference of two ordinals of one sign fits int64 exactly; across zero a float64 is exact enough)
    d = np.where(same, np.abs(np.where(same, og - orf, 0)).astype(np.float64), np.abs(og.astype(np.float64) - orf.astype(np.float64)))
    nan_g, nan_r = np.isnan(got), np.isnan(ref)
    return np.where(nan_g & nan_r, 0.0, np.where(nan_g | nan_r, INF, d))


# ---- every record the three implementations are compared on --------------------------------------------------------------------------------------------------

SPECIALS = np.array([NAN, INF, -INF, 1e9, -1e9, 710.0, -746.0, 0.0, -0.0, 1e300, -1e300, DENORM_MIN])


def specials(fn):
    """What the other half of a wave holds in the per-lane test: the specials inside the domain of ``fn``.  Outside it the contract converts a NaN or an
    out-of-range float64 to an integer, which C leaves undefined and x86-64 and gfx950 answer differently: nphip_w_leaf never sees a NaN (a leaf whose
    energy error is not finite has diverged) and nphip_sincos2pi only [0, 1]."""
    if fn == "sincos2pi":
        return np.array([0.0, 0.125, 0.25, 0.375, 0.5, 0.625, 0.75, 0.875, 1.0, 1.0 - 2.0 ** -53, 2.0 ** -54, DENORM_MIN])
    return SPECIALS[1:] if fn == "w_leaf" else SPECIALS


@functools.lru_cache(maxsize=None)
def records():
    """fn -> the argument rows ``[n, n_in]`` at which header, oracle and device are compared: the fixture's tables, the same table through the other
    entry of a function (``exp_scale``, ``exp_scale_select`` and ``w_leaf`` on arguments of ``exp``), and the records of the weight sequences as the
    header computes them (``w_add`` and ``accept`` inputs: the running totals are the header's, which the CPU tests hold to the fixture)."""
    fix = load()
    t = {name: args_of(fix, name) for name in TABLES}
    w = unpack_weights(fix)
    adds, accepts = [t["w_add"]], []
    for name, (lo, hi) in weight_offsets().items():
        _, _, rec = run_sequence(header, t["weights"][lo:hi, 0])
        adds.append(rec)
        for j in range(2):
            accepts.append(np.concatenate([w[name]["u"][1:, j:j + 1], rec], 1))
    exp_x = np.concatenate([t["exp"][:, 0], [5e8, -5e8, 2e9, -2e9]])
    return {"exp": t["exp"], "log": t["log"], "log1p": t["log1p"], "sincos2pi": np.concatenate([t["sincos2pi"], [[1.0]]]), "sqrt": t["sqrt"], "div": t["div"],
            "logaddexp": t["logaddexp"], "exp_parts": t["exp_parts"], "exp_scale": exp_x[:, None], "exp_scale_select": exp_x[:, None],
            "w_leaf": np.concatenate([t["weights"][:, 0], exp_x[~np.isnan(exp_x)], t["exp_parts"][:, 0]])[:, None], "w_rel": t["w_rel"], "w_add": np.concatenate(adds),
            "accept": np.concatenate(accepts), "normal_pair": np.concatenate([t["normal_pair"], NORMAL_PAIR_U2_ONE]), "philox": t["philox"], "u01": t["u01"]}
