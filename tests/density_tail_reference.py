"""The element-wise functions and the densities of the front end (nutpie_amd/symbolic.py) restated by hand in mpmath at 60 digits, at
arguments far in the tails, with the rounding bound that a double-precision evaluation has to keep there.

Nothing of the code under test is used: no ``evaluate``, no ``gradient``, no ``Expr``.  mpmath is needed only to compute a reference
(``function_rows``, ``density_rows``: the generator tests/golden/make_density_tail_reference.py and the CPU test that recomputes thinned
rows); the tables, the counts and the checks import without it, so the GPU tests read the fixture alone.

A. The function table.  ``FUNCTIONS[name]`` lists at most 64 arguments (one wave's width) at the edges where an implementation switches
method or the result leaves the double range.  For each argument the fixture holds f, f', x f' and x f'' (f and f' as a double and the
rest that the double misses: ``hi + lo``).  A value is held in units of 2^-53 (|f| + |x f'|), a derivative in units of
2^-53 (|f'| + |x f''|): what the rounding of the argument alone costs, plus the result's own.  sigmoid' and tanh' are floored at 1:
the rules n (1 - n) and 1 - n^2 are absolute by design.  An exact value below 2^-1022 gets an additive 2^-1074.  Where the exact value
exceeds the double range the expected result is that infinity, exactly.

B. The densities.  ``DENSITIES[name]``: the textbook formula of ONE observation's addend as a function of its arguments ``a`` (data
values first, then the constrained parameter values), three observations as data columns, the kind of every parameter ("real":
theta = q, "pos": theta = exp(q), the log-Jacobian q added to logp), the grid of unconstrained positions, and the count c.

C. The bound.  With s_i = max(1, |f_i| + sum_k |a_k df_i/da_k|) per addend, the value scale is sum_i s_i + sum |q_j| over the
positive parameters (their log-Jacobians).  For the gradient element j, h_ij = (dtheta_j/dq_j) df_i/dtheta_j and the scale is
sum_i max(1, |h_ij| + sum_k |a_k dh_ij/da_k|) + 1.  The floor of 1 says that an absolute error of 2^-53 per addend cannot matter to a
trajectory; the Jacobian's own contribution to a gradient is exactly 1.  An output passes when err <= (N - 1 + c) 2^-53 scale, N = 3
addends; the gradient gets 2 c.  The bound excuses conditioning in the density's own arguments (an argument off by one rounding moves
the exact value that much); it does not excuse cancellation inside the formula.  The partials are mpmath's (``mp.diff``: central
differences at raised precision), Laplace's — not differentiable where y = mu — by hand.

c is written out per density below, from the textbook formula: the number of arithmetic operations plus, for each elementary function,
its allowance A_f; a positive parameter adds A_exp + 1 (theta = exp(q), and the addition of q).

D. The allowance.  ``HOST_WORST[f]``: the worst error, in the units of A, of the host's double-precision library (numpy; scipy.special
for erf, erfc, lgamma, digamma; the composed softplus and sigmoid; the derivative rules of the front end evaluated with numpy) on the
function table — measured by tests/test_density_tails_cpu.py, recorded in profiles/density_tails.txt.
A_f = max(4, 4 x the host's worst, rounded up to an integer).  An argument at which the host returns no finite value for a finite exact
one (``HOST_FAILS``) is not a measurement of rounding and is left out; the device is held to A_f there all the same.
"""
import itertools
import math
import os

import numpy as np

try:
    import mpmath as mp
except ImportError:      # the tables and the checks are still there
    mp = None

DPS = 60
U = 2.0 ** -53
TINY = 2.0 ** -1074
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "density_tail_reference.npz")


def _around(v):
    v = float(v)
    return [float(np.nextafter(v, -np.inf)), v, float(np.nextafter(v, np.inf))]


def _pm(vs):
    return [s * float(v) for v in vs for s in (1.0, -1.0)]


_PI = math.pi
_ROOT_LGAMMA = -2.4570247382208006
_ROOT_DIGAMMA = 1.4616321449683623

#: the points the table is built around (a test asserts that every one is among the function's arguments)
EDGES = {
    "exp": [5e-324, -5e-324, 0.35, -0.35, 709.782712893384, float(np.nextafter(709.782712893384, np.inf)), -745.1332191019411, -745.1332191019412, -37.0],
    "expm1": [5e-324, -5e-324, 0.35, -0.35, 709.782712893384, float(np.nextafter(709.782712893384, np.inf)), -745.1332191019411, -37.0],
    "log": _around(1.0) + _around(math.sqrt(2.0)) + [5e-324, 1e300, 1.0 - 2.0 ** -53],
    "log1p": _around(0.0) + _around(math.sqrt(2.0) - 1.0) + [1e300, -1.0 + 2.0 ** -53],
    "softplus": [0.0, 18.0, -18.0, 37.0, -37.0, 709.0, -709.0, -745.0],
    "sigmoid": [0.0, 18.0, -18.0, 37.0, -37.0, 709.0, -709.0, -745.0],
    "tanh": [5e-324, 0.55, 19.06, 22.0],
    "erf": [5e-324, 0.84375, 1.25, 1.0 / 0.35, 6.0],
    "erfc": [5e-324, 0.84375, 1.25, 1.0 / 0.35, 6.0, 26.54, -6.0],
    "sin": [k * _PI / 2 for k in range(1, 5)] + [1e5, 1e22, 2.0 ** 1000],
    "cos": [k * _PI / 2 for k in range(1, 5)] + [1e5, 1e22, 2.0 ** 1000],
    "atan": [5e-324, 7 / 16, 11 / 16, 19 / 16, 39 / 16, 2.0 ** 66],
    "lgamma": [5e-324, 1e-8, 0.5] + _around(1.0) + _around(2.0) + [2.5, 8.0, 1e5, 1e305, -0.5, -2.5] + _around(_ROOT_LGAMMA),
    "digamma": [1e-300, 1e-8, 0.5, 1.0, _ROOT_DIGAMMA, float(np.nextafter(_ROOT_DIGAMMA, 2.0)), 1.5, 2.0, 9.999999, 10.0, 10.5, 30.0, 1e3, 1e8, 1e300,
                -0.5, -1.0 + 1e-10, -1e-10, -2.5, -1000000.25],
}

_EXP_MORE = _pm([1e-300, 2.0 ** -54, 1e-10, 0.34657359027997264, 1.0, 88.0]) + _around(0.35) + _around(-0.35) + [709.0, 710.0, 1000.0, -708.3964185322641,
                                                                                                               -745.0, -746.0, -1000.0, -36.7, -37.5]
FUNCTIONS = {
    "exp": EDGES["exp"] + _EXP_MORE,
    "expm1": EDGES["expm1"] + _EXP_MORE + [-745.1332191019412],
    "log": EDGES["log"] + _around(1.0 / math.sqrt(2.0)) + [2.2250738585072014e-308, 1e-300, 0.5, 2.0, 10.0, 0.9, 1.1, 1e-5, 1.7976931348623157e308],
    "log1p": EDGES["log1p"] + _around(1.0 / math.sqrt(2.0) - 1.0) + _pm([2.0 ** -53, 1e-300, 1e-10, 0.25]) + [-0.5, 1.0, 1e16, -0.9999, 1.7976931348623157e308],
    "softplus": EDGES["softplus"] + _pm([1e-10, 0.5, 1.0, 5.0, 36.0, 40.0]) + [33.3, 709.78, 745.0],
    "sigmoid": EDGES["sigmoid"] + _pm([1e-10, 0.5, 1.0, 5.0, 36.0, 40.0]) + [33.3, 709.78, 745.0],
    "tanh": EDGES["tanh"] + _around(0.55) + _around(19.061547465398498) + _pm([1e-300, 2.0 ** -28, 1e-5, 1.0, 0.5493061443340549, 22.000001, 40.0, 709.0])
    + [-0.55, -19.06, -22.0, -5e-324],
    "erf": EDGES["erf"] + _around(0.84375) + _around(1.25) + _around(1.0 / 0.35) + _around(6.0) + _pm([1e-300, 2.0 ** -28, 0.5, 1.0, 2.0, 3.0, 5.9, 28.0])
    + [-0.84375, -1.25, -6.0, -5e-324],
    "erfc": EDGES["erfc"] + _around(0.84375) + _around(1.25) + _around(1.0 / 0.35) + _around(6.0) + _around(-6.0) + _around(26.54)
    + _pm([1e-300, 2.0 ** -28, 0.5, 1.0, 2.0, 3.0, 5.9]) + [26.5432, 26.6, 27.2, 27.3, 28.0, -0.84375, -1.25, -5e-324],
    "sin": EDGES["sin"] + _pm([5e-324, 1e-300, 2.0 ** -27, 0.5, 1.0, _PI / 4, 3 * _PI / 4]) + [-k * _PI / 2 for k in range(1, 5)] + [-1e5, -1e22, -2.0 ** 1000]
    + _around(_PI) + [1e10, 1e15, 1.7976931348623157e308],
    "cos": EDGES["cos"] + _pm([5e-324, 1e-300, 2.0 ** -27, 0.5, 1.0, _PI / 4, 3 * _PI / 4]) + [-k * _PI / 2 for k in range(1, 5)] + [-1e5, -1e22, -2.0 ** 1000]
    + _around(_PI / 2) + [1e10, 1e15, 1.7976931348623157e308],
    "atan": EDGES["atan"] + _around(7 / 16) + _around(11 / 16) + _around(19 / 16) + _around(39 / 16) + _pm([1e-300, 2.0 ** -29, 1.0, 1e300])
    + [float(np.nextafter(2.0 ** 66, np.inf)), -7 / 16, -39 / 16, -2.0 ** 66, -5e-324],
    "lgamma": EDGES["lgamma"] + [1e-300, 0.25, 1.5, 3.0, _ROOT_DIGAMMA, 170.5, 171.7, 1e15, 2.0 ** 52, 1e306, 1e10, 13.0, 7.999, 1e-5, -1e-8, -1.5, -3.5, -100.5,
                                 -2.7476826467274127],
    "digamma": EDGES["digamma"] + [5e-324, 0.25, 3.0, 6.0, 9.0, 1e15, 100.0, 1e5, -1.5, -3.5, -100.5, -0.25],
}
FUNCTIONS = {k: list(dict.fromkeys(float(t) for t in v)) for k, v in FUNCTIONS.items()}      # (a point named twice is held once)
assert all(len(v) <= 64 for v in FUNCTIONS.values()), {k: len(v) for k, v in FUNCTIONS.items()}
#: digamma has no derivative rule in the front end: its argument is data and only its value is checked
NO_DERIVATIVE = ("digamma",)
#: derivative rules that are absolute by design: their unit is floored at 1
FLOORED_DERIVATIVE = ("sigmoid", "tanh")

#: worst error of the host's double-precision library on the table, (value, derivative), in the units of A (profiles/density_tails.txt)
HOST_WORST = {
    "exp": (0.516, 0.516), "expm1": (0.467, 0.516), "log": (0.593, 0.5), "log1p": (0.804, 1.0), "softplus": (0.471, 1.083), "sigmoid": (1.083, 1.098),
    "tanh": (0.596, 1.004), "erf": (0.882, 0.457), "erfc": (2.0, 0.457), "sin": (0.294, 0.345), "cos": (0.345, 0.294), "atan": (0.466, 0.612),
    "lgamma": (6.424, 0.655), "digamma": (3.971, 0.0),
}
#: arguments at which the host's library gives no finite value where the exact one is finite (scipy's gammaln overflows on 1 / x at a
#: subnormal x): they say nothing about rounding, are left out of HOST_WORST, and the device is still held to A_f there
HOST_FAILS = {"lgamma": (5e-324,)}
#: expected-limit rows: (function, "value" | "derivative") -> {x: (limit in units: the measured figure rounded up to a power of two, the
#: measured figure, why)} — points outside the regions the densities reach, where the device's library exceeds A_f
LIMITS = {}
A = {f: max(4, int(math.ceil(4.0 * max(w)))) for f, w in HOST_WORST.items()}


# --------------------------------------------------------------------------- mpmath: the functions
def _sech2(x):
    return 1 / mp.cosh(x) ** 2


def _sig(x):
    return 1 / (1 + mp.exp(-x))


def _lgamma(x):
    return mp.re(mp.loggamma(x))


def _mp_functions():
    """name -> (f, f', f'') by hand"""
    c = 2 / mp.sqrt(mp.pi)
    return {
        "exp": (mp.exp, mp.exp, mp.exp),
        "expm1": (mp.expm1, mp.exp, mp.exp),
        "log": (mp.log, lambda x: 1 / x, lambda x: -1 / (x * x)),
        "log1p": (mp.log1p, lambda x: 1 / (1 + x), lambda x: -1 / ((1 + x) * (1 + x))),
        "softplus": (lambda x: x + mp.log1p(mp.exp(-x)) if x > 0 else mp.log1p(mp.exp(x)), _sig, lambda x: _sig(x) * _sig(-x)),
        "sigmoid": (_sig, lambda x: _sig(x) * _sig(-x), lambda x: -_sig(x) * _sig(-x) * mp.tanh(x / 2)),
        "tanh": (mp.tanh, _sech2, lambda x: -2 * mp.tanh(x) * _sech2(x)),
        "erf": (mp.erf, lambda x: c * mp.exp(-x * x), lambda x: -2 * x * c * mp.exp(-x * x)),
        "erfc": (mp.erfc, lambda x: -c * mp.exp(-x * x), lambda x: 2 * x * c * mp.exp(-x * x)),
        "sin": (mp.sin, mp.cos, lambda x: -mp.sin(x)),
        "cos": (mp.cos, lambda x: -mp.sin(x), lambda x: -mp.cos(x)),
        "atan": (mp.atan, lambda x: 1 / (1 + x * x), lambda x: -2 * x / (1 + x * x) ** 2),
        "lgamma": (_lgamma, mp.digamma, lambda x: mp.psi(1, x)),
        "digamma": (mp.digamma, lambda x: mp.psi(1, x), lambda x: mp.psi(2, x)),
    }


COLUMNS = ("x", "f", "f_lo", "d", "d_lo", "xd", "xdd", "fu", "du")


def _dbl(v) -> float:
    """the double nearest to ``v``: an infinity past the double range, one rounding in the subnormal range"""
    if abs(v) >= mp.mpf(2) ** 1024 - mp.mpf(2) ** 970:
        return math.copysign(math.inf, v)
    if abs(v) < mp.mpf(2) ** -1022:
        return float(int(mp.nint(v * mp.mpf(2) ** 1074))) * TINY
    return float(v)


def _split(v):
    hi = _dbl(v)
    return hi, (0.0 if math.isinf(hi) else _dbl(v - mp.mpf(hi)))


def function_rows(name: str, xs=None) -> dict:
    """the table of ``name`` at ``xs`` (default: all its arguments): arrays x, f, f_lo, d, d_lo, xd (= x f'), xdd (= x f''), and the units
    fu = 2^-53 (|f| + |x f'|), du = 2^-53 (|f'| + |x f''|) (formed here: x f' can leave the double range where its unit does not)"""
    xs = FUNCTIONS[name] if xs is None else xs
    out = {k: [] for k in COLUMNS}
    with mp.workdps(DPS):
        f, f1, f2 = _mp_functions()[name]
        for x in xs:
            X = mp.mpf(float(x))
            v, d, dd = f(X), f1(X), f2(X)
            hi, lo = _split(v)
            dhi, dlo = _split(d)
            u = mp.mpf(2) ** -53
            for k, t in zip(out, (float(x), hi, lo, dhi, dlo, _dbl(X * d), _dbl(X * dd), _dbl(u * (abs(v) + abs(X * d))), _dbl(u * (abs(d) + abs(X * dd))))):
                out[k].append(t)
    return {k: np.array(v, dtype=np.float64) for k, v in out.items()}


# --------------------------------------------------------------------------- the checks (numpy only)
def _err(got, hi, lo):
    """|got - (hi + lo)| in double precision: got - hi is exact where the two are close"""
    with np.errstate(all="ignore"):
        return np.abs((np.asarray(got, dtype=np.float64) - hi) - lo)


def ratios(got, hi, lo, unit_u, allowance, underflow=True):
    """err / (allowance unit_u [+ 2^-1074 where the exact value is below 2^-1022]) per element, ``unit_u`` the unit times 2^-53; where the
    exact value is an infinity the result must be that infinity, exactly (ratio 0 or inf); where only the unit is (a slope that left the
    double range) anything but a NaN passes"""
    got, hi, lo, unit = (np.asarray(t, dtype=np.float64) for t in (got, hi, lo, unit_u))
    with np.errstate(all="ignore"):
        bound = allowance * unit + np.where(np.abs(hi) < 2.0 ** -1022, TINY if underflow else 0.0, 0.0)
        r = np.where(bound > 0, _err(got, hi, lo) / bound, np.where(_err(got, hi, lo) == 0, 0.0, np.inf))
    exact = np.isinf(hi)
    r = np.where(exact, np.where(got == hi, 0.0, np.inf), r)
    r = np.where(~exact & np.isinf(unit), np.where(np.isnan(got), np.inf, 0.0), r)
    return np.where(np.isnan(r), np.inf, r)


def function_ratios(name: str, t: dict, value, deriv=None):
    """(value ratios, derivative ratios or None) of a double-precision evaluation of ``name`` on the table ``t``, in units of A_f = 1"""
    with np.errstate(all="ignore"):
        rv = ratios(value, t["f"], t["f_lo"], t["fu"], 1.0)
        if deriv is None:
            return rv, None
        return rv, ratios(deriv, t["d"], t["d_lo"], np.maximum(t["du"], U) if name in FLOORED_DERIVATIVE else t["du"], 1.0)


def table(fix, name: str) -> dict:
    return {k: fix[f"fn_{name}_{k}"] for k in COLUMNS}


# --------------------------------------------------------------------------- the densities
Q9 = (-30.0, -12.0, -3.0, 0.0, 3.0, 8.0, 14.0, 20.0, 25.0)      # scale and shape parameters exp(q)
Q5 = (-12.0, -3.0, 0.0, 3.0, 8.0)                               # where the wider grid overflows
Q4 = (-12.0, -3.0, 0.0, 3.0)                                    # Weibull's shape: exp(alpha (log x - log beta)) overflows from alpha = e^8 on
LOC = (-500.0, -3.0, 0.0, 40.0, 500.0)
LOGIT = (-745.0, -37.0, -3.0, 0.0, 3.0, 37.0, 709.0)
LOG_RATE = (-745.0, -37.0, -3.0, 0.0, 3.0, 37.0, 700.0)         # Poisson's log rate: the logits, but three addends of exp(709) overflow
PHI = (-12.0, -3.0, 0.0, 3.0, 5.0, 7.0, 12.0, 18.0, 25.0, 30.0)
ETA = (-4.0, 0.0, 3.0, 12.0)

#: the data columns: three observations each.  lf = lgamma(cnt + 1) and lb = log C(ntr, cnt) are the doubles scipy gives, taken as exact
#: inputs (the fixture holds them: ``data_columns``)
DATA = {
    "y": (-1.3, 0.2, 40.0),
    "pos": (1e-3, 1.0, 50.0),
    "unit": (1e-9, 0.5, 1.0 - 1e-9),
    "bin": (0.0, 1.0, 1.0),
    "cnt": (0.0, 3.0, 50.0),
    "ntr": (1.0, 7.0, 50.0),
}
N_OBS = 3


def data_columns() -> dict:
    """every data column as float64 (needs scipy for lf and lb: the generator; the tests read them from the fixture)"""
    from scipy.special import gammaln

    d = {k: np.array(v, dtype=np.float64) for k, v in DATA.items()}
    d["lf"] = gammaln(d["cnt"] + 1.0)
    d["lb"] = gammaln(d["ntr"] + 1.0) - gammaln(d["cnt"] + 1.0) - gammaln(d["ntr"] - d["cnt"] + 1.0)
    return d


def _c(ops, functions, n_pos):
    return ops + sum(A[f] for f in functions) + n_pos * (A["exp"] + 1)


def _log_pi():
    return mp.log(mp.pi)


_NU = 3.5     # student_t with nu a number


def _student(y, nu, mu, sigma):
    z = (y - mu) / sigma
    return _lgamma((nu + 1) / 2) - _lgamma(nu / 2) - mp.log(nu * mp.pi) / 2 - mp.log(sigma) - (nu + 1) / 2 * mp.log1p(z * z / nu)


def _laplace_partials(a):
    """f = -log 2 - log b - |y - mu| / b by hand (a = y, mu, b): f, df/da_k, d2f/(dtheta_j da_k) for theta = (mu, b)"""
    y, mu, b = a
    r, s = abs(y - mu), mp.sign(y - mu)
    f = -mp.log(2) - mp.log(b) - r / b
    d1 = [-s / b, s / b, -1 / b + r / (b * b)]
    d2 = [[mp.mpf(0), mp.mpf(0), -s / (b * b)], [s / (b * b), -s / (b * b), 1 / (b * b) - 2 * r / b ** 3]]
    return f, d1, d2


#: name -> data columns (the first arguments of f), parameters (name, kind, grid) in the order of the flat position (the last arguments
#: of f), f, and the count c: operations of the textbook formula + the allowances of its functions (+ A_exp + 1 per positive parameter)
DENSITIES = {
    # -z^2/2 - log sigma - C, z = (y - mu) / sigma: sub div mul mul sub sub
    "normal": dict(data=("y",), params=(("mu", "real", LOC), ("sigma", "pos", Q9)), c=_c(6, ["log"], 1),
                   f=lambda y, mu, s: -((y - mu) / s) ** 2 / 2 - mp.log(s) - mp.log(2 * mp.pi) / 2),
    # -(x/sigma)^2/2 - log sigma + C: div mul mul sub add
    "halfnormal": dict(data=("pos",), params=(("sigma", "pos", Q9),), c=_c(5, ["log"], 1),
                       f=lambda x, s: -(x / s) ** 2 / 2 - mp.log(s) + mp.log(2 / mp.pi) / 2),
    # C(nu) - log sigma - (nu+1)/2 log1p(z^2/nu): sub div mul div mul sub sub, the constant
    "student_t_number": dict(data=("y",), params=(("mu", "real", LOC), ("sigma", "pos", Q9)), c=_c(8, ["log", "log1p"], 1),
                             f=lambda y, mu, s: _student(y, mp.mpf(_NU), mu, s)),
    # nu = a + 1; lgamma((nu+1)/2) - lgamma(nu/2) - log(nu pi)/2 - log sigma - (nu+1)/2 log1p(z^2/nu): 15 operations
    "student_t_expr": dict(data=("y",), params=(("a", "pos", Q9), ("mu", "real", (-3.0,)), ("sigma", "pos", Q9)),
                           c=_c(15, ["lgamma", "lgamma", "log", "log", "log1p"], 2), f=lambda y, a, mu, s: _student(y, a + 1, mu, s)),
    # -log pi - log gamma - log1p(z^2): sub div mul sub sub
    "cauchy": dict(data=("y",), params=(("mu", "real", LOC), ("gamma", "pos", Q9)), c=_c(5, ["log", "log1p"], 1),
                   f=lambda y, mu, g: -_log_pi() - mp.log(g) - mp.log1p(((y - mu) / g) ** 2)),
    "halfcauchy": dict(data=("pos",), params=(("gamma", "pos", Q9),), c=_c(4, ["log", "log1p"], 1),
                       f=lambda x, g: mp.log(2 / mp.pi) - mp.log(g) - mp.log1p((x / g) ** 2)),
    # log r - r x: mul sub
    "exponential": dict(data=("pos",), params=(("rate", "pos", Q9),), c=_c(2, ["log"], 1), f=lambda x, r: mp.log(r) - r * x),
    # -z^2/2 - log sigma - log x - C, z = (log x - mu) / sigma: sub div mul mul sub sub sub; log x enters twice
    "lognormal": dict(data=("pos",), params=(("mu", "real", LOC), ("sigma", "pos", Q9)), c=_c(7, ["log", "log", "log"], 1),
                      f=lambda x, mu, s: -((mp.log(x) - mu) / s) ** 2 / 2 - mp.log(s) - mp.log(x) - mp.log(2 * mp.pi) / 2),
    # alpha log beta - lgamma alpha + (alpha - 1) log x - beta x: mul sub sub mul add mul sub
    "gamma": dict(data=("pos",), params=(("alpha", "pos", Q9), ("beta", "pos", Q9)), c=_c(7, ["log", "lgamma", "log"], 2),
                  f=lambda x, al, be: al * mp.log(be) - _lgamma(al) + (al - 1) * mp.log(x) - be * x),
    # alpha log beta - lgamma alpha - (alpha + 1) log x - beta / x
    "inverse_gamma": dict(data=("pos",), params=(("alpha", "pos", Q9), ("beta", "pos", Q9)), c=_c(7, ["log", "lgamma", "log"], 2),
                          f=lambda x, al, be: al * mp.log(be) - _lgamma(al) - (al + 1) * mp.log(x) - be / x),
    # lgamma(a+b) - lgamma a - lgamma b + (a-1) log x + (b-1) log1p(-x): add sub sub sub mul add sub mul add
    "beta": dict(data=("unit",), params=(("a", "pos", Q9), ("b", "pos", Q9)), c=_c(9, ["lgamma", "lgamma", "lgamma", "log", "log1p"], 2),
                 f=lambda x, a, b: _lgamma(a + b) - _lgamma(a) - _lgamma(b) + (a - 1) * mp.log(x) + (b - 1) * mp.log1p(-x)),
    # -log 2 - log b - |y - mu| / b: sub abs div sub sub
    "laplace": dict(data=("y",), params=(("mu", "real", LOC), ("b", "pos", Q9)), c=_c(5, ["log"], 1), f=None, partials=_laplace_partials),
    # -z - log s - 2 softplus(-z): sub div neg sub mul sub
    "logistic": dict(data=("y",), params=(("mu", "real", LOC), ("s", "pos", Q9)), c=_c(6, ["log", "softplus"], 1),
                     f=lambda y, mu, s: -(y - mu) / s - mp.log(s) - 2 * mp.log1p(mp.exp(-(y - mu) / s))),
    # log alpha - log beta + (alpha-1)(log x - log beta) - exp(alpha (log x - log beta)): sub sub sub mul add mul sub
    "weibull": dict(data=("pos",), params=(("alpha", "pos", Q4), ("beta", "pos", Q5)), c=_c(7, ["log", "log", "log", "exp"], 2),
                    f=lambda x, al, be: mp.log(al) - mp.log(be) + (al - 1) * (mp.log(x) - mp.log(be)) - (x / be) ** al),
    # y eta - softplus(eta): mul sub
    "bernoulli_logit": dict(data=("bin",), params=(("eta", "real", LOGIT),), c=_c(2, ["softplus"], 0),
                            f=lambda y, eta: y * eta - mp.log1p(mp.exp(eta))),
    # y eta - n softplus(eta) + lb: mul mul sub add
    "binomial_logit": dict(data=("cnt", "ntr", "lb"), params=(("eta", "real", LOGIT),), c=_c(4, ["softplus"], 0),
                           f=lambda y, n, lb, eta: y * eta - n * mp.log1p(mp.exp(eta)) + lb),
    # y eta - exp(eta) - lf: mul sub sub
    "poisson_log": dict(data=("cnt", "lf"), params=(("eta", "real", LOG_RATE),), c=_c(3, ["exp"], 0),
                        f=lambda y, lf, eta: y * eta - mp.exp(eta) - lf),
    # lgamma(y+phi) - lgamma(phi) - lf + y (eta - L) + phi (log phi - L), L = log(exp(eta) + phi): add sub sub, add, sub mul add, sub mul add; L twice
    "negative_binomial_log": dict(data=("cnt", "lf"), params=(("eta", "real", ETA), ("phi", "pos", PHI)),
                                  c=_c(11, ["lgamma", "lgamma", "exp", "log", "log", "log"], 1),
                                  f=lambda y, lf, eta, phi: (_lgamma(y + phi) - _lgamma(phi) - lf + y * (eta - mp.log(mp.exp(eta) + phi))
                                                             + phi * (mp.log(phi) - mp.log(mp.exp(eta) + phi)))),
}


def grid(name: str) -> np.ndarray:
    """the unconstrained positions of ``name``: the product of its parameters' grids, [rows, parameters]"""
    return np.array(list(itertools.product(*(g for _, _, g in DENSITIES[name]["params"]))), dtype=np.float64)


def _diff_partials(f, a, first_param):
    """f(a), df/da_k, and d2f/(da_j da_k) for the parameters j (= the arguments from ``first_param`` on); a term that is multiplied by
    a_k = 0 in the bound is not computed"""
    n = len(a)
    val = f(*a)
    d1 = [mp.diff(f, tuple(a), tuple(int(i == k) for i in range(n))) for k in range(n)]
    d2 = []
    for j in range(first_param, n):
        row = []
        for k in range(n):
            if a[k] == 0:
                row.append(mp.mpf(0))
                continue
            orders = [0] * n
            orders[j] += 1
            orders[k] += 1
            row.append(mp.diff(f, tuple(a), tuple(orders)))
        d2.append(row)
    return val, d1, d2


def density_rows(name: str, data: dict, rows=None) -> dict:
    """the reference of ``name`` at the rows ``rows`` of its grid (default: all): q, value, value_lo, vscale, grad, grad_lo, gscale"""
    e = DENSITIES[name]
    qs = grid(name)
    qs = qs if rows is None else qs[list(rows)]
    nd, P = len(e["data"]), len(e["params"])
    out = {k: [] for k in ("value", "value_lo", "vscale", "grad", "grad_lo", "gscale")}
    with mp.workdps(DPS):
        for q in qs:
            Q = [mp.mpf(float(t)) for t in q]
            pos = [kind == "pos" for _, kind, _ in e["params"]]
            theta = [mp.exp(t) if p else t for t, p in zip(Q, pos)]
            value, vscale = mp.mpf(0), mp.mpf(0)
            grad, gscale = [mp.mpf(0)] * P, [mp.mpf(0)] * P
            for i in range(N_OBS):
                a = [mp.mpf(float(data[col][i])) for col in e["data"]] + theta
                f, d1, d2 = e["partials"](a) if e.get("partials") else _diff_partials(e["f"], a, nd)
                value += f
                vscale += max(1, abs(f) + sum(abs(ak * dk) for ak, dk in zip(a, d1)))
                for j in range(P):
                    fac = theta[j] if pos[j] else mp.mpf(1)
                    h = fac * d1[nd + j]
                    dh = [fac * d2[j][k] + (d1[nd + j] if (pos[j] and k == nd + j) else 0) for k in range(len(a))]
                    grad[j] += h
                    gscale[j] += max(1, abs(h) + sum(abs(ak * t) for ak, t in zip(a, dh)))
            for j in range(P):
                if pos[j]:
                    value += Q[j]
                    vscale += abs(Q[j])
                    grad[j] += 1
                gscale[j] += 1
            hi, lo = _split(value)
            g = [_split(t) for t in grad]
            for k, t in zip(out, (hi, lo, _dbl(vscale), [t[0] for t in g], [t[1] for t in g], [_dbl(t) for t in gscale])):
                out[k].append(t)
    res = {k: np.array(v, dtype=np.float64) for k, v in out.items()}
    res["q"] = qs
    return res


def density_table(fix, name: str) -> dict:
    return {k: fix[f"den_{name}_{k}"] for k in ("q", "value", "value_lo", "vscale", "grad", "grad_lo", "gscale")}


def density_ratios(name: str, t: dict, logp, grad):
    """(err / bound of logp per row, err / bound of the gradient [rows, parameters]) of a double-precision evaluation on the table ``t``"""
    c = DENSITIES[name]["c"]
    rv = ratios(logp, t["value"], t["value_lo"], U * t["vscale"], N_OBS - 1 + c, underflow=False)
    rg = ratios(grad, t["grad"], t["grad_lo"], U * t["gscale"], N_OBS - 1 + 2 * c, underflow=False)
    return rv, rg


def record(label: str, worst: float) -> None:
    """the worst err / bound of a run: printed (pytest -s), and appended to the file DENSITY_TAIL_RECORD names when it is set — how the
    figures of profiles/density_tails.txt were taken"""
    line = f"density tails: {label}: worst err / bound = {worst:.3f}"
    print(line)
    if os.environ.get("DENSITY_TAIL_RECORD"):
        with open(os.environ["DENSITY_TAIL_RECORD"], "a") as f:
            f.write(line + "\n")
