"""The probe models of tests/loop_edge_models.py restated by hand in 50-digit decimal arithmetic: log-density, gradient, and for every
output the rounding bound that a double-precision evaluation in any order has to keep.

Standard library only (``decimal``): ``Decimal(float)`` is exact, ``Decimal.exp`` and ``Decimal.ln`` are correctly rounded at the working
precision, pi is a literal.  Nothing of the code under test is used: not ``evaluate``, not ``gradient``, not ``_derive`` — the ranges of an
index are never formed, every sum over a group runs over the observations and adds into the group's element.

The model (tests/loop_edge_models.py), in the unconstrained coordinates q = (mu, b, rsg, rsig, a[G], variant's vectors):

    sg = exp(rsg), sig = exp(rsig), P(v) = -v^2 / 2 - C, C = log(2 pi) / 2
    eta_i = mu + b x_i + a[g_i] sg + variant_i,   z_i = (y_i - eta_i) / sig,   e_i = z_i / sig  (= d logp / d eta_i)
    logp  = rsg + rsig + P(mu) + P(b) + P(sg) + P(sig) + sum_g P(a_g) + [the variant's priors] + sum_i (-z_i^2 / 2 - rsig - C)
    d mu   = -mu + sum_i e_i                       d b    = -b + sum_i e_i x_i
    d rsg  = 1 - sg^2 + sg sum_i e_i a[g_i]        d rsig = 1 - sig^2 + sum_i (z_i^2 - 1)
    d a_g  = -a_g + sg sum_{i in g} e_i
    crossed  eta += c[h_i]:                 d c_g  = -c_g + sum_{i: h_i = g} e_i
    three    eta += a2[g_i] x_i + a3[g_i] w_i:   d a2_g = -a2_g + sum_{i in g} e_i x_i,  d a3_g likewise with w
    p2d      eta += B[p_i]:                 d B_q  = -B_q + sum_{i: p_i = q} e_i
    zs       eta += v[g_i],  v_g = r_g - s k1 (g < G - 1), v_{G-1} = -s k2,  s = sum r,  k1 = 1 / (sqrt G + G), k2 = 1 / sqrt G
             (k1, k2 the doubles the front end computes: constants of the model);  A_g = -v_g + sum_{i in g} e_i,
             d r_j = A_j - k1 sum_{g < G-1} A_g - k2 A_{G-1}

The bound.  An output that sums n addends in any order, each addend made by at most c operations that are correctly rounded or off by
1 ulp, differs from the exact value by at most (n - 1 + c) 2^-53 M to first order, M the sum of the magnitudes of the addends.  The
MAGNITUDE of an addend is its formula with every term of an inner sum replaced by its absolute value (|y| + |mu| + |b x| + ... for a
residual): rounding errors of an inner sum are relative to its terms, not to what is left after cancellation.  A logarithm of a computed
value turns that value's relative error into an absolute one, so log(sig) has the magnitude |rsig| + 1.  Device exp, log and log1p count
as 2 operations (2 ulp).  The counts, per addend and with multiplicity (z^2 uses z twice):

    sg, sig                   2           (one exp)
    eta_i        c_eta = 3 + t            t terms, the costliest a[g] sg (1 product + 2 for sg), t - 1 additions, rounded up;
                                          zs adds G + 1: v_g holds a sum over G - 1 values and two products
    z_i          c_z   = c_eta + 4        y - eta, / sig (1 + 2 for sig)
    logp addend  c_lp  = 2 c_z + 8        z z, the factor 1/2, log(sig) (2 + 2 for sig), two subtractions, the rounded constant C
    e_i          c_e   = c_z + 6          -z/2 - z/2 (3), / sig (1 + 2)
    gradient     c_g   = c_e + 4          up to a product with x_i or a[g_i], with sg (1 + 2); zs: + G + 4 (the sum over the groups, k1, k2)
    d rsig       c_s   = 2 c_z + 10       (-z/2 - z/2) z / sig, the chain factor sig (1 + 2), N / sig as N addends of magnitude 1
    n: logp 6 + (number of prior elements) + N;  d mu, d b, d rsg, d rsig: N + 2;  an element of a vector: its range's length + 1;  zs: N + G + 2
"""
import os
from decimal import Decimal, getcontext

import numpy as np

getcontext().prec = 50
PI = Decimal("3.14159265358979323846264338327950288419716939937510582097494")
C = (2 * PI).ln() / 2
U = Decimal(2) ** -53
D = Decimal


def _dec(v):
    return [D(float(t)) for t in np.asarray(v, dtype=np.float64).reshape(-1)]


def counts_c(variant: str, G: int) -> dict:
    t = {"base": 3, "crossed": 4, "three": 5, "zs": 4, "p2d": 4}[variant]
    c_eta = 3 + t + (G + 1 if variant == "zs" else 0)
    c_z = c_eta + 4
    c_e = c_z + 6
    return {"c_lp": 2 * c_z + 8, "c_g": c_e + 4 + (G + 4 if variant == "zs" else 0), "c_s": 2 * c_z + 10, "c_e": c_e}


def reference(variant: str, G: int, data: dict, q) -> dict:
    """One position ``q``: {"logp": (value, bound, M), "grad": [(value, bound, M)] in the order of the flat vector, "bound_mu": d mu's bound,
    "min_resid": the smallest |y_i - eta_i|, "obs_lp": the observations' addends of logp, "obs_e": their e_i} — all Decimal."""
    q = _dec(q)
    x, y, gi = _dec(data["x"]), _dec(data["y"]), [int(g) for g in data["gi"]]
    N = len(x)
    mu, b, rsg, rsig = q[0], q[1], q[2], q[3]
    a = q[4:4 + G]
    rest = q[4 + G:]
    sg, sig = rsg.exp(), rsig.exp()
    cc = counts_c(variant, G)

    def P(v):
        return -v * v / 2 - C

    def PM(v):
        return v * v / 2 + C

    # the variant's term of eta_i as (value, magnitude), its priors, and where e_i goes
    prior, prior_m, n_prior = D(0), D(0), G
    if variant == "crossed":
        hi = [int(h) for h in data["hi"]]
        extra = lambda i: (rest[hi[i]], abs(rest[hi[i]]))  # noqa: E731
    elif variant == "three":
        w = _dec(data["w"])
        a2, a3 = rest[:G], rest[G:]
        extra = lambda i: (a2[gi[i]] * x[i] + a3[gi[i]] * w[i], abs(a2[gi[i]] * x[i]) + abs(a3[gi[i]] * w[i]))  # noqa: E731
    elif variant == "zs":
        n = G
        k1 = D(1.0 / (float(np.sqrt(n)) + n))
        k2 = D(1.0 / float(np.sqrt(n)))
        s, s_abs = sum(rest, D(0)), sum((abs(r) for r in rest), D(0))
        v = [r - s * k1 for r in rest] + [-s * k2]
        v_m = [abs(r) + s_abs * k1 for r in rest] + [s_abs * k2]
        extra = lambda i: (v[gi[i]], v_m[gi[i]])  # noqa: E731
    elif variant == "p2d":
        pi = [int(p) for p in data["pi"]]
        extra = lambda i: (rest[pi[i]], abs(rest[pi[i]]))  # noqa: E731
    else:
        extra = lambda i: (D(0), D(0))  # noqa: E731
    vectors = {"crossed": [rest], "three": [rest[:G], rest[G:]], "zs": [v] if variant == "zs" else [], "p2d": [rest]}.get(variant, [])
    for vec in [a] + vectors:
        prior += sum((P(t) for t in vec), D(0))
        prior_m += sum((PM(t) for t in (v_m if variant == "zs" and vec is v else vec)), D(0))
    n_prior = len(a) + sum(len(vec) for vec in vectors)

    logp = rsg + rsig + P(mu) + P(b) + P(sg) + P(sig) + prior
    logp_m = abs(rsg) + abs(rsig) + PM(mu) + PM(b) + PM(sg) + PM(sig) + prior_m
    d_mu, m_mu = -mu, abs(mu)
    d_b, m_b = -b, abs(b)
    d_sg, m_sg = 1 - sg * sg, 1 + sg * sg
    d_sig, m_sig = 1 - sig * sig, 1 + sig * sig
    seg = {name: ([D(0)] * size, [D(0)] * size, [0] * size) for name, size in
           (("a", G), ("c", G), ("a2", G), ("a3", G), ("zs", G), ("B", 2 * G))}

    def add(name, k, val, m):
        s_, m_, n_ = seg[name]
        s_[k] += val
        m_[k] += m
        n_[k] += 1

    obs_lp, obs_e, min_resid = [], [], None
    for i in range(N):
        ev, em = extra(i)
        g = gi[i]
        eta = mu + b * x[i] + a[g] * sg + ev
        R = abs(y[i]) + abs(mu) + abs(b * x[i]) + abs(a[g] * sg) + em
        r = y[i] - eta
        min_resid = abs(r) if min_resid is None else min(min_resid, abs(r))
        z, Z = r / sig, R / sig
        e, E = z / sig, Z / sig
        lp = -z * z / 2 - rsig - C
        logp += lp
        logp_m += Z * Z / 2 + abs(rsig) + 1 + C
        obs_lp.append(lp)
        obs_e.append(e)
        d_mu += e
        m_mu += E
        d_b += e * x[i]
        m_b += E * abs(x[i])
        d_sg += sg * e * a[g]
        m_sg += sg * E * abs(a[g])
        d_sig += z * z - 1
        m_sig += Z * Z + 1
        add("a", g, sg * e, sg * E)
        if variant == "crossed":
            add("c", hi[i], e, E)
        elif variant == "three":
            add("a2", g, e * x[i], E * abs(x[i]))
            add("a3", g, e * w[i], E * abs(w[i]))
        elif variant == "zs":
            add("zs", g, e, E)
        elif variant == "p2d":
            add("B", pi[i], e, E)

    def held(value, n, c, m):
        """(value, its bound (n - 1 + c) 2^-53 M, M)"""
        return value, (n - 1 + c) * U * m, m

    out = {"logp": held(logp, 6 + n_prior + N, cc["c_lp"], logp_m), "min_resid": min_resid, "obs_lp": obs_lp, "obs_e": obs_e}
    grad = [held(d_mu, N + 2, cc["c_g"], m_mu), held(d_b, N + 2, cc["c_g"], m_b), held(d_sg, N + 2, cc["c_g"], m_sg),
            held(d_sig, N + 2, cc["c_s"], m_sig)]
    out["bound_mu"] = grad[0][1]

    def vector(name, values):
        s_, m_, n_ = seg[name]
        return [held(-values[k] + s_[k], n_[k] + 1, cc["c_g"], abs(values[k]) + m_[k]) for k in range(len(values))]

    grad += vector("a", a)
    if variant == "crossed":
        grad += vector("c", rest)
    elif variant == "three":
        grad += vector("a2", rest[:G]) + vector("a3", rest[G:])
    elif variant == "p2d":
        grad += vector("B", rest)
    elif variant == "zs":
        s_, m_, _ = seg["zs"]
        A = [-v[k] + s_[k] for k in range(G)]
        A_m = [v_m[k] + m_[k] for k in range(G)]
        tail = -k1 * sum(A[:-1], D(0)) - k2 * A[-1]
        tail_m = k1 * sum(A_m[:-1], D(0)) + k2 * A_m[-1]
        grad += [held(A[j] + tail, N + G + 2, cc["c_g"], A_m[j] + tail_m) for j in range(G - 1)]
    out["grad"] = grad
    return out


def check(variant: str, G: int, data: dict, positions, logp, grad) -> float:
    """the worst err / bound of a double-precision evaluation (``logp[n]``, ``grad[n, D]``) at ``positions``; an output with bound 0 (an
    empty range's sum: exactly its one addend) must be exact"""
    worst = 0.0
    for q, lp, g in zip(np.atleast_2d(positions), np.atleast_1d(logp), np.atleast_2d(grad)):
        ref = reference(variant, G, data, q)
        pairs = [(float(lp), ref["logp"])] + [(float(t), r) for t, r in zip(g, ref["grad"])]
        assert len(pairs) == 1 + len(q)
        for got, (want, bnd, _) in pairs:
            if got != got:
                return float("inf")
            err = abs(D(got) - want)
            worst = max(worst, float(err / bnd) if bnd > 0 else (0.0 if err == 0 else float("inf")))
    return worst


def record(label: str, worst: float) -> None:
    """the worst err / bound of a run: printed (pytest -s), and appended to the file LOOP_EDGE_RECORD names when it is set — how the
    figures of profiles/generated_loop_edges.txt were taken"""
    line = f"loop edges: {label}: worst err / bound = {worst:.3f}"
    print(line)
    if os.environ.get("LOOP_EDGE_RECORD"):
        with open(os.environ["LOOP_EDGE_RECORD"], "a") as f:
            f.write(line + "\n")
