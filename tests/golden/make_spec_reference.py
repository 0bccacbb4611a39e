"""Writes tests/golden/spec_reference.npz: the edge table of the numerics contract (tests/spec_reference.py: CASES) with its reference in mpmath at 50
digits, and profiles/spec_accuracy.txt: the largest error of include/nphip_spec.h as gcc compiles it (tests/fixtures/spec_header.c) at those points,
measured against mpmath directly (fractions of an ulp, which the rounded fixture cannot show).

    python tests/golden/make_spec_reference.py [--no-profile]

About a minute.  The reference alone decides what goes into the fixture; the header is only measured.
"""
from __future__ import annotations

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from tests import spec_reference as sr  # noqa: E402

WORD_TABLES = ("philox", "u01", "normal_pair")


def build_fixture():
    out = {}
    for name in sr.TABLES:
        x = sr.CASES[name]
        out[name + ".x"] = x.astype(np.uint32) if name in WORD_TABLES else (x.astype(np.float32) if name == "weights" else x)
        if name == "weights":
            continue
        for k, v in sr.reference(name).items():
            out["%s.%s" % (name, k)] = v
    w = sr.reference_weights()
    n_u = n_left_out = 0
    for name, r in w.items():
        n_u += r["keep"][1:].size
        n_left_out += int((~r["keep"][1:]).sum())
    # the rule "the decision is checked where |u - P| > n 2^-51" may leave out at most 1 % of the stored uniforms: the reference alone decides this
    assert n_left_out <= 0.01 * n_u, (n_left_out, n_u)
    out.update(sr.pack_weights(w))
    print("weights: %d of %d uniforms lie within n 2^-51 of the exact probability and are left out" % (n_left_out, n_u))
    return out


def measure():
    """The header's largest errors against mpmath: lines of text."""
    import mpmath as mp

    lines = []

    def worst(title, errs, args, unit):
        i = int(np.nanargmax(errs))
        a = np.atleast_1d(args[i])
        lines.append("%-34s max %.3g %s at %s" % (title, errs[i], unit, ", ".join("%s (%r)" % (float(v).hex(), float(v)) for v in a)))

    with mp.workdps(sr.DPS):
        f = lambda v: sr._exact(mp, v)   # noqa: E731

        def ulps(got, exact, ref):
            """|got - exact| in units of the spacing of float64 at ref (the correctly rounded value)."""
            sp = float(np.spacing(abs(ref))) if ref != 0 else 5e-324
            return float(abs(f(got) - exact) / f(sp))

        for name, fn in (("exp", mp.exp), ("log", mp.log), ("log1p", mp.log1p)):
            x = sr.CASES[name]
            got = sr.header(name, x)[:, 0]
            e_norm, e_sub = np.full(x.size, np.nan), np.full(x.size, np.nan)
            for i, (v, g) in enumerate(zip(x, got)):
                if not (np.isfinite(v) and np.isfinite(g)) or (name != "exp" and v <= 0) or (name == "exp" and not (-745.14 < v < 709.78)):
                    continue
                exact = fn(f(v))
                ref = sr._round(mp, exact)
                (e_sub if 0 < abs(ref) < sr.DBL_MIN else e_norm)[i] = ulps(g, exact, ref) if ref != 0 or g != 0 else 0.0
            worst(name + (" (normal results)" if name == "exp" else ""), e_norm, x, "ulp")
            if name == "exp":
                worst("exp (subnormal results)", e_sub, x, "ulp")
        x = sr.CASES["sincos2pi"]
        got = sr.header("sincos2pi", x)
        es, ec = np.zeros(x.size), np.zeros(x.size)
        for i, v in enumerate(x):
            ang = 2 * mp.pi * f(v)
            es[i], ec[i] = float(abs(f(got[i, 0]) - mp.sin(ang))), float(abs(f(got[i, 1]) - mp.cos(ang)))
        worst("sin(2 pi u) (absolute)", es, x, "")
        worst("cos(2 pi u) (absolute)", ec, x, "")
        x = sr.CASES["logaddexp"]
        got = sr.header("logaddexp", x)[:, 0]
        ea, eu = np.full(len(x), np.nan), np.full(len(x), np.nan)
        for i, ((a, b), g) in enumerate(zip(x, got)):
            if not (np.isfinite(a) and np.isfinite(b)):
                continue
            exact = f(max(a, b)) + mp.log1p(mp.exp(f(min(a, b)) - f(max(a, b))))
            ea[i] = float(abs(f(g) - exact)) / (2.0 ** -53 * max(1.0, abs(a), abs(b)))
            ref = sr._round(mp, exact)
            eu[i] = ulps(g, exact, ref) if ref != 0 else np.nan
        worst("logaddexp (2^-53 max(1,|a|,|b|))", ea, x, "units")
        worst("logaddexp (ulp of the result)", eu, x, "ulp")
        x = sr.CASES["exp_parts"]
        got = sr.header("exp_parts", x)
        er = np.array([float(abs(f(p) * mp.mpf(2) ** int(k) / mp.exp(f(v)) - 1)) for v, (p, k) in zip(x, got)])
        worst("exp_parts |p 2^k / e^x - 1|", er, x, "")
        lines.append("%-34s p in [%.6f, %.6f]" % ("exp_parts", got[:, 0].min(), got[:, 0].max()))
        x = sr.CASES["normal_pair"]
        got = sr.header("normal_pair", x)
        ref = sr.reference_normal_pair()["ref"]
        big = np.abs(ref[:, :2]) >= 1e-15
        d = sr.ulp_distance(got, ref[:, :2])
        i, j = np.unravel_index(int(np.argmax(np.where(big, d, 0))), d.shape)
        lines.append("%-34s max %d float64 steps from the correctly rounded value (z%d of words %s)" % ("normal_pair", d[i, j], j, [int(v) for v in x[i]]))
    return lines


def main():
    fix = build_fixture()
    np.savez_compressed(sr.FIXTURE, **fix)
    size = os.path.getsize(sr.FIXTURE)
    largest = max(os.path.getsize(os.path.join(HERE, f)) for f in os.listdir(HERE) if f != os.path.basename(sr.FIXTURE))
    print("%s: %d bytes (largest other fixture: %d)" % (sr.FIXTURE, size, largest))
    assert size < largest
    if "--no-profile" not in sys.argv:
        text = ["The largest errors of include/nphip_spec.h, compiled for the host (tests/fixtures/spec_header.c: gcc -O2 -ffp-contract=off), at the points of",
                "tests/spec_reference.py against mpmath at %d digits.  Written by tests/golden/make_spec_reference.py; the device and the oracle give the same bits" % sr.DPS,
                "at every one of these points (tests/test_gpu_spec_edges.py, tests/test_spec_reference_cpu.py).", ""]
        text += ["%-12s %d points" % (n, len(sr.CASES[n])) for n in sr.TABLES] + [""] + measure()
        path = os.path.join(ROOT, "profiles", "spec_accuracy.txt")
        with open(path, "w") as fh:
            fh.write("\n".join(text) + "\n")
        print("\n".join(text))


if __name__ == "__main__":
    main()
