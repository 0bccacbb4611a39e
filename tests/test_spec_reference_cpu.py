"""include/nphip_spec.h as gcc compiles it (tests/fixtures/spec_header.c), held to the 50-digit reference of tests/golden/spec_reference.npz at the edge
table of tests/spec_reference.py, and to the oracle's restatement bit for bit at the same points.  The bounds are the header's own claims (exp, log), what
tests/test_spec.py already allows (log1p, sin, cos) and the error analyses written next to each test; DESIGN.md §5 and profiles/spec_accuracy.txt have the
measured maxima.  The device runs the same records in tests/test_gpu_spec_edges.py."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import spec_reference as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def fix():
    return sr.load()


@pytest.fixture(scope="module")
def weights(fix):
    """name -> (x, leaf, total, reference) of every weight sequence, through the header."""
    ref, off, x = sr.unpack_weights(fix), sr.weight_offsets(), sr.args_of(fix, "weights")[:, 0]
    out = {}
    for name, (lo, hi) in off.items():
        leaf, tot, _ = sr.run_sequence(sr.header, x[lo:hi])
        out[name] = (x[lo:hi], leaf, tot, ref[name])
    return out


def _report(what, err, x, bound):
    i = int(np.argmax(err))
    print("%s: max %.4g (bound %.4g) at %s" % (what, err[i], bound, [float(v).hex() for v in np.atleast_1d(x[i])]))


# ---- the fixture ---------------------------------------------------------------------------------------------------------------------------------------------


def test_table_imports_without_mpmath():
    code = "import sys; from tests import spec_reference as sr; assert 'mpmath' not in sys.modules; assert len(sr.CASES['exp']) > 4000"
    subprocess.run([sys.executable, "-c", code], check=True, cwd=ROOT)


def test_fixture_holds_the_table(fix):
    for name in sr.TABLES:
        assert sr.same_bits(sr.args_of(fix, name), sr.CASES[name].reshape(len(sr.CASES[name]), -1)).all(), name
    golden = os.path.dirname(sr.FIXTURE)
    assert os.path.getsize(sr.FIXTURE) < max(os.path.getsize(os.path.join(golden, f)) for f in os.listdir(golden) if f != os.path.basename(sr.FIXTURE))
    for n in sr.TABLES:
        assert len(sr.CASES[n]) <= 5000


def test_fixture_is_what_the_reference_gives(fix):
    pytest.importorskip("mpmath")
    for name in sr.TABLES:
        if name == "weights":
            continue
        rows = np.arange(0, len(sr.CASES[name]), 37)
        for k, v in sr.reference(name, rows).items():
            want = fix["%s.%s" % (name, k)][rows]
            assert (sr.same_bits(v, want) if v.dtype == np.float64 else v == want).all(), (name, k)
    names = ["n2_s0.5", "n8_s3000", "n64_s30", "clamp"]
    got, want = sr.reference_weights(names), sr.unpack_weights(fix)
    for name in names:
        for k, v in got[name].items():
            assert np.array_equal(v[1:] if k in ("u", "decision", "keep") else v, want[name][k][1:] if k in ("u", "decision", "keep") else want[name][k]), (name, k)


# ---- header == oracle restatement ------------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("fn", list(sr.SHAPES))
def test_header_and_restatement_give_the_same_bits(oracle, fn):
    x = sr.records()[fn]
    a, b = sr.header(fn, x), oracle.spec(fn, x)
    bad = ~sr.same_bits(a, b)
    assert not bad.any(), (fn, x[bad.any(axis=1)][:5], a[bad.any(axis=1)][:5], b[bad.any(axis=1)][:5])


def test_oracle_entry_refuses_a_wrong_record_shape(oracle):
    import ctypes as C

    assert oracle.lib().oracle_spec(5, C.c_uint64(0), 1, None, 1, None) == -1 and oracle.lib().oracle_spec(17, C.c_uint64(0), 1, None, 1, None) == -1


# ---- accuracy of the header ------------------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("fn,bound", [("exp", 2), ("log", 2), ("log1p", 4), ("sqrt", 0), ("div", 0), ("u01", 0)])
def test_float64_steps_from_the_correctly_rounded_value(fix, fn, bound):
    """exp, log: the header's claim of 2 ulp; log1p on [0, 1]: the 4 ulp of tests/test_spec.py; sqrt, division (point 2 of the contract) and u01 (one
    rounding): correctly rounded.  Specials: NaN where the reference is NaN, and inf counts as the float64 after DBL_MAX."""
    x, ref = sr.args_of(fix, fn), fix[fn + ".ref"]
    got = sr.header(fn, x)[:, 0]
    d = sr.ulp_distance(got, ref)
    _report(fn, d, x, bound)
    assert d.max() <= bound
    if bound == 0:
        assert sr.same_bits(got, ref).all()       # the sign of a zero too
    zero = ref == 0
    assert (np.signbit(got[zero]) == np.signbit(ref[zero])).all()


def test_exp_special_values_and_cut_offs(fix):
    e = lambda *v: sr.header("exp", np.array(v))[:, 0].tolist()    # noqa: E731
    assert e(-745.13, -745.14) == [5e-324, 0.0]
    assert e(sr.EXP_HI, sr._next(sr.EXP_HI, 1), np.inf) == [pytest.approx(sr.DBL_MAX, rel=1e-13), np.inf, np.inf]
    assert e(sr.EXP_LO, sr._next(sr.EXP_LO, -1), -np.inf, 0.0, -0.0) == [0.0, 0.0, 0.0, 1.0, 1.0]
    # the leaf's form (parts of the clamped argument, then the scaling) is nphip_exp on the whole table and beyond the clamp
    x = sr.records()["exp_scale"]
    assert sr.same_bits(sr.header("exp_scale", x), sr.header("exp", x)).all()


def test_sincos2pi(fix):
    """Absolute error <= 4e-16 (tests/test_spec.py), measured against the double-double reference; exact at the quarter points."""
    u, ref, lo = sr.args_of(fix, "sincos2pi")[:, 0], fix["sincos2pi.ref"], fix["sincos2pi.lo"].astype(np.float64)
    got = sr.header("sincos2pi", u)
    err = np.abs((got - ref) - lo)
    _report("sincos2pi", err.max(axis=1), u, 4e-16)
    assert err.max() <= 4e-16
    for q, (s, c) in sr.QUARTERS.items():
        assert sr.header("sincos2pi", [q])[0].tolist() == [s, c]
    assert (np.abs(got) <= 1.0).all()


def test_logaddexp(fix):
    """|error| <= 8 * 2^-53 * max(1, |a|, |b|): one rounding of the sum, plus the log1p term (at most ln 2) at its 4 ulp.  The reference is the correctly
    rounded sum: its own half ulp (2^-53 of |result| <= max(|a|, |b|) + ln 2) is added to the bound."""
    x, ref = sr.args_of(fix, "logaddexp"), fix["logaddexp.ref"]
    got = sr.header("logaddexp", x)[:, 0]
    fin = np.isfinite(ref)
    assert sr.same_bits(got[~fin], ref[~fin]).all()
    scale = np.maximum(1.0, np.abs(x[fin]).max(axis=1))
    err = np.abs(got[fin] - ref[fin]) / (2.0 ** -53 * scale)
    _report("logaddexp", err, x[fin], 8)
    assert (np.abs(got[fin] - ref[fin]) <= 8 * 2.0 ** -53 * scale + 2.0 ** -53 * (np.abs(ref[fin]))).all()


def test_exp_parts(fix):
    """|p 2^k / e^x - 1| <= 2^-51 (exp's 2 ulp in relative form: p 2^k is the value before the exact scaling), p in [0.70, 1.42], k integral."""
    x = sr.args_of(fix, "exp_parts")
    p, k = sr.header("exp_parts", x).T
    hi, lo, e = fix["exp_parts.ref"], fix["exp_parts.lo"].astype(np.float64), fix["exp_parts.e"]
    assert (k == np.rint(k)).all() and (p >= 0.70).all() and (p <= 1.42).all()
    assert (np.abs(k - e) <= 1).all()
    t = np.ldexp(p, (k - e).astype(np.int32))          # exact
    rel = np.abs(((t - hi) - lo) / hi)                 # t - hi is exact: the two are within a factor 2
    _report("exp_parts", rel, x, 2.0 ** -51)
    assert rel.max() <= 2.0 ** -51


# ---- tree weights ------------------------------------------------------------------------------------------------------------------------------------------


def test_weight_sums(weights):
    """After n leaves |m 2^e / sum exp(x_i) - 1| <= n 2^-52 (each addition rounds once, the scalings are exact, a leaf is within 1 ulp, dropped terms are
    below n 2^-1000), at every stored prefix of every sequence; the mantissa stays in (0, 2n)."""
    worst = 0.0
    for name, (x, leaf, tot, ref) in weights.items():
        n = len(x)
        assert (tot[:, 0] > 0).all() and (tot[:, 0] < 2.0 * np.arange(1, n + 1)).all(), name
        assert (tot[:, 1] == np.maximum.accumulate(leaf[:, 1])).all(), name
        for c, hi, lo, e in zip(sr.checkpoints(n), ref["sum_hi"], ref["sum_lo"].astype(np.float64), ref["sum_e"]):
            m, em = tot[c - 1]
            rel = abs(((np.ldexp(m, int(em - e)) - hi) - lo) / hi)
            worst = max(worst, rel / (c * 2.0 ** -52))
            assert rel <= c * 2.0 ** -52, (name, c, rel)
    print("weights: the largest error is %.3f of its bound n 2^-52" % worst)


def test_weight_clamps(weights):
    """-energy_error beyond +-1e9 (inf included) is the leaf of +-1e9, where k ln2_hi is still exact; the sum of such a sequence is held by test_weight_sums."""
    x, leaf, _, _ = weights["clamp"]
    at = sr.header("w_leaf", np.array([1e9, -1e9]))
    assert at[:, 1].tolist() == [1442695041.0, -1442695041.0]          # rint(1e9 / ln 2)
    beyond = np.abs(x) >= 1e9
    assert beyond.sum() >= 5 and sr.same_bits(leaf[beyond], at[np.where(x[beyond] > 0, 0, 1)]).all()
    assert (np.abs(leaf[~beyond, 1]) < 1442695041.0).all()


def test_weight_drop_threshold(fix):
    """Contributions 2^-1000 and more below the larger weight are dropped: d = 999 is kept (exactly), d = 1000 is 0."""
    x, ref = sr.args_of(fix, "w_rel"), fix["w_rel.ref"]
    assert sr.same_bits(sr.header("w_rel", x)[:, 0], ref).all()
    d = x[:, 2] - x[:, 1]
    assert (ref[d == 999] == x[d == 999, 0] * 2.0 ** -999).all() and (ref[d == 999] > 0).all() and (d == 999).sum() >= 5
    assert (ref[d >= 1000] == 0).all() and (d == 1000).sum() >= 5
    xa = sr.args_of(fix, "w_add")
    got = sr.header("w_add", xa)
    assert sr.same_bits(got[:, 0], fix["w_add.ref"]).all() and (got[:, 1] == fix["w_add.e"]).all()     # one rounding of the aligned sum


def test_weight_acceptance_decisions(weights):
    """u * w_total < w_rel(other) is the exact decision u < w_other / w_total wherever u is further than n 2^-51 from the exact probability (the fixture
    says where; its make script asserts that this leaves out at most 1 % of the uniforms)."""
    n_checked = n_all = 0
    for name, (x, leaf, tot, ref) in weights.items():
        for j in range(2):
            rows = np.concatenate([ref["u"][1:, j:j + 1], tot[:-1], leaf[1:]], 1)
            got = sr.header("accept", rows)[:, 0] != 0
            keep = ref["keep"][1:, j]
            assert (got[keep] == ref["decision"][1:, j][keep]).all(), (name, j)
            n_checked, n_all = n_checked + int(keep.sum()), n_all + keep.size
    assert n_checked >= 0.99 * n_all


# ---- normals -------------------------------------------------------------------------------------------------------------------------------------------------


def test_normal_pair(fix):
    """z0, z1 within 8 ulp of sqrt(-2 ln u1) cos / sin(2 pi u2); where the exact value is below 1e-15 in magnitude, within 4e-16 sqrt(-2 ln u1)."""
    w, ref = sr.args_of(fix, "normal_pair"), fix["normal_pair.ref"]
    got = sr.header("normal_pair", w)
    for j in range(2):
        big = np.abs(ref[:, j]) >= 1e-15
        d = sr.ulp_distance(got[big, j], ref[big, j])
        _report("normal_pair z%d" % j, d, w[big], 8)
        assert d.max() <= 8
        assert (np.abs(got[~big, j] - ref[~big, j]) <= 4e-16 * ref[~big, 2]).all()
    assert (~(np.abs(ref[:, :2]) >= 1e-15)).sum() >= 4      # the octant boundaries are in the table


def test_largest_uniform_is_one_and_what_follows():
    """(k + 0.5) 2^-53 is not a float64 for odd k >= 2^52: it rounds to even, and k = 2^53 - 1 (probability 2^-53 per uniform) gives 1.0 — the interval is
    (0, 1].  u1 = 1.0 gives a radius of -0.0; u2 = 1.0 is outside the domain of nphip_sincos2pi, which answers (-1, 0) where sin, cos(2 pi) = (0, 1).  The
    arithmetic is the contract (every golden vector depends on it), so these values are pinned and documented in the header, not bounded."""
    hi, lo = sr._words_of_k(2 ** 53 - 1)
    assert sr.header("u01", [[hi, lo]])[0, 0] == 1.0 and sr.header("u01", [[0, 0]])[0, 0] == 2.0 ** -54
    assert sr.header("u01", [list(sr._words_of_k(2 ** 53 - 2))])[0, 0] == 1.0 - 2.0 ** -52       # 2^53 - 1.5 rounds to the even 2^53 - 2
    assert sr.header("sincos2pi", [1.0])[0].tolist() == [-1.0, 0.0]
    z0, z1 = sr.header("normal_pair", sr.NORMAL_PAIR_U2_ONE)[0]
    rad = np.sqrt(-2.0 * sr.header("log", [sr.u01_value(*sr.NORMAL_PAIR_U2_ONE[0, :2])])[0, 0])
    assert z0 == 0.0 and z1 == -rad


def test_philox_known_answers(fix):
    x, ref = sr.args_of(fix, "philox"), fix["philox.ref"]
    assert [tuple(int(v) for v in r) for r in ref[:3]] == [out for _, out in sr.PHILOX_KAT]
    assert (sr.header("philox", x) == ref).all()
