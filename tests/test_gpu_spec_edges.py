"""The device's include/nphip_spec.h at the edge table of tests/spec_reference.py (``nphip_test_spec``: one thread per point, one launch per function):
the same bits as the oracle's restatement and as the header compiled for the host — which tests/test_spec_reference_cpu.py holds to the 50-digit
reference of tests/golden/spec_reference.npz — at every point of every function, NaN equal to NaN and the sign of zero respected.  Reads the committed
fixture only."""
import numpy as np
import pytest

from tests import spec_reference as sr

pytestmark = pytest.mark.gpu

ONE_ARGUMENT = [fn for fn, (n_in, _) in sr.SHAPES.items() if n_in == 1]


@pytest.fixture(scope="module")
def fix():
    return sr.load()


@pytest.fixture(scope="module")
def device(hip):
    """fn -> the device's results on sr.records()[fn], each function computed once."""
    return {fn: hip.test_spec(fn, x) for fn, x in sr.records().items()}


def _assert_same_bits(a, b, x, what):
    bad = ~sr.same_bits(a, b).reshape(len(x), -1).all(axis=1)
    assert not bad.any(), "%s: %d of %d points differ, first at %s: %s != %s" % (what, bad.sum(), len(x), [float(v).hex() for v in x[bad][0]], a[bad][0], b[bad][0])


@pytest.mark.parametrize("fn", list(sr.SHAPES))
def test_device_oracle_and_header_give_the_same_bits(device, oracle, fn):
    x = sr.records()[fn]
    assert len(x) >= 50
    _assert_same_bits(device[fn], oracle.spec(fn, x), x, fn + ": device != oracle")
    _assert_same_bits(device[fn], sr.header(fn, x), x, fn + ": device != header")


def test_exp_scale_select_is_nphip_exp(device):
    """The pair path's scaling with its range cases as selects gives nphip_exp(x) on the whole exp table: between the cut-offs, beyond both (where the
    scaled product is made of bits the selects replace), at the cut-offs, at +-inf and NaN, and at +-1e9 and beyond after the clamp."""
    x = sr.records()["exp_scale_select"]
    assert (x > sr.EXP_HI).sum() >= 5 and (x < sr.EXP_LO).sum() >= 5 and np.isnan(x).any() and (np.abs(x) >= 1e9).sum() >= 6
    want = sr.header("exp", x)
    _assert_same_bits(device["exp_scale_select"], want, x, "exp_scale_select != nphip_exp")
    _assert_same_bits(device["exp_scale"], want, x, "nphip_exp_scale != nphip_exp")
    _assert_same_bits(device["exp"][:len(x) - 4], want[:len(x) - 4], x[:len(x) - 4], "device nphip_exp != header nphip_exp")


@pytest.mark.parametrize("fn", ["div", "sqrt", "u01", "w_rel"])
def test_correctly_rounded_on_the_device(device, fix, fn):
    """a / b and sqrt (point 2 of the contract: nphip_log and nphip_log1p divide), subnormal operands and results included; u01's one rounding; w_rel's exact
    scaling with its drop at d = 1000 (d = 999 kept): the fixture's correctly rounded values, bit for bit."""
    x, ref = sr.args_of(fix, fn), fix[fn + ".ref"]
    _assert_same_bits(device[fn][:len(x), 0], ref, x, fn)
    if fn == "w_rel":
        d = x[:, 2] - x[:, 1]
        got = device[fn][:len(x), 0]
        assert (got[d == 999] == x[d == 999, 0] * 2.0 ** -999).all() and (got[d == 999] > 0).all() and (got[d == 1000] == 0).all() and (d == 1000).sum() >= 5


def test_philox_known_answers_on_the_device(device, fix):
    got = device["philox"]
    assert [tuple(int(v) for v in r) for r in got[:3]] == [out for _, out in sr.PHILOX_KAT]       # Random123's kat_vectors
    assert (got == fix["philox.ref"]).all()


def test_weights_on_the_device(device, fix):
    """Sums against the aligned exact sum (one rounding) and the acceptance decisions against the exact ones, on the device's own results."""
    xa = sr.args_of(fix, "w_add")
    got = device["w_add"][:len(xa)]
    assert sr.same_bits(got[:, 0], fix["w_add.ref"]).all() and (got[:, 1] == fix["w_add.e"]).all()
    w, acc, o = sr.unpack_weights(fix), device["accept"][:, 0] != 0, 0
    for name in sr.weight_offsets():
        for j in range(2):
            keep, want = w[name]["keep"][1:, j], w[name]["decision"][1:, j]
            assert (acc[o:o + keep.size][keep] == want[keep]).all(), (name, j)
            o += keep.size
    assert o == acc.size


@pytest.mark.parametrize("fn", ONE_ARGUMENT)
@pytest.mark.parametrize("specials_in", ["upper", "lower"])
def test_a_lane_does_not_see_its_neighbours_special(hip, device, fn, specials_in):
    """The two halves of a wave hold different arguments, as the two leaves of a pair do: 32 table points beside 32 specials (sr.specials: NaN, inf, beyond the
    cut-offs and the clamp, zeros) in every wave, either way round.  Every lane gives what it gives in the plain run: the range cases are per lane."""
    x = sr.records()[fn][:, 0]
    n = len(x) // 32 * 32
    sp = np.resize(sr.specials(fn), n)
    rows = np.stack([x[:n].reshape(-1, 32), sp.reshape(-1, 32)][::1 if specials_in == "upper" else -1], 1).reshape(-1)
    got = hip.test_spec(fn, rows).reshape(n // 32, 2, 32, -1)
    own, other = (0, 1) if specials_in == "upper" else (1, 0)
    _assert_same_bits(got[:, own].reshape(n, -1), device[fn][:n], x[:n, None], fn + ": table lanes")
    _assert_same_bits(got[:, other].reshape(n, -1), sr.header(fn, sp), sp[:, None], fn + ": special lanes")
