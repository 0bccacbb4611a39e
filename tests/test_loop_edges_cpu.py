"""The generated density loops at their shape edges, the part that needs no GPU: the numpy evaluation of every probe case against the
50-digit restatement (tests/loop_edge_reference.py) within the derived rounding bound, the condition on the inputs that makes a wrong
loop show, what the case table covers, what its generated sources contain, and a cross-compile per number of waves."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import loop_edge_models as M  # noqa: E402
import loop_edge_reference as R  # noqa: E402


def _all_cases(W):
    extra = [given for _, given in M.swap_cases(W)] + ([M.spill_case()] if W == 1 else [])
    return list(M.cases(W)) + extra


@pytest.mark.parametrize("W", M.WAVES)
def test_numpy_evaluation_is_within_the_bound_of_the_reference(W):
    """``_derive``, the adjoint rules and ``evaluate`` against a statement that shares nothing with them"""
    worst = 0.0
    for c in _all_cases(W):
        lp, g = c.compile().logp_and_grad_numpy(c.pos)
        ratio = R.check(c.variant, c.G, c.data, c.pos, lp, g)
        assert ratio <= 1.0, (c.name, ratio)
        worst = max(worst, ratio)
    for variant in M.VARIANTS:
        base, given = M.sweep(W, variant)
        m = base.compile(specialize=False)
        for c in given:
            lp, g = m.with_data(**c.updates()).logp_and_grad_numpy(c.pos)
            ratio = R.check(c.variant, c.G, c.data, c.pos, lp, g)
            assert ratio <= 1.0, (c.name, ratio)
            worst = max(worst, ratio)
    R.record(f"numpy W={W}", worst)


@pytest.mark.parametrize("W", M.WAVES)
def test_dropping_or_doubling_one_element_moves_an_output_by_100_bounds(W):
    """Dropping (or doubling) observation i changes logp by its addend lp_i and d mu by e_i; dropping a group's element changes logp by its
    prior's addend, at least log(2 pi) / 2 in magnitude.  One of the two has to be 100 bounds or more, at every position; and no residual
    is below 1e-3."""
    for c in _all_cases(W) + [g for v in M.VARIANTS for g in M.sweep(W, v)[1]]:
        for q in c.pos:
            ref = R.reference(c.variant, c.G, c.data, q)
            b_lp, b_mu = 100 * ref["logp"][1], 100 * ref["bound_mu"]
            assert ref["min_resid"] >= R.D("1e-3"), (c.name, ref["min_resid"])
            assert all(abs(lp) >= b_lp or abs(e) >= b_mu for lp, e in zip(ref["obs_lp"], ref["obs_e"])), c.name
            assert R.C >= b_lp, c.name


def test_the_table_covers_every_length_and_profile_at_every_W():
    for W in M.WAVES:
        T = 64 * W
        cs = M.cases(W)
        assert len(cs) <= 16
        assert {c.obs_class for c in cs} == set(M.OBS_CLASSES)
        assert {c.group_class for c in cs} == set(M.GROUP_CLASSES[W])
        assert {c.profile for c in cs} == set(M.PROFILES)
        for p in ("b", "d", "e", "f"):        # ((a) has one group with observations, (c) is split in c2 and c3: each once)
            assert {c.shuffled for c in cs if c.profile == p} == {False, True}, p
        assert {c.shuffled for c in cs if c.profile in ("c2", "c3")} == {False, True}
        assert {c.variant for c in cs} == set(M.VARIANTS)
        for variant in M.VARIANTS:
            base, given = M.sweep(W, variant)
            assert {c.obs_class for c in given} == set(M.OBS_CLASSES)
            assert base is given[-1] and {c.profile for c in given} == set(M.PROFILES)
            assert {c.shuffled for c in given} == {False, True}
        # the profiles are what their names say
        for c in cs:
            lens = c.counts
            if c.profile == "a":
                assert (lens > 0).sum() == 1 and (c.G < 3 or (lens[0] == 0 and lens[-1] == 0))
            elif c.profile == "b":
                assert (lens == 1).all()
            elif c.profile in ("c2", "c3"):
                assert lens.max() == int(c.profile[1])
            elif c.profile == "d":
                assert set((20, 21, 22) if c.variant == "three" else (31, 32, 33)) <= set(lens.tolist()) and np.sort(lens)[-4] <= 2
            elif c.profile == "e":
                U = min(4, -(-c.G // T))
                g = int(np.argmax(lens))
                assert U >= 2 and (g % (T * U)) // T == U - 1 and lens[g] == 10 and np.sort(lens)[-2] <= 2
            elif c.profile == "f":
                g = int(np.flatnonzero(lens == 40)[0])
                assert lens[g - 2:g].sum() == 0 and lens[:g - 2].sum() > 0 and lens[g + 1:].sum() > 0
        for (_, given), want in zip(M.swap_cases(W), (40, 1)):
            assert given.counts.max() == want
        assert (M.swap_cases(W)[1][1].counts == 0).any()


_LOOP = re.compile(r"// level (\d+), over (\w+)")
_STEP = re.compile(r"for \(int i0 = lane; i0 < n_(\w+); i0 \+= (\d+)\)")
_REST = re.compile(r"for \(int k = r0(\w+)_(\d)(?: \+ (\d+))?; k < r1")


def _caps(src):
    """{(loop number, index): {slot: cap}} of a generated source"""
    out, loop = {}, 0
    for line in src.splitlines():
        if _LOOP.search(line):
            loop += 1
        r = _REST.search(line)
        if r:
            out.setdefault((loop, r.group(1)), {})[int(r.group(2))] = int(r.group(3) or 0)
    return out


def test_the_generated_sources_of_the_table_take_every_path():
    """The table cannot stop exercising a path of ``_Gen.loop`` unnoticed: over its sources, caps of 0, 3, 21 and 32, a rest loop behind a
    capped batch, different caps in two slots of one loop, two segment dictionaries in one loop, a hoisted vector and one that is not, a
    partial parameter read, a grouped store, a ``perm`` output, a spilled array and the plain loop it takes, every ``unroll`` from 1 to 4,
    sizes as constants and as run-time values."""
    caps, unrolls, seen = set(), set(), set()
    for W in M.WAVES:
        T = 64 * W
        for c in M.cases(W):
            src = c.compile()._source
            assert f"const int n_obs = {c.N};" in src and f"const int n_group = {c.G};" in src
            by_loop = _caps(src)
            for (_, index), slots in by_loop.items():
                caps |= set(slots.values())
                if len(set(slots.values())) > 1:
                    seen.add("different caps in one loop")
                if any(v for v in slots.values()):
                    seen.add("rest loop behind a batch")
            if len({loop for loop, _ in by_loop}) < len(by_loop):
                seen.add("two segment dictionaries in one loop")
            for dim, step in _STEP.findall(src):
                if dim == "group":
                    unrolls.add(int(step) // T)
                    assert int(step) // T == max(1, min(4, -(-c.G // T)))
                elif dim == "obs":
                    assert int(step) == 4 * T          # (a data dimension: unrolled four times whatever its length)
            hoisted = re.search(r"const double H\d+_\d+ = ", src) is not None
            assert hoisted == (c.G <= 4 * T), c.name     # (a is read by the loop that stores a sg and by the loop of its gradient)
            seen.add("hoisted" if hoisted else "not hoisted")
            if c.variant == "zs":
                bounds = {int(v) for v in re.findall(r"< (\d+)\) \? x\[", src)}
                assert c.G - 1 in bounds, c.name
                seen.add("partial read")
            if re.search(r"M\d+\[pgi_\d\] = ", src):
                seen.add("grouped store")
            if re.search(r"g\[\d+ \+ \(\(i_\d % 2\) \* \d+ \+ i_\d / 2\)\] = ", src):
                assert c.variant == "p2d"
                seen.add("perm output")
        src = M.sweep(W, "base")[0].compile(specialize=False)._source
        assert "const int n_obs = data.n_x;" in src
        seen.add("run-time sizes")
    spilled = M.spill_case().compile()
    src = spilled._source
    assert M.spilled_doubles(spilled) == M.SPILL_N and M.spilled_doubles(M.spill_case(M.SPILL_N - 1).compile()) == 0
    assert "data.scratch__" in src and re.search(r"double\* const M\d+ = scratch_ \+ ", src)
    assert all(set(slots.values()) == {0} for (_, index), slots in _caps(src).items() if index == "gi")      # the plain loop
    assert M.spill_case().counts.max() >= 40
    assert {0, 3, 21, 32} <= caps, caps
    assert unrolls == {1, 2, 3, 4}
    assert seen == {"different caps in one loop", "rest loop behind a batch", "two segment dictionaries in one loop", "hoisted", "not hoisted",
                    "partial read", "grouped store", "perm output", "run-time sizes"}, seen


def test_with_data_at_unchanged_lengths_keeps_the_source():
    """the two specialised ``with_data`` cases keep the library: same source, the caps of the data it was compiled with"""
    for W in M.WAVES:
        for with_, given in M.swap_cases(W):
            m = with_.compile()
            swapped = m.with_data(**given.updates())
            assert swapped._source == m._source and swapped._waves == W
            assert not np.array_equal(swapped._data["gi__rows"], m._data["gi__rows"])


@pytest.mark.parametrize("W", M.WAVES)
def test_a_probe_model_cross_compiles(W):
    path = M.cases(W)[6].compile().library_path()
    assert os.path.exists(path)
