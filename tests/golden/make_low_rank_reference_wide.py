"""Writes tests/golden/low_rank_estimator_wide_<case>.npz for every case of tests/low_rank_reference_wide.py::CASES: the SHA-256 of the
regenerated window (not the window: 64 x 1024 doubles are too large to commit, and the inputs regenerate bit for bit), the settings,
``pick``, the 50-digit reference metric (the diagonal and four probe products), ``k``, the sorted scores, the Gram eigenvalues, and
``err_numpy`` / ``err_torch`` — the error of the two float64 formulations on the CPU against the reference, which the GPU tests derive
the kernel's bound from.

    python tests/golden/make_low_rank_reference_wide.py --screen [--seeds N]         (float64, seconds: which seeds are worth a reference run)
    python tests/golden/make_low_rank_reference_wide.py [--jobs N] [--only CASE ...] (from the repository root; about six minutes per
                                                                                      order-128 case, in parallel)
"""
from __future__ import annotations

import argparse
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from tests import low_rank_reference as R  # noqa: E402
from tests import low_rank_reference_wide as W  # noqa: E402


def conditions(ev, scores, cutoff, k_max):
    """The conditions of test_fixture_inputs_sit_away_from_every_threshold, as a list of what is missed."""
    miss = []
    if not np.all((ev > 1e-6) | (ev < 1e-13)):
        miss.append("gram %s" % ev[(ev <= 1e-6) & (ev >= 1e-13)])
    if len(scores) and np.abs(scores - math.log(cutoff)).min() < 5e-3:
        miss.append("score at the cutoff")
    outside = int((scores > math.log(cutoff)).sum())
    if outside > k_max and scores[k_max - 1] - scores[k_max] < 1e-2:
        miss.append("gap at k_max %.3g" % (scores[k_max - 1] - scores[k_max]))
    return miss, outside


def make(name):
    t0 = time.perf_counter()
    c = W.case(name)
    x, g = W.inputs(c)
    pick = R.pick_of(c["m"], c["b"])
    want = R.reference(x, g, pick, c["gamma"], c["cutoff"], c["k_max"])
    with R.one_blas_thread():
        err_numpy, err_torch = R.cpu_errors(x, g, c, want)
    out = dict(sha256=np.array(W.digest(x, g)), pick=np.asarray(pick, dtype=np.int64), gamma=np.float64(c["gamma"]), cutoff=np.float64(c["cutoff"]),
               k_max=np.int64(c["k_max"]), err_numpy=np.float64(err_numpy), err_torch=np.float64(err_torch), **want)
    np.savez_compressed(W.fixture_path(name), **out)
    size = os.path.getsize(W.fixture_path(name))
    assert size < 100 * 1024, (name, size)
    miss, outside = conditions(want["gram_ev"], want["scores"], c["cutoff"], c["k_max"])
    return "%-32s k %2d outside %3d  err_numpy %.2e  err_torch %.2e  %6d bytes  %5.1f s  %s" % (
        name, int(want["k"]), outside, err_numpy, err_torch, size, time.perf_counter() - t0, "MISSES " + "; ".join(miss) if miss else "ok")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--jobs", type=int, default=min(8, os.cpu_count() or 1))
    ap.add_argument("--only", nargs="*", default=None)
    ap.add_argument("--screen", action="store_true")
    ap.add_argument("--seeds", type=int, default=1)
    a = ap.parse_args()
    names = a.only or W.CASE_NAMES
    if a.screen:
        for name in names:
            for seed in range(W.case(name)["seed"], W.case(name)["seed"] + a.seeds):
                c = dict(W.case(name), seed=seed)
                x, g = W.inputs(c)
                ev, scores = W.screen(x, g, np.asarray(R.pick_of(c["m"], c["b"])), c["gamma"])
                miss, outside = conditions(ev, scores, c["cutoff"], c["k_max"])
                print("%-32s seed %3d rank %3d of %3d outside %3d  %s" % (name, seed, len(scores), len(ev), outside, "; ".join(miss) or "ok"), flush=True)
        return
    import multiprocessing as mp

    import torch

    torch.set_num_threads(1)
    with mp.get_context("fork").Pool(a.jobs) as pool:
        # (the order-128 cases first: they take the longest)
        for line in pool.imap_unordered(make, sorted(names, key=lambda n: -W.case(n)["b"] * 10000 - W.case(n)["D"])):
            print(line, flush=True)


if __name__ == "__main__":
    main()
