"""Writes tests/golden/low_rank_estimator_<case>.npz: the window of every case of tests/low_rank_reference.py::CASES, its settings, the
50-digit reference metric (dense up to 64 dimensions; the diagonal and four probe products above), ``k``, the sorted scores, the Gram
eigenvalues, and ``err_numpy`` / ``err_torch`` — the error of the two float64 formulations on the CPU against the reference, which the
GPU tests derive the kernel's bound from.

    python tests/golden/make_low_rank_reference.py [--jobs N] [--only CASE ...]      (from the repository root; minutes in all)
    python tests/golden/make_low_rank_reference.py --gamma-sweep                     (prints the table in profiles/low_rank_estimator_accuracy.txt)
"""
from __future__ import annotations

import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from tests import low_rank_reference as R  # noqa: E402


def make(name):
    t0 = time.perf_counter()
    c = R.case(name)
    x, g = R.inputs(c)
    pick = R.pick_of(c["m"], c["b"])
    want = R.reference(x, g, pick, c["gamma"], c["cutoff"], c["k_max"])
    with R.one_blas_thread():
        err_numpy, err_torch = R.cpu_errors(x, g, c, want)
    out = dict(x=x, g=g, pick=np.asarray(pick, dtype=np.int64), gamma=np.float64(c["gamma"]), cutoff=np.float64(c["cutoff"]), k_max=np.int64(c["k_max"]),
               err_numpy=np.float64(err_numpy), err_torch=np.float64(err_torch), **want)
    np.savez_compressed(R.fixture_path(name), **out)
    size = os.path.getsize(R.fixture_path(name))
    assert size < 100 * 1024, (name, size)
    return "%-32s k %2d  err_numpy %.2e  err_torch %.2e  %6d bytes  %5.1f s" % (name, int(want["k"]), err_numpy, err_torch, size, time.perf_counter() - t0)


def gamma_sweep_case(args):
    name, gamma = args
    c = dict(R.case(name), gamma=gamma)
    x, g = R.inputs(c)
    want = R.reference(x, g, R.pick_of(c["m"], c["b"]), gamma, c["cutoff"], c["k_max"])
    with R.one_blas_thread():
        return (name, gamma) + R.cpu_errors(x, g, c, want)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--jobs", type=int, default=min(8, os.cpu_count() or 1))
    ap.add_argument("--only", nargs="*", default=None)
    ap.add_argument("--gamma-sweep", action="store_true")
    a = ap.parse_args()
    import multiprocessing as mp

    import torch

    torch.set_num_threads(1)
    with mp.get_context("fork").Pool(a.jobs) as pool:
        if a.gamma_sweep:
            jobs = [(n, gm) for n in ("fullrank_24_8_8", "fullrank_70_32_32") for gm in (1e-5, 1e-6, 1e-7, 1e-8)]
            print("%-20s %8s %10s %10s" % ("case", "gamma", "err_numpy", "err_torch"))
            for name, gm, en, et in pool.imap(gamma_sweep_case, jobs):
                print("%-20s %8.0e %10.2e %10.2e" % (name, gm, en, et), flush=True)
            return
        names = a.only or R.CASE_NAMES
        for line in pool.imap_unordered(make, names):
            print(line, flush=True)


if __name__ == "__main__":
    main()
