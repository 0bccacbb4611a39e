"""Ahead-of-time compilation of the density libraries the wide-matrix GPU tests use (tests/test_gpu_matrix_wide.py) into the in-tree cache
nutpie_amd/_density_cache, which travels to the GPU box.  Run by ``__graft_entry__.build()`` as a separate process after the other
prebuild scripts; it only compiles.  Safe to run by hand:
    python tests/prebuild_wide_cache.py
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    import chain_stage_probes_wide as PW
    import matrix_models as mm
    import oracle

    oracle.lib()                                          # (the probes' cases factor their matrices with the restatement)
    for W in (1, 2, 4):                                   # one probe per number of waves per chain
        PW.probe(W).model.library_path()
    PW.containment_probe().model.library_path()
    for K in (33, 64, 128):
        for N in (1, 85):
            mm.gp_rows(K, N).compile(wide_matrices=True).library_path()
    mm.gp_rows(128, 1).compile(wide_matrices=True, waves_per_chain=4).library_path()
    c = mm.gp_rows(64, 1).compile(wide_matrices=True)     # the resident, batched and low-rank forms
    c.library_path(), c.library_path(low_rank=True)
    mm.gp_rows(40, 2, factor_deterministic=True).compile(wide_matrices=True).library_path()
    from nutpie_amd import from_torch_density, gp

    t, y = gp.synthetic_gp(100, 0.8, 1.0, 0.2)
    gp.compile_gp_regression(t, y).library_path()
    D, logp = gp.gp_regression_torch_density(t, y)
    from_torch_density(D, logp, compile=True, wide_matrices=True).library_path()


if __name__ == "__main__":
    main()
