"""Ahead-of-time compilation of the density libraries the Kalman GPU tests use (tests/test_gpu_kalman_stages.py, tests/test_gpu_kalman.py)
into the in-tree cache nutpie_amd/_density_cache, which travels to the GPU box.  Run by ``__graft_entry__.build()`` as a separate
process after tests/prebuild_hmm_cache.py; it only compiles.  Safe to run by hand:
    python tests/prebuild_kalman_cache.py
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    import kalman_models
    import kalman_reference

    kalman_reference.lib()                                # the C restatement of the order contract
    for W in (1, 2, 4):                                   # one probe per number of waves per chain
        kalman_reference.probe(W).model.library_path()
    for W in (1, 2, 4):                                   # the example and the AR(p) model: the gradient rows at W = 1, 2, 4
        kalman_models.example(**kalman_models.EXAMPLE).compile(waves_per_chain=W).library_path()
        kalman_models.ar(**kalman_models.AR).compile(waves_per_chain=W).library_path()
    kalman_models.example(**kalman_models.EXAMPLE).compile(resident=False).library_path()
    kalman_models.traced_twin(**kalman_models.EXAMPLE).library_path()
    kalman_models.local_level_marginal().compile().library_path()      # the law test's two forms
    kalman_models.local_level_latent().compile().library_path()
    kalman_models.kalman_with_cholesky().compile().library_path()      # tests/test_kalman_cpu.py: a Kalman stage beside a matrix stage


if __name__ == "__main__":
    main()
