"""Ahead-of-time compilation of the density libraries the HMM GPU tests use (tests/test_gpu_hmm_stages.py, tests/test_gpu_hmm.py) into
the in-tree cache nutpie_amd/_density_cache, which travels to the GPU box.  Run by ``__graft_entry__.build()`` as a separate process
after tests/prebuild_density_cache.py; it only compiles — libraries built after the engine library are not purged by that script.
Safe to run by hand:
    python tests/prebuild_hmm_cache.py
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    import hmm_models
    import hmm_reference

    hmm_reference.lib()                                   # the C restatement of the order contract
    for W in (1, 2, 4):                                   # one probe per number of waves per chain
        hmm_reference.probe(W).model.library_path()
    for shape in (hmm_models.EXAMPLE, hmm_models.PANEL):  # the example and its panel variant: the gradient rows at W = 1, 2, 4
        for W in (1, 2, 4):
            hmm_models.example(**shape).compile(waves_per_chain=W).library_path()
    hmm_models.example(**hmm_models.EXAMPLE).compile(resident=False).library_path()
    hmm_models.example(**hmm_models.LAW).compile().library_path()
    hmm_models.traced_twin(**hmm_models.EXAMPLE).library_path()
    hmm_models.hmm_with_cholesky().compile().library_path()    # tests/test_hmm_cpu.py: an HMM beside a matrix stage


if __name__ == "__main__":
    main()
