"""Ahead-of-time compilation of the density libraries the Kalman smoother GPU tests use (tests/test_gpu_kalman_smoother_stages.py,
tests/test_gpu_kalman_smoother.py) into the in-tree cache nutpie_amd/_density_cache, which travels to the GPU box.  Run by
``__graft_entry__.build()`` as a separate process, started after tests/prebuild_kalman_cache.py and running beside the script that
follows; it only compiles — the seven libraries side by side (every compilation is a compiler process of its own, a library arrives
in the cache by an atomic rename), so that it adds next to nothing to the build's wall time.  Safe to run by hand:
    python tests/prebuild_kalman_smoother_cache.py
"""
import os
import sys
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    import kalman_models
    import kalman_smoother_reference

    kalman_smoother_reference.lib()                       # the C restatement of the order contract (and the filter's)
    kalman_smoother_reference.K.lib()
    models = [kalman_smoother_reference.probe(W).model for W in (1, 2, 4)]      # one probe per number of waves per chain
    models += [kalman_models.example(**kalman_smoother_reference.SMOOTHED_EXAMPLE).compile(waves_per_chain=W) for W in (1, 2)]      # the example with its smoothed level
    models.append(kalman_smoother_reference.local_level_smoothed().compile())      # the law test's marginal form with its two reported states
    models.append(kalman_models.local_level_latent(**kalman_smoother_reference.LAW).compile())
    with ThreadPoolExecutor(max_workers=len(models)) as pool:
        list(pool.map(lambda m: m.library_path(), models))


if __name__ == "__main__":
    main()
