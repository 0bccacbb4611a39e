"""Ahead-of-time compilation of the density libraries the loop-edge GPU tests use (tests/test_gpu_loop_edges.py) into the in-tree cache
nutpie_amd/_density_cache, which travels to the GPU box.  Run by ``__graft_entry__.build()`` as a separate process beside the
other prebuild scripts; it only compiles.  Safe to run by hand:
    python tests/prebuild_loop_edge_cache.py
"""
import os
import sys
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    import loop_edge_models as M

    models = []
    for W in M.WAVES:
        models += [c.compile() for c in M.cases(W)]                                                   # the specialised table: 16 + 12 + 12
        models += [M.sweep(W, variant)[0].compile(specialize=False) for variant in M.VARIANTS]        # one library for data of any length
    models.append(M.spill_case().compile())                                                           # an adjoint array in device memory
    # (compile(resident=False) is the same library: both forms of a density live in one; the compiler runs as a child process, so a few
    #  threads keep a few of them going — half the processors: build() runs this script beside the other prebuild scripts)
    with ThreadPoolExecutor(max_workers=max(1, min(4, len(os.sched_getaffinity(0)) // 2))) as pool:
        paths = list(pool.map(lambda m: m.library_path(), models))
    print(f"loop-edge cache: {len(set(paths))} libraries")


if __name__ == "__main__":
    main()
