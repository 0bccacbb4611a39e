"""Ahead-of-time compilation of the density libraries the density-tail GPU tests use (tests/test_gpu_density_tails.py) into the in-tree
cache nutpie_amd/_density_cache, which travels to the GPU box.  Run by ``__graft_entry__.build()`` as a separate process beside the
other prebuild scripts; it only compiles.  Safe to run by hand:
    python tests/prebuild_density_tail_cache.py
"""
import os
import sys
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    import density_tail_models as M

    models = M.all_models()      # one library per density entry and per function of the table
    # (the compiler runs as a child process, so a few threads keep a few of them going: at most four, build() runs this script beside
    #  the other prebuild scripts)
    with ThreadPoolExecutor(max_workers=max(1, min(4, len(os.sched_getaffinity(0)) // 2))) as pool:
        paths = list(pool.map(lambda m: m.library_path(), models))
    print(f"density-tail cache: {len(set(paths))} libraries")


if __name__ == "__main__":
    main()
