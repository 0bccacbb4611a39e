"""Writes tests/golden/density_tail_reference.npz from the mpmath restatement tests/density_tail_reference.py: arguments, values and
scales only.  Needs mpmath and scipy (the doubles of lgamma(cnt + 1) and log C(ntr, cnt) that a user's data would hold):
    python tests/golden/make_density_tail_reference.py
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import density_tail_reference as R  # noqa: E402


def main():
    out = {}
    data = R.data_columns()
    for col, v in data.items():
        out[f"data_{col}"] = v
    for name in R.FUNCTIONS:
        for k, v in R.function_rows(name).items():
            out[f"fn_{name}_{k}"] = v
    for name in R.DENSITIES:
        for k, v in R.density_rows(name, data).items():
            out[f"den_{name}_{k}"] = v
        print(name, len(out[f"den_{name}_q"]), "rows")
    np.savez_compressed(R.FIXTURE, **out)
    print(R.FIXTURE, os.path.getsize(R.FIXTURE), "bytes")


if __name__ == "__main__":
    main()
