"""Writes tests/golden/depthmap/<case>.npz: the results of the numpy restatement of depthmap.cc (tests/depthmap_cases.py) for every case
and method, with a digest of the tables they were computed with (the tables are the library's, from osfm_depthmap_tables; no GPU is
needed).  tests/test_depthmap_host.py regenerates them and compares; tests/test_gpu_depthmap.py reads them."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

import depthmap_cases as cases  # noqa: E402


def generate(tables_of):
    """`tables_of(min_depth, max_depth)` -> the library's tables"""
    os.makedirs(cases.GOLDEN_DIR, exist_ok=True)
    for name in cases.CASES:
        problem = cases.problem(name)
        tables = tables_of(problem["min_depth"], problem["max_depth"])
        out = {"tables_digest": np.array(cases.tables_digest(tables, tables["init_depth"]))}
        for method, label in cases.METHOD_NAMES.items():
            result = cases.expected(name, method, tables, tables["init_depth"], fresh=True)
            for key, value in zip(("depth", "plane", "score", "nghbr"), result):
                out[f"{label}_{key}"] = value
        np.savez_compressed(os.path.join(cases.GOLDEN_DIR, name + ".npz"), **out)
        print(name, flush=True)


if __name__ == "__main__":
    from opensfm_amd import dense

    generate(dense.tables)
