"""Generates tests/golden/binding_names.json: the names the reference's pybind.cc files define and the functions its
bundle/bundle_adjuster.h declares, as tests/test_compat_names.py reads them, so that the test runs where the reference is absent.

Run from the repository root, where the reference is mounted:  python tests/golden/gen_binding_names.py
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import test_compat_names  # noqa: E402

json.dump(test_compat_names.binding_names(test_compat_names.REF), open(os.path.join(HERE, "binding_names.json"), "w"), indent=1)
