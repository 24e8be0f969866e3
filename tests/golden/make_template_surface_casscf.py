#!/usr/bin/env python3
"""Generates tests/golden/template_surface_casscf.json: the chemistry import surface of the reference's
calculate_casscf.py, as names only (same extraction as make_template_surface.py).

  python tests/golden/make_template_surface_casscf.py <reference>/templates"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_template_surface import surface  # noqa: E402

if __name__ == "__main__":
    imports, chains = surface(os.path.join(sys.argv[1], "calculate_casscf.py"))
    out = {"script": "calculate_casscf", "imports": sorted(set(map(tuple, imports)), key=str), "chains": sorted(chains)}
    with open(os.path.join(HERE, "template_surface_casscf.json"), "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
