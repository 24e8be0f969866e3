#!/usr/bin/env python3
"""Generates tests/golden/template_surface.json: the chemistry import surface of the reference's template scripts, as data.

  python tests/golden/make_template_surface.py <reference>/templates

Each script is parsed with `ast` (read as text, never imported or executed).  Stored per script: every `import` /
`from ... import ...` of a package this repo stands in for, and every dotted attribute chain rooted at a name such an
import binds (`gto.Mole`, `scf.hf.RHF`, `gpu4pyscf.dft.rks.RKS`, `Chem.AddHs`, ...), with the root resolved to its module
path.  Only these names are kept -- no code of the scripts -- so tests/test_template_surface.py runs without the reference."""
import ast
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
OURS = ("pyscf", "gpu4pyscf", "cupy", "rdkit")   # top-level packages this repo stands in for
NAMES = ("calculate_energy", "optimize_geometry", "calculate_bde", "opt-freq", "calculate_interaction",
         "calculate_reaction_energy", "calculate_ir_spectrum")


def surface(path):
    """-> (imports, chains): imports = [(module, symbol|None)], chains = dotted names rooted at an alias of one of OURS."""
    with open(path, "r", encoding="utf-8") as fh:
        tree = ast.parse(fh.read())
    imports, alias = [], {}
    for node in ast.walk(tree):
        if isinstance(node, ast.Import):
            for a in node.names:
                if a.name.split(".")[0] in OURS:
                    imports.append((a.name, None))
                    alias[a.asname or a.name.split(".")[0]] = a.name if a.asname else a.name.split(".")[0]
        elif isinstance(node, ast.ImportFrom) and node.module and node.module.split(".")[0] in OURS:
            for a in node.names:
                imports.append((node.module, a.name))
                alias[a.asname or a.name] = node.module + "." + a.name
    chains = set()
    for node in ast.walk(tree):
        if isinstance(node, ast.Attribute):
            parts, cur = [], node
            while isinstance(cur, ast.Attribute):
                parts.append(cur.attr)
                cur = cur.value
            if isinstance(cur, ast.Name) and cur.id in alias:
                chains.add((alias[cur.id], tuple(reversed(parts))))
    return imports, chains


def main(templates):
    out = {}
    for name in NAMES:
        imports, chains = surface(os.path.join(templates, name + ".py"))
        out[name] = {"imports": [[m, s] for m, s in imports],
                     "chains": [[root, list(attrs)] for root, attrs in sorted(chains)]}
    with open(os.path.join(HERE, "template_surface.json"), "w") as fh:
        json.dump(out, fh, indent=1, sort_keys=True)
        fh.write("\n")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    main(sys.argv[1])
