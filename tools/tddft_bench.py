#!/usr/bin/env python3
"""Linear-response figures, one JSON line: J/K per density of the batched build (mi_build_jk_multi) against the looped
single-density build for n_dm in --ndm (call time, synchronised, median of --reps), and the wall time of td.kernel() for
B3LYP TDA / RPA with the number of densities that went through J/K.  --xc-response analytic,fd runs every TD kind once per
route, the routes alternated in one process for --reps rounds (XC seconds per trial vector and td.kernel() wall time).

  python tools/tddft_bench.py --jk benzene:cc-pvtz --ndm 1,2,4,8,16,32 --td O=C1C=CC(=O)C=C1:6-31g*
  python tools/tddft_bench.py --td benzene:cc-pvtz --xc-response analytic,fd --reps 3"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "computational-chemistry-ai_amd", "python"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

SMILES = {"benzene": "c1ccccc1", "benzoquinone": "O=C1C=CC(=O)C=C1"}


def _mol(spec):
    from mi355scf import smiles_fixtures
    from mi355scf.mole import Mole
    name, basis = spec.split(":")
    sym, xyz = smiles_fixtures.lookup(SMILES.get(name, name))
    return Mole(atom=[(s, tuple(x)) for s, x in zip(sym, xyz)], basis=basis, verbose=0).build()


def _median_ms(fn, reps):
    t = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        t.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(t)), float(np.min(t)), float(np.max(t))


def bench_jk(spec, ndms, reps):
    from mi355scf.engine import Engine
    mol = _mol(spec)
    eng = Engine(mol)
    eng.prepare_eri(1e-13)
    out = {"system": spec, "nao": mol.nao, "store_gb": eng.stats()["stored_bytes"] / 1e9, "rows": []}
    rng = np.random.default_rng(0)
    for n in ndms:
        a = rng.standard_normal((n, mol.nao, mol.nao))
        D = torch.as_tensor(0.5 * (a + a.transpose(0, 2, 1)), device=eng.device)
        sym = [1] * n

        def loop():
            for m in range(n):
                eng.get_jk(D[m])

        def multi():
            eng.get_jk_multi(D, sym)
        loop(); multi()   # warm
        # A/B alternated inside one process
        rl, rm = [], []
        for _ in range(reps):
            rl.append(_median_ms(loop, 1)[0]); rm.append(_median_ms(multi, 1)[0])
        out["rows"].append({"n_dm": n, "loop_ms_per_density": float(np.median(rl)) / n, "multi_ms_per_density": float(np.median(rm)) / n,
                            "loop_spread_ms": [float(min(rl)), float(max(rl))], "multi_spread_ms": [float(min(rm)), float(max(rm))]})
    return out


def _run_td(mf, cls, nstates, route):
    td = cls(mf)
    td.nstates = nstates
    if route is not None:
        td.xc_response = route
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    e, _ = td.kernel()
    torch.cuda.synchronize()
    xs, xv = td.stats.get("xc_seconds", 0.0), td.stats.get("xc_vectors", 0)
    return {"seconds": time.perf_counter() - t0, "converged": bool(np.all(td.converged)),
            "jk_densities": td.stats["n_jk_densities"], "matvecs": td.stats["n_matvec"], "xc_seconds": xs, "xc_vectors": xv,
            "xc_ms_per_vector": 1e3 * xs / max(xv, 1), "e_ev": (np.asarray(e) * 27.211386245988).round(4).tolist()}


def bench_td(spec, nstates, routes=None, reps=1):
    from pyscf import dft, tdscf
    mol = _mol(spec)
    mf = dft.RKS(mol)
    mf.xc = "B3LYP"
    mf.kernel()
    res = {"system": spec, "nao": mol.nao, "nstates": nstates}
    for kind, cls in (("tda", tdscf.TDA), ("rpa", tdscf.TDDFT)):
        if not routes:
            res[kind] = _run_td(mf, cls, nstates, None)
            continue
        runs = {r: [] for r in routes}
        for _ in range(reps):            # A/B alternated inside one process
            for r in routes:
                runs[r].append(_run_td(mf, cls, nstates, r))
        res[kind] = {}
        for r, rr in runs.items():
            out = dict(rr[-1])
            for key in ("seconds", "xc_seconds", "xc_ms_per_vector"):
                v = [x[key] for x in rr]
                out[key], out[key + "_spread"] = float(np.median(v)), [float(min(v)), float(max(v))]
            res[kind][r] = out
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--jk", default=None)
    ap.add_argument("--ndm", default="1,2,4,8,16,32")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--td", default=None)
    ap.add_argument("--nstates", type=int, default=10)
    ap.add_argument("--xc-response", default=None, help="comma-separated TD XC routes to alternate: analytic,fd")
    a = ap.parse_args()
    out = {}
    if a.jk:
        out["jk"] = bench_jk(a.jk, [int(x) for x in a.ndm.split(",")], a.reps)
    if a.td:
        routes = a.xc_response.split(",") if a.xc_response else None
        out["td"] = bench_td(a.td, a.nstates, routes, a.reps if routes else 1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
