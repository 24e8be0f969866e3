#!/usr/bin/env python3
"""CAM-B3LYP figures, one JSON line: seconds to evaluate the long-range ERI store against the full store (mi_eri_get_stats),
warm RKS cycle time of CAM-B3LYP against B3LYP, and the wall time of a 10-state TDDFT (RPA) kernel() for both.

  python tools/rsh_bench.py [benzene:cc-pvtz]"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "computational-chemistry-ai_amd", "python"))

import torch  # noqa: E402

SMILES = {"benzene": "c1ccccc1", "benzoquinone": "O=C1C=CC(=O)C=C1"}


def _mol(spec):
    from pyscf import gto
    from mi355scf import smiles_fixtures
    name, basis = spec.split(":")
    sym, xyz = smiles_fixtures.lookup(SMILES.get(name, name))
    return gto.M(atom=[(s, tuple(x)) for s, x in zip(sym, xyz)], basis=basis, unit="Angstrom", verbose=0)


def _cycle_ms(mf, n=20):
    st = mf._start(mf.make_rdm1())
    for _ in range(6):
        mf._step(st)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        mf._step(st)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e3


def _key(xc):
    return xc.replace("-", "").lower()


def main():
    from pyscf import dft, tdscf
    from mi355scf import engine
    spec = sys.argv[1] if len(sys.argv) > 1 else "benzene:cc-pvtz"
    mol = _mol(spec)
    out = {"case": spec, "nao": mol.nao}
    stores = {}
    for omega in (0.0, 0.33):      # a second evaluation of each after a warm-up one (first-use costs excluded)
        for _ in range(2):
            e = engine.Engine(mol)
            e.set_option("omega", omega)
            st = e.prepare_eri(1e-13)
            e.close()
        stores["lr" if omega else "full"] = st
    out["eri_seconds_full"] = stores["full"]["seconds_eri"]
    out["eri_seconds_lr"] = stores["lr"]["seconds_eri"]
    out["stored_gb"] = stores["full"]["stored_bytes"] / 1e9
    out["stored_gb_lr"] = stores["lr"]["stored_bytes"] / 1e9
    mfs = {}
    for xc in ("B3LYP", "CAM-B3LYP"):
        mf = dft.RKS(mol)
        mf.xc = xc
        mf = mf.to_gpu()
        out[f"e_tot_{_key(xc)}"] = mf.kernel()
        mfs[xc] = mf
    for rnd in range(2):           # alternating, two rounds: the spread between rounds shows the noise
        for xc, mf in mfs.items():
            out.setdefault(f"ms_per_cycle_{_key(xc)}", []).append(round(_cycle_ms(mf), 3))
    for rnd in range(2):           # first round: first-use costs of the response code paths; both rounds reported
        for xc, mf in mfs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            td = tdscf.TDDFT(mf)
            td.nstates = 10
            td.kernel()
            torch.cuda.synchronize()
            out.setdefault(f"td10_seconds_{_key(xc)}", []).append(round(time.perf_counter() - t0, 3))
            out[f"td10_jk_densities_{_key(xc)}"] = td.stats["n_jk_densities"]
            out[f"td10_first_ev_{_key(xc)}"] = float(td.e[0] * 27.211386245988)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
