#!/usr/bin/env python3
"""C-PCM costs on one MI355X (RHF): bytes and evaluation time of the surface-charge integral store B, the two per-cycle passes
(device events, achieved GB/s against 8 TB/s), a warm SCF cycle gas vs PCM water, and the PCM gradient.

  python tools/pcm_bench.py [benzene|ibuprofen ...]      (default: both)"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "computational-chemistry-ai_amd", "python"))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

CASES = {"benzene": ("c1ccccc1", "cc-pVTZ"), "ibuprofen": ("CC(C)Cc1ccc(cc1)C(C)C(=O)O", "def2-TZVP")}
PEAK = 8.0e12


def build(smiles, basis):
    from pyscf import gto
    from rdkit import Chem
    from rdkit.Chem import AllChem
    m = Chem.AddHs(Chem.MolFromSmiles(smiles))
    AllChem.EmbedMolecule(m, randomSeed=42)
    AllChem.MMFFOptimizeMolecule(m)
    conf = m.GetConformer()
    atoms = [a.GetSymbol() for a in m.GetAtoms()]
    mol = gto.Mole()
    mol.atom = "; ".join(f"{a} {conf.GetAtomPosition(i).x:.6f} {conf.GetAtomPosition(i).y:.6f} {conf.GetAtomPosition(i).z:.6f}"
                         for i, a in enumerate(atoms))
    mol.basis, mol.verbose = basis, 0
    mol.build()
    return mol


def events(fn, reps=20):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def warm_cycle(mf):
    mf.kernel()
    n0 = mf.cycles
    t = time.time()
    mf.kernel(dm0=mf.make_rdm1())
    torch.cuda.synchronize()
    return (time.time() - t) / max(mf.cycles + 1, 1) * 1e3, n0


def run(name):
    from pyscf import scf, solvent
    mol = build(*CASES[name])
    out = {"case": name, "nao": mol.nao}
    gas = scf.RHF(mol)
    out["gas_warm_ms_per_cycle"], _ = warm_cycle(gas)
    gas.reset(mol)
    del gas
    torch.cuda.empty_cache()
    mf = solvent.PCM(scf.RHF(mol))
    mf.eps = 78.3553
    mf._setup_once()
    ws = mf.with_solvent
    eng = mf.engine
    torch.cuda.synchronize()
    t = time.time()
    ws._key = None
    ws.build(eng, mol)
    torch.cuda.synchronize()
    out["pcm_setup_seconds"] = time.time() - t
    out["points"], out["B_bytes"] = ws.surface.npts, ws.nbytes
    out["B_eval_ms"] = events(lambda: eng.pcm_eval(ws._pts, ws._blk, ws.ld, ws._B), reps=3)
    D = torch.eye(mol.nao, dtype=torch.float64, device=eng.device)
    q = torch.ones(ws.surface.npts, dtype=torch.float64, device=eng.device)
    V = torch.empty_like(D)
    tp = events(lambda: eng.pcm_potential(ws._B, ws.ld, D, ws._dpack, ws._vn, ws._v))
    tf = events(lambda: eng.pcm_fock(ws._B, ws.ld, q, -1.0, False, ws._part, V))
    out["potential_pass_ms"], out["fock_pass_ms"] = tp, tf
    out["potential_GBs"] = ws.nbytes / (tp * 1e-3) / 1e9
    out["fock_GBs"] = ws.nbytes / (tf * 1e-3) / 1e9
    out["roofline_fraction_potential"] = ws.nbytes / (tp * 1e-3) / PEAK
    out["roofline_fraction_fock"] = ws.nbytes / (tf * 1e-3) / PEAK
    out["pcm_warm_ms_per_cycle"], out["pcm_cycles_cold"] = warm_cycle(mf)
    out["E_pcm"] = ws.e
    g = mf.nuc_grad_method()
    g.kernel()
    torch.cuda.synchronize()
    t = time.time()
    ws.grad(mf._dm)
    torch.cuda.synchronize()
    out["pcm_grad_seconds"] = time.time() - t
    t = time.time()
    g.kernel()
    out["total_grad_seconds"] = time.time() - t
    return out


if __name__ == "__main__":
    names = sys.argv[1:] or list(CASES)
    for n in names:
        print(json.dumps(run(n)), flush=True)
