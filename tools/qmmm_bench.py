#!/usr/bin/env python3
"""Point-charge embedding costs on one MI355X (benzene/cc-pVTZ, RHF): `Engine.pc_fock` and `Engine.pc_grad` for 1 538 (the sites
of benzene's C-PCM cavity, widths included), 10^4 and 10^5 sites, the same 1 538 sites through the C-PCM store route (`pcm_eval`
+ `pcm_fock` + `pcm_grad`), and one embedded against one gas-phase `kernel()`.  Device events around warm repeats; the two
entry points copy the sites to the host once per call to check them, which the figures include.

  python tools/qmmm_bench.py [reps]"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "computational-chemistry-ai_amd", "python"))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from pcm_bench import build, events  # noqa: E402


def shell_sites(mol, n, seed):
    """n sites 4 .. 40 Bohr from the molecule's centre and at least 3 Bohr from every atom, every other one Gaussian."""
    rng = np.random.default_rng(seed)
    X = mol.atom_coords()
    out = np.zeros((0, 3))
    while out.shape[0] < n:
        u = rng.standard_normal((2 * n, 3))
        p = X.mean(axis=0) + u / np.linalg.norm(u, axis=1)[:, None] * rng.uniform(4.0, 40.0, (2 * n, 1))
        d = np.linalg.norm(p[:, None, :] - X[None], axis=2).min(axis=1)
        out = np.concatenate([out, p[d > 3.0]])
    pts = np.zeros((n, 4))
    pts[:, :3] = out[:n]
    pts[1::2, 3] = rng.uniform(0.5, 2.0, n // 2)
    return pts, rng.uniform(-0.8, 0.8, n)


def main(reps):
    from pyscf import qmmm, scf
    from mi355scf.pcm import PCMSolvent
    mol = build("c1ccccc1", "cc-pVTZ")
    gas = scf.RHF(mol)
    t = time.time()
    gas.kernel()
    torch.cuda.synchronize()
    out = {"nao": mol.nao, "gas_kernel_seconds_cold": time.time() - t}
    t = time.time()
    gas.kernel()
    torch.cuda.synchronize()
    out["gas_kernel_seconds"] = time.time() - t
    eng = gas.engine
    D = gas._dm.contiguous()
    V = torch.empty_like(D)
    dev = eng.device
    ws = PCMSolvent(mol).build(eng, mol)
    n0 = ws.surface.npts
    q0 = torch.as_tensor(np.random.default_rng(1).uniform(-0.05, 0.05, n0), device=dev)
    row = {"sites": n0}
    row["pcm_eval_ms"] = events(lambda: eng.pcm_eval(ws._pts, ws._blk, ws.ld, ws._B), reps)
    row["pcm_fock_ms"] = events(lambda: eng.pcm_fock(ws._B, ws.ld, q0, -1.0, False, ws._part, V), reps)
    part = torch.empty(len(eng.pcm_pairs(True)) * ws._blk.shape[0] * 3, dtype=torch.float64, device=dev)
    row["pcm_grad_ms"] = events(lambda: eng.pcm_grad(ws._pts, ws._blk, D, q0, part), reps)
    V_store = V.clone()
    row["pc_fock_ms"] = events(lambda: eng.pc_fock(ws._pts, q0, V, scale=-1.0), reps)
    row["pc_fock_vs_store_max_abs_diff"] = float((V - V_store).abs().max())
    row["pc_grad_ms"] = events(lambda: eng.pc_grad(ws._pts, q0, D), reps)
    row["pc_fock_us_per_site"] = 1e3 * row["pc_fock_ms"] / n0
    row["pc_grad_us_per_site"] = 1e3 * row["pc_grad_ms"] / n0
    row["pc_grad_work_MB"] = 8e-6 * eng.pc_grad_work(n0)
    out["rows"] = [row]
    print(json.dumps(row), flush=True)
    for n in (10_000, 100_000):
        pts, q = shell_sites(mol, n, n)
        dp, dq = torch.as_tensor(pts, device=dev), torch.as_tensor(q, device=dev)
        r = {"sites": n}
        r["pc_fock_ms"] = events(lambda: eng.pc_fock(dp, dq, V, scale=-1.0), max(2, reps // 4))
        r["pc_grad_ms"] = events(lambda: eng.pc_grad(dp, dq, D), max(2, reps // 4))
        r["pc_fock_us_per_site"] = 1e3 * r["pc_fock_ms"] / n
        r["pc_grad_us_per_site"] = 1e3 * r["pc_grad_ms"] / n
        r["pc_grad_work_MB"] = 8e-6 * eng.pc_grad_work(n)
        out["rows"].append(r)
        print(json.dumps(r), flush=True)
    pts, q = shell_sites(mol, 1538, 7)
    radii = np.where(pts[:, 3] > 0, 1.0 / np.where(pts[:, 3] > 0, pts[:, 3], 1.0), 0.0)
    emb = qmmm.mm_charge(scf.RHF(mol), pts[:, :3], 0.1 * q, radii=radii, unit="Bohr")
    emb.kernel()
    torch.cuda.synchronize()
    emb.reset(mol)
    t = time.time()
    emb.kernel()
    torch.cuda.synchronize()
    out["embedded_kernel_seconds"] = time.time() - t
    gas.reset(mol)
    t = time.time()
    gas.kernel()
    torch.cuda.synchronize()
    out["gas_kernel_seconds_after_reset"] = time.time() - t
    out["embedded_cycles"], out["gas_cycles"] = emb.cycles, gas.cycles
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 20)
