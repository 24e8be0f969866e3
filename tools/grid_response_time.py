"""Time the XC gradient term with and without the grid-weight response, and one `mi_grid_becke_grad` launch beside one
`mi_grid_becke` launch on the same grid (the numbers of DESIGN.md section 8.12).
   python tools/grid_response_time.py benzene cc-pVTZ [level]
The density is that of a few density-fitted B3LYP cycles: the time of the XC term does not depend on its convergence."""
import sys
import time

import numpy as np
import torch

sys.path.insert(0, "computational-chemistry-ai_amd/python")
from mi355scf import fixtures, smiles_fixtures   # noqa: E402
from pyscf import gto, dft   # noqa: E402

name, basis = sys.argv[1], sys.argv[2]
level = int(sys.argv[3]) if len(sys.argv) > 3 else 3
if name == "benzene":
    atom = fixtures.BENZENE
else:
    sym, xyz = smiles_fixtures.TABLE["CC(C)Cc1ccc(cc1)C(C)C(=O)O"]()
    atom = "; ".join(f"{s} {x:.6f} {y:.6f} {z:.6f}" for s, (x, y, z) in zip(sym, xyz))
mol = gto.Mole()
mol.atom, mol.basis, mol.verbose = atom, basis, 0
mol.build()
mf = dft.RKS(mol, xc="B3LYP").density_fit()
mf.grids.level = level
mf.max_cycle = 3
mf.kernel()
dm = mf._dm
eng, gr = mf.engine, mf.grids
ng = gr.weights.numel()
print(f"{name}/{basis}: {mol.natm} atoms, {mol.nao} AOs, level {level}: {ng} points after density pruning", flush=True)


def best(fn, reps=5):
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return min(ts), float(np.median(ts)), out


g = mf.nuc_grad_method()
for flag in (False, True, False, True):
    g.grid_response = flag
    lo, med, de = best(lambda: g.grad_xc(dm))
    print(f"grad_xc grid_response={flag}: best {lo * 1e3:.1f} ms, median {med * 1e3:.1f} ms, |sum over atoms| {np.abs(de.sum(axis=0)).max():.2e}",
          flush=True)
e = torch.rand(ng, dtype=torch.float64, device=eng.device)
lo_w, med_w, _ = best(lambda: eng.becke_weights(gr.coords, gr.atom_of_dev, gr.vol, gr.adjust), 10)
lo_g, med_g, _ = best(lambda: eng.becke_weights_grad(gr.coords, gr.atom_of_dev, gr.vol, gr.adjust, e), 10)
print(f"one call on {ng} points (host set-up and synchronisation included): mi_grid_becke best {lo_w * 1e3:.3f} ms median {med_w * 1e3:.3f} ms, "
      f"mi_grid_becke_grad best {lo_g * 1e3:.3f} ms median {med_g * 1e3:.3f} ms, ratio {lo_g / lo_w:.2f}")
