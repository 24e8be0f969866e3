"""Time one excited-state gradient of benzene (lowest singlet, TD-B3LYP by default), split into Z-vector, 1e, 2e and XC, with the
one-pass two-electron kernel and with `algorithm = "loop"`, next to the ground-state gradient; median of --repeat warm calls in one
process.  With --scan the third-order XC step (`xc3_step`) is scanned instead: the gradient at each step against the smallest-
difference pair, and the third-order matrix d2V[U, U] itself.
   python tools/tdgrad_time.py cc-pVTZ [--xc b3lyp] [--tda] [--repeat 3] [--scan]"""
import argparse
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, "computational-chemistry-ai_amd/python")
from mi355scf import fixtures, tdscf_grad   # noqa: E402
from pyscf import dft, gto, scf, tdscf   # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("basis")
ap.add_argument("--xc", default="b3lyp")
ap.add_argument("--tda", action="store_true")
ap.add_argument("--repeat", type=int, default=3)
ap.add_argument("--scan", action="store_true")
ap.add_argument("--mol", default="benzene")
a = ap.parse_args()

mol = gto.Mole()
mol.atom = fixtures.BENZENE if a.mol == "benzene" else a.mol
mol.basis, mol.verbose = a.basis, 0
mol.build()
if a.xc.lower() == "hf":
    mf = scf.RHF(mol)
else:
    mf = dft.RKS(mol)
    mf.xc = a.xc
mf.conv_tol = 1e-10
t0 = time.time()
mf.kernel()
t_scf = time.time() - t0
td = tdscf.TDA(mf) if a.tda else tdscf.TDDFT(mf)
td.nstates = 3
td.conv_tol = 1e-9
t0 = time.time()
td.kernel()
print(f"{a.mol}/{a.basis} ({mol.nao} AOs) {a.xc} {'TDA' if a.tda else 'TDDFT'}: SCF {t_scf:.2f} s, TD {time.time() - t0:.2f} s, "
      f"w = {td.e}, converged {td.converged}", flush=True)


def timed(make):
    rows = []
    for _ in range(a.repeat + 1):            # the first call (derivative records, allocations) is not counted
        torch.cuda.synchronize()
        t = time.time()
        g = make()
        de = g.kernel(state=1) if isinstance(g, tdscf_grad.Gradients) else g.kernel()
        torch.cuda.synchronize()
        rows.append(dict(g.timing, total=time.time() - t))
    keys = rows[-1].keys()
    return {k: statistics.median(r[k] for r in rows[1:]) for k in keys}, de, g


if a.scan:
    eng = mf.engine
    res = {}
    for step in (1e-1, 3e-2, 1e-2, 3e-3, 1e-3, 3e-4, 1e-4, 1e-5, 1e-6):
        g = td.nuc_grad_method()
        g.xc3_step = step
        de = g.kernel(state=1)
        x, y = td.xy[0]
        Nu = td._Co @ torch.as_tensor(x + y, device=eng.device) @ td._Cv.T
        res[step] = (de, tdscf_grad.third_order(td, 0.5 * (Nu + Nu.T), step).cpu().numpy())
    steps = list(res)
    ref = res[1e-3]
    for s in steps:
        print(f"xc3_step {s:.0e}: max |de - de(1e-3)| = {np.abs(res[s][0] - ref[0]).max():.2e}, max |d2V - d2V(1e-3)| = "
              f"{np.abs(res[s][1] - ref[1]).max():.2e} of {np.abs(ref[1]).max():.2e}")
    sys.exit(0)


def loop():
    g = td.nuc_grad_method()
    g.algorithm = "loop"
    return g


t_one, de_one, g_one = timed(td.nuc_grad_method)
t_loop, de_loop, _ = timed(loop)
t_gs, _de, _ = timed(mf.nuc_grad_method)
fmt = lambda t: ", ".join(f"{k} {v:.4f}" for k, v in t.items())
print(f"excited state, one pass : {fmt(t_one)}   (Z-vector {g_one.niter} iterations)")
print(f"excited state, loop     : {fmt(t_loop)}")
print(f"ground state            : {fmt(t_gs)}")
print(f"|de_onepass - de_loop| = {np.abs(de_one - de_loop).max():.2e}; 2e one pass / ground-state 2e = "
      f"{t_one['grad_eri'] / t_gs['grad_eri']:.2f}, loop / one pass = {t_loop['grad_eri'] / t_one['grad_eri']:.2f}")
