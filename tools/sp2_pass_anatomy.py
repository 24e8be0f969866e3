#!/usr/bin/env python3
"""Time planned purification chains of K back-to-back passes (K = 1, 5, 21) with HIP events, for the LDS-staged
`sp2_plan_kernel` (engine option sp2_direct=0) and the register-operand `sp2_direct_kernel` (sp2_direct=1), on the orthonormal
Fock-like matrix of benzene at N = nao of the basis.  The slope between K = 5 and K = 21 is the cost of one dependent pass
(kernel boundary included); K = 1 adds the host launch and the first-launch overheads.  Both kernels are also checked to give
the same projector.  python3 tools/sp2_pass_anatomy.py [basis ...]   (default: cc-pVTZ cc-pVDZ)"""
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, __file__.rsplit("/tools/", 1)[0] + "/computational-chemistry-ai_amd/python")
from mi355scf.engine import Engine  # noqa: E402
from mi355scf.mole import Mole  # noqa: E402
from mi355scf import fixtures, sp2plan  # noqa: E402

REPS, ROUNDS = 200, 5


def chain_us(eng, Fd, A, B, coef, tr):
    """median over ROUNDS of (time of REPS back-to-back chains) / REPS, in us"""
    for _ in range(10):
        eng.sp2_iterate_planned(Fd, A, B, coef, tr, out_scale=2.0)
    torch.cuda.synchronize()
    out = []
    for _ in range(ROUNDS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(REPS):
            eng.sp2_iterate_planned(Fd, A, B, coef, tr, out_scale=2.0)
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1) * 1e3 / REPS)
    return statistics.median(out)


def main(bases):
    for basis in bases:
        eng = Engine(Mole(atom=fixtures.BENZENE, basis=basis, verbose=0).build())
        n = eng.nao
        nocc = 21
        rng = np.random.default_rng(n)
        q, _ = np.linalg.qr(rng.normal(size=(n, n)))
        ev = np.sort(np.concatenate([rng.uniform(-20.0, -0.4, nocc), rng.uniform(0.1, 30.0, n - nocc)]))
        F = (q * ev) @ q.T
        F = 0.5 * (F + F.T)
        Fd = torch.as_tensor(F, device=eng.device)
        plan = sp2plan.plan(*sp2plan.bounds_from_spectrum(ev, nocc))
        # chains of K passes: the first K rows of the plan, padded with x -> x^2 passes where the plan is shorter
        full = np.vstack([plan] + [[[1.0, 0.0, 0.0]]] * max(0, 21 - plan.shape[0]))
        A = torch.empty((n, n), dtype=torch.float64, device=eng.device)
        B = torch.empty_like(A)
        tr = torch.zeros(64 * 80, dtype=torch.float64, device=eng.device)
        print(f"benzene/{basis}: N = {n}, triangular grid {((n + 15) // 16) * ((n + 15) // 16 + 1) // 2} workgroups, "
              f"plan of {plan.shape[0]} passes")
        res = {}
        for direct in (0, 1):
            eng.set_option("sp2_direct", direct)
            t = {K: chain_us(eng, Fd, A, B, full[:K], tr) for K in (1, 5, 21)}
            per = (t[21] - t[5]) / 16
            name = "sp2_direct_kernel" if direct else "sp2_plan_kernel  "
            print(f"  {name}  K=1 {t[1]:7.1f} us  K=5 {t[5]:7.1f} us  K=21 {t[21]:7.1f} us   per dependent pass {per:5.2f} us")
            r, off = eng.sp2_iterate_planned(Fd, A, B, plan, tr, out_scale=2.0)
            torch.cuda.synchronize()
            res[direct] = (r.cpu().numpy().copy(), tr[off:off + 2 * ((n + 15) // 16)].cpu().numpy().reshape(-1, 2).sum(axis=0))
        eng.set_option("sp2_direct", 0)
        d = np.abs(res[0][0] - res[1][0]).max()
        sym = np.array_equal(res[1][0], res[1][0].T)
        print(f"  max |D(plan) - D(direct)| = {d:.2e}, direct result exactly symmetric: {sym}, "
              f"last-pass traces {res[0][1]} / {res[1][1]}")


if __name__ == "__main__":
    main(sys.argv[1:] or ["cc-pVTZ", "cc-pVDZ"])
