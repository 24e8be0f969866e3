"""Time one FCI sigma = H c on random Hamiltonians, split into its three parts (gather D, GEMM, gather sigma).

    python tools/fci_sigma_bench.py [--cas 10 12 14] [--reps 7] [--warmup 2] [--nvec 1] [--workspace-mb N]

CAS(n,n): n orbitals, n electrons (Ms = 0).  Each part is timed with a device synchronisation around it (`FCISolver.profile`),
`warmup` untimed products first, then the median of `reps`.  Printed beside the accounting of DESIGN.md "Determinant FCI":
bytes of the two gather passes over the 2 (norb^2 + 1) ndet 8-byte work arrays against 8 TB/s, 2 norb^4 ndet flops of the GEMM.
One JSON line per space."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "computational-chemistry-ai_amd", "python"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cas", type=int, nargs="+", default=[10, 12])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--nvec", type=int, default=1)
    ap.add_argument("--workspace-mb", type=float, default=None)
    a = ap.parse_args()
    import torch
    from mi355scf import fci
    for n in a.cas:
        rng = np.random.default_rng(n)
        h = rng.standard_normal((n, n))
        h = h + h.T
        e = rng.standard_normal((n,) * 4)
        e = e + e.transpose(1, 0, 2, 3)
        e = e + e.transpose(0, 1, 3, 2)
        e = e + e.transpose(2, 3, 0, 1)
        s = fci.FCISolver()
        if a.workspace_mb:
            s.max_workspace_mb = a.workspace_mb
        tb = s._tab(n, (n // 2, n - n // 2))
        ndet = tb["nsa"] * tb["nsb"]
        M, _, _ = s._operator(h, e, n, tb["dev"])
        c = torch.randn((a.nvec, tb["nsa"], tb["nsb"]), dtype=torch.float64, device=tb["dev"])
        s.profile = True
        rows = []
        for it in range(a.warmup + a.reps):
            for k in ("gather_d", "gemm", "gather_sigma"):
                s.timing[k] = 0.0
            s.timing["chunks"] = 0
            s._sigma(M, c, tb)
            if it >= a.warmup:
                rows.append([s.timing["gather_d"], s.timing["gemm"], s.timing["gather_sigma"]])
        gd, gm, gs = (float(x) for x in np.median(np.array(rows), axis=0))
        plane = (n * n + 1) * ndet * 8 * a.nvec
        out = {"cas": n, "ndet": ndet, "nvec": a.nvec, "chunks": s.timing["chunks"], "gather_d_ms": 1e3 * gd, "gemm_ms": 1e3 * gm,
               "gather_sigma_ms": 1e3 * gs, "total_ms": 1e3 * (gd + gm + gs),
               "work_array_gb": 2 * plane * 1e-9,
               "gather_d_write_tbs": plane / gd * 1e-12, "gather_sigma_read_tbs": plane / gs * 1e-12,
               "gather_bound_ms_at_8tbs": 1e3 * plane / 8e12, "gemm_tflops": 2.0 * n ** 4 * ndet * a.nvec / gm * 1e-12}
        print(json.dumps(out), flush=True)
        del c, M
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
