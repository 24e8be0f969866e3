"""Spin-unrestricted Kohn-Sham behind `pyscf.dft.UKS` / `gpu4pyscf.dft.UKS` (call sites
`templates/calculate_bde.py:128,140,197,215`: `mf = UKS(mol); mf.xc = method` for the radical fragments).

Same grid, AO, density and V_xc HIP kernels as RKS, and the same block body (`dft.KSMixin._nr_raw`, over two densities); the
functional is evaluated by `xc_eval_spin_kernel` (forward-mode dual numbers over rho_a, rho_b, sigma_aa, sigma_ab, sigma_bb:
spin-scaled exchange, VWN/PW92 spin interpolation, open-shell LYP, PBE correlation with phi(zeta)) through `mi_xc_eval_spin_p`.
Meta-GGAs (TPSS; the template's default M06-2X, parameter tables unverified-memory) go through `mi_xc_eval_mgga_spin`: the same
kernel instantiated with tau_a, tau_b among the dual variables.
The grid is not pruned by density (PySCF's `small_rho_cutoff` step is RKS-only here).
"""
import numpy as np
import torch

from .dft import KSMixin, check_rsh_scf, is_rsh, lr_engine, parse_xc, rsh_coeff
from .uhf import UHF


class UKS(KSMixin, UHF):
    def _xc_block_size(self, n, npts):
        """Full blocks of a 64 N bytes per point working set and a short tail, not the equal blocks of RKS (whose rule would
        change the launch shapes of this loop)."""
        return max(self.grid_block, int(self._xc_block_bytes() / (64.0 * n)) // 1024 * 1024)

    def nr_uks(self, dm):
        """((N_alpha, N_beta), E_xc, V_xc[2,N,N], hyb) on device for the spin densities dm[2,N,N] (numint.nr_uks [MEM]): this
        rank's share of the grid; sharded callers all-reduce."""
        n = self.engine.nao
        vmat = torch.zeros(2, n, n, dtype=torch.float64, device=self.engine.device)
        tail = torch.zeros(3, dtype=torch.float64, device=self.engine.device)
        hyb = self._nr_uks_raw(dm, vmat, tail)
        return tail[:2], tail[2], vmat + vmat.transpose(1, 2), hyb

    def _nr_uks_raw(self, dm, vmat, tail):
        """`KSMixin._nr_raw` of the spin densities: unsymmetrised V_xc,s into `vmat[2,N,N]`, [N_alpha, N_beta, E_xc] into `tail`."""
        # spin densities declared projectors by the fast UHF/UKS loop (`_xc_projector_pair`): D_s = Z_s Z_s^T without orbitals
        Zts = [None, None]
        proj = getattr(self, "_xc_projector_pair", None)
        if self.xc_lowrank and proj is not None and proj[0] is dm:
            Zts = [self._lowrank_factor(proj[1][s_], proj[2][s_], ("uks", s_)) if proj[2][s_] > 0 else None for s_ in range(2)]
        return self._nr_raw(dm, Zts, [("uks", 0), ("uks", 1)], vmat, tail)

    def _fock_pair(self, dm):
        """One collective per Fock build: [J(2) | K(2) | Vxc(2) | N_alpha N_beta E_xc] partial sums in one flat buffer."""
        self.n_fock_builds = getattr(self, "n_fock_builds", 0) + 1
        eng = self.engine
        n = eng.nao
        nn = n * n
        hyb = parse_xc(self.xc)[0]
        rsh = is_rsh(self.xc)
        if rsh:          # K_s -> K_eff,s = hyb K_s + (alpha - hyb) K_LR,s (one K-only pass over the long-range store)
            check_rsh_scf(self)
            _omega, alpha, hyb = rsh_coeff(self.xc)
        with_k = abs(hyb) > 1e-12 or rsh
        nj = 2 if with_k else 1          # pure functionals: one J build for the total density
        nk = 2 if with_k else 0
        buf = torch.zeros((nj + nk + 2) * nn + 3, dtype=torch.float64, device=eng.device)
        J = buf[:nj * nn].view(nj, n, n)
        K = buf[nj * nn:(nj + nk) * nn].view(2, n, n) if with_k else None
        V = buf[(nj + nk) * nn:(nj + nk + 2) * nn].view(2, n, n)
        tail = buf[(nj + nk + 2) * nn:]
        self._nr_uks_raw(dm, V, tail)
        D = dm[0] + dm[1]
        if with_k:
            self._jk_into(dm.contiguous(), J, K)
            Jt = J[0] + J[1]
        else:
            self._jk_into(D.contiguous(), J[0], None)
            Jt = J[0]
        if self._nranks > 1:
            from . import parallel
            parallel.all_reduce_sum(buf, self._pg)
            Jt = J[0] + J[1] if with_k else J[0]
        if rsh:
            K.mul_(hyb).add_(lr_engine(self).get_jk(dm.contiguous(), with_j=False)[1], alpha=alpha - hyb)
            hyb = 1.0
        vxc = V + V.transpose(1, 2)
        self._nelec_grid = tail[:2]
        exc = tail[2]
        h1 = self._h1.unsqueeze(0)
        if with_k:
            F = h1 + Jt.unsqueeze(0) + vxc - hyb * K
            e = torch.sum(D * self._h1) + 0.5 * torch.sum(D * Jt) - 0.5 * hyb * torch.sum(dm * K) + exc
        else:
            F = h1 + Jt.unsqueeze(0) + vxc
            e = torch.sum(D * self._h1) + 0.5 * torch.sum(D * Jt) + exc
        return F, e
