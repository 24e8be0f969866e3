"""Analytic nuclear gradients of a state-specific CASSCF wavefunction behind `mc.nuc_grad_method()` (`casscf.CASSCF`).

The wavefunction is variational in the CI and in the orbital parameters, so the gradient is an expectation value -- no response
equations:

    dE/dR = D . dh - W . dS + 1/2 sum Gamma_abcd (ab|cd)^R + dE_nuc/dR

With D = Dc + Da (AO core and active one-particle densities) and PySCF's RDM convention E2,act = 1/2 sum Gamma_tuvw (tu|vw):

    E2     = [ 1/2 D.J[D] - 1/4 D.K[D] ]  +  1/2 sum_tuvw Lambda_tuvw (tu|vw)
    Lambda = Gamma_tuvw - gamma_tu gamma_vw + 1/4 (gamma_tv gamma_uw + gamma_tw gamma_uv)        (`cumulant`)

The bracket is what `Engine.grad_eri(D, 1.0)` contracts.  Lambda (the cumulant of the active 2-RDM, symmetrised over the 8-fold
symmetry of the integrals) vanishes for a closed-shell determinant.  As a symmetric matrix over the active pairs it is
eigendecomposed (`cumulant_pairs`),

    Lambda = sum_k s_k p^k (x) p^k,   K <= ncas (ncas + 1) / 2,   Q^k = Ca p^k Ca^T,

so the cumulant energy is 1/2 sum_k s_k (Q^k|Q^k) and the whole two-electron gradient is ONE pass over the derivative quartets
with the two-particle density  D_ab D_cd - 1/4 (D_ac D_bd + D_ad D_bc) + sum_k s_k Q^k_ab Q^k_cd  (`mi_grad_eri_pairs`,
`algorithm = "pairs"`).  `algorithm = "loop"` is the cross-check on the plain kernel alone: `grad_eri(D, 1.0)` plus K calls
`grad_eri(Q^k, 0.0)` scaled by s_k -- every derivative quartet K + 1 times.

The one-electron part is `Engine.grad_1e(D, W, g)` with W = C . 1/2 (F + F^T) . C^T, F the generalised Fock matrix
(`casscf.generalized_fock`); its core rows are 2 (F^I + F^A), so for a closed shell W is the 1/2 D F D of `grad.Gradients`.

Refused (NotImplementedError): state-averaged objects (they need coupled-perturbed MCSCF), `mcscf.CASCI` (its orbitals are not
variational), and whatever `casscf.CASSCF` itself refuses (sharded, direct-mode, density-fitted, PCM, open-shell references).
"""
import time

import numpy as np

from .grad import _GradScanner, assemble, log_gradient

ALGORITHMS = ("pairs", "loop")


# ---- plain algebra (NumPy in, NumPy out) ------------------------------------------------------------------------------------------
def cumulant(gamma, Gamma):
    """Lambda_tuvw = Gamma_tuvw - gamma_tu gamma_vw + 1/4 (gamma_tv gamma_uw + gamma_tw gamma_uv), averaged over the 8-fold
    symmetry (t <-> u, v <-> w, (tu) <-> (vw)) of the integrals it is contracted with."""
    g = np.asarray(gamma, dtype=np.float64)
    G = np.asarray(Gamma, dtype=np.float64)
    L = G - np.einsum("tu,vw->tuvw", g, g) + 0.25 * (np.einsum("tv,uw->tuvw", g, g) + np.einsum("tw,uv->tuvw", g, g))
    L = 0.5 * (L + L.transpose(1, 0, 2, 3))
    L = 0.5 * (L + L.transpose(0, 1, 3, 2))
    return 0.5 * (L + L.transpose(2, 3, 0, 1))


def cumulant_pairs(Lambda, ncas, rtol=1e-14):
    """(s [K], p [K, ncas, ncas]) with Lambda = sum_k s_k p^k (x) p^k, the p^k symmetric: the eigendecomposition of Lambda as a
    symmetric matrix over the packed pairs t >= u, the off-diagonal pairs weighted by 2 (so the p^k are orthonormal over the full
    pair index and s_k are Lambda's eigenvalues there).  Terms with |s_k| <= rtol max(1, max|s|) are dropped (the RDM elements are
    O(1): such a term is below the rounding of Lambda itself)."""
    L = np.asarray(Lambda, dtype=np.float64).reshape(ncas, ncas, ncas, ncas)
    t, u = np.tril_indices(ncas)
    w = np.where(t == u, 1.0, np.sqrt(2.0))
    M = L[t, u][:, t, u] * w[:, None] * w[None, :]
    s, V = np.linalg.eigh(0.5 * (M + M.T))
    keep = np.abs(s) > rtol * max(1.0, float(np.abs(s).max()))
    s, V = s[keep], V[:, keep]
    p = np.zeros((s.size, ncas, ncas))
    v = (V / w[:, None]).T
    p[:, t, u] = v
    p[:, u, t] = v
    return s, p


def energy_weighted_density(C, F):
    """W = C . 1/2 (F + F^T) . C^T (AO basis) of the generalised Fock matrix F (MO basis)."""
    C = np.asarray(C, dtype=np.float64)
    F = np.asarray(F, dtype=np.float64)
    return C @ (0.5 * (F + F.T)) @ C.T


# ---- driver -----------------------------------------------------------------------------------------------------------------------
class Gradients:
    """Analytic state-specific CASSCF gradient on the MI355X engine."""

    def __init__(self, mc, algorithm="pairs"):
        from .casscf import CASSCF
        if not isinstance(mc, CASSCF):
            raise NotImplementedError("CASCI nuclear gradients are not implemented: the orbitals of a CASCI wavefunction are not "
                                      "variational (orbital response needed); optimise them with mcscf.CASSCF")
        if mc.weights is not None:
            raise NotImplementedError("state-averaged CASSCF nuclear gradients are not implemented: they need coupled-perturbed "
                                      "MCSCF equations")
        self.base = mc
        self.mol = mc.mol
        self.de = None
        self.timing = {}
        self.npairs = None         # K of the last gradient
        self.verbose = mc.verbose
        self._algorithm = None
        self.algorithm = algorithm

    @property
    def algorithm(self):
        return self._algorithm

    @algorithm.setter
    def algorithm(self, name):
        if name not in ALGORITHMS:
            raise ValueError(f"CASSCF gradients: algorithm must be one of {ALGORITHMS}, got {name!r}")
        self._algorithm = name

    def kernel(self, mo_coeff=None, ci=None, atmlst=None):
        import torch
        from .ao2mo import resident_engine
        mc = self.base
        if mc.weights is not None:
            raise NotImplementedError("state-averaged CASSCF nuclear gradients are not implemented: they need coupled-perturbed "
                                      "MCSCF equations")
        if mc.ci is None or not mc.converged:
            mc.kernel()
        if not mc.converged:
            mc._log(2, "CASSCF gradients: the wavefunction is not converged; the gradient is not that of a stationary point")
        mf = mc._scf
        eng = resident_engine(mf, "CASSCF gradients")
        mol = mc.mol
        ncore, nc = mc.ncore, mc.ncas
        nocc = ncore + nc
        tm = {}
        t0 = time.time()
        # densities and generalised Fock matrix of the final orbitals: one macro evaluation, the CI warm-started from its solution
        cur = mc._macro(np.asarray(mc.mo_coeff if mo_coeff is None else mo_coeff), mc.ci if ci is None else ci)
        tm["state"] = time.time() - t0
        C = cur["mo"]
        gamma, Gamma, F = cur["gamma"], cur["Gamma"], cur["F"]
        Cc, Ca = C[:, :ncore], C[:, ncore:nocc]
        dev = dict(dtype=torch.float64, device=eng.device)
        D = torch.as_tensor(2.0 * Cc @ Cc.T + Ca @ gamma @ Ca.T, **dev).contiguous()
        W = torch.as_tensor(energy_weighted_density(C, F), **dev).contiguous()
        s, p = cumulant_pairs(cumulant(gamma, Gamma), nc)
        K = self.npairs = int(s.size)
        Q = torch.as_tensor(np.einsum("at,ktu,bu->kab", Ca, p, Ca, optimize=True), **dev).contiguous() if K else None

        def two_electron(g2):
            if self.algorithm == "pairs":
                return eng.grad_eri(D, 1.0, g2, pairs=(Q, s))
            eng.grad_eri(D, 1.0, g2)
            for k in range(K):
                gk = torch.zeros_like(g2)
                eng.grad_eri(Q[k].contiguous(), 0.0, gk)
                g2 += float(s[k]) * gk
        self.timing = tm
        self.de = de = assemble(eng, mol, D, W, two_electron, timing=tm)
        log_gradient(mc._log, mol, de, self.verbose >= 4, tm, f"CASSCF gradient ({self.algorithm}, K = {K})")
        return de

    grad = kernel

    def as_scanner(self):
        return _CASGradScanner(self)


def lowdin_orthonormalize(C, S):
    """C (C^T S C)^(-1/2): the orbitals C made orthonormal in the metric S, changed as little as possible."""
    w, U = np.linalg.eigh(C.T @ S @ C)
    return C @ ((U / np.sqrt(w)[None, :]) @ U.T)


class _CASGradScanner(_GradScanner):
    """(e_tot, de) at a new geometry: the SCF from the previous density, the CASSCF from the previous orbitals (re-orthonormalised
    in the new overlap) and CI vector."""

    def _energy(self, mol, dm0):
        mc = self.base
        mf = mc._scf
        warm = mc.ci is not None and mc.mo_coeff is not None
        mo_prev, ci_prev = (np.array(mc.mo_coeff), mc.ci) if warm else (None, None)
        self._run_scf(mol, dm0)       # (the gradient's prefetch overlaps the CASSCF as well)
        mc.mol = mol
        mo = lowdin_orthonormalize(mo_prev, mf.get_ovlp()) if warm else mf.mo_coeff
        mc.kernel(mo, ci0=ci_prev)
        self.converged = bool(mf.converged and mc.converged)
        return mc.e_tot
