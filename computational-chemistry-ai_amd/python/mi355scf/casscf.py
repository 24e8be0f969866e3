"""Complete-active-space SCF behind `pyscf.mcscf.CASSCF(mf, ncas, nelecas)` (`templates/calculate_casscf.py:92-118`, the default
branch) for a converged closed-shell RHF of this engine on one GPU with the resident, unsharded, full-Coulomb ERI store.

One macro iteration at the orbitals C = [Cc | Ca | Cv]:

    Jp[vw]   = sum_rs (pq|rs) Ca[r,v] Ca[s,w]          one pass over the resident tiles (`Engine.active_pair_j`)
    (tu|vw)  = Ca^T Jp[vw] Ca,   (pu|vw) = C^T Jp[vw] Ca
    F^I, E_core: frozen-core Fock matrix and energy (`ao2mo.core_fock`),  h_act = Ca^T F^I Ca
    CI       : `fcisolver.kernel`, warm-started from the previous vectors; gamma, Gamma from `make_rdm12`
    Da = Ca gamma Ca^T,  F^A = J(Da) - K(Da) / 2
    F        : generalised Fock matrix (`generalized_fock`),  g = 2 (F - F^T) on the non-redundant blocks (`orbital_gradient`)
    step     : C <- C exp(kappa), L-BFGS on kappa preconditioned with a diagonal Hessian estimate (`hessian_diagonal`)

The CI is solved again at every trial point, so the function minimised is E(C) = min_ci E(C, ci); by Hellmann-Feynman its
gradient is the orbital gradient above.  Safeguard: a trial point whose energy rises above the last accepted one (by more than
`RISE_NOISE`, the CI eigenvalue's own noise) is discarded, the step from the last accepted point is halved and the quasi-Newton
history dropped; every trial costs -- and is counted as -- one macro iteration.  J/K(Dc) is needed before the CI and J/K(Da)
after it (gamma depends on h_act, which depends on J/K(Dc)), so they are two single-density J/K builds per macro iteration
through the reference's own `_jk`; neither is ever built twice.

Saddle points: a rotation that mixes two symmetries has zero gradient at every symmetric point, so the descent alone stops at
symmetric saddles (h2o/sto-3g CAS(4,4) from RHF orbitals).  With `stability_check` (default) the driver finds the lowest
eigenpair of the orbital Hessian of E(C) (`lowest_eigenpair`; H v by central differences of the gradient) at the starting
orbitals and again at convergence; below -`stability_tol` it steps along the eigenvector and descends again.  The gradient
probes move no orbitals: they are counted in `stability_evaluations`, not in `macro_iterations`.  `stable` reports the last
search: True, False (negative curvature but no lower energy along it) or None (search not converged, nothing negative seen).

Convergence: max |g| < conv_tol_grad and |E - E_previous accepted| < conv_tol; a first point whose gradient is already below
the threshold has nothing to compare with and counts as converged.  `converged` is False when `max_cycle_macro` runs out or the
step shrinks to nothing.

State averaging (`state_average(weights)` / `state_average_`): `fcisolver.nroots = len(weights)`, gamma and Gamma are the weighted
averages, `e_tot` the weighted energy, `e_states` the per-state energies, `ci` the list of vectors.

The gradient, rotation and step algebra are plain functions of NumPy arrays (tests/test_casscf_host.py drives them on a CPU).

Not implemented (refused with NotImplementedError): the references of row "CASSCF" of `reference.SUPPORT` (ROHF / ROKS among them:
no ROHF-based CASSCF), references that have not been run, direct-mode stores, state-specific excited states (`fcisolver.nroots > 1`
without `state_average`).  Nuclear gradients (`nuc_grad_method()`, casscf_grad.py) exist for the state-specific wavefunction only:
state-averaged objects are refused there.
"""
import copy

import numpy as np
import torch

from .ao2mo import core_fock, resident_engine, symmetrize8
from .casci import CASCI
from .reference import require

RISE_NOISE = 1e-11        # Hartree: an energy "rise" below this is the CI eigenvalue's noise, not a rise
HDIAG_FLOOR = 0.05        # smallest diagonal Hessian element the preconditioner divides by
LBFGS_HISTORY = 12


# ---- plain algebra (NumPy in, NumPy out) ------------------------------------------------------------------------------------------
def pair_index(ncas):
    """(v, w) of the packed pairs v >= w in the order v (v + 1) / 2 + w."""
    v, w = np.tril_indices(ncas)
    return v, w


def unpack_pairs(X, ncas):
    """[npair, ...] over the packed pairs v >= w -> [ncas, ncas, ...], symmetric in (v, w)."""
    X = np.asarray(X)
    v, w = pair_index(ncas)
    out = np.empty((ncas, ncas) + X.shape[1:], dtype=X.dtype)
    out[v, w] = X
    out[w, v] = X
    return out


def check_weights(weights):
    """State-average weights: non-negative, summing to 1."""
    w = np.asarray(weights, dtype=np.float64).ravel()
    if w.size < 1 or not np.all(np.isfinite(w)) or np.any(w < 0) or abs(w.sum() - 1.0) > 1e-10:
        raise ValueError(f"state_average: weights must be non-negative and sum to 1, got {list(np.asarray(weights).ravel())}")
    return w


def average_rdms(weights, rdms):
    """Weighted (gamma, Gamma) of a list of per-state (dm1, dm2)."""
    w = check_weights(weights)
    if len(rdms) != w.size:
        raise ValueError(f"state_average: {w.size} weights for {len(rdms)} states")
    g = sum(wi * np.asarray(d1) for wi, (d1, _d2) in zip(w, rdms))
    G = sum(wi * np.asarray(d2) for wi, (_d1, d2) in zip(w, rdms))
    return g, G


def generalized_fock(FI, FA, gamma, Gamma, puvw, ncore, ncas):
    """Generalised Fock matrix in the MO basis, the density on the first index:
         core rows    F[i, p] = 2 (F^I + F^A)[i, p]
         active rows  F[t, p] = sum_u gamma[t, u] F^I[u, p] + sum_uvw Gamma[t, u, v, w] (p u|v w)
         virtual rows 0
    FI, FA: [nmo, nmo] (MO basis); puvw: [nmo, ncas, ncas, ncas]; Gamma in PySCF's convention (E_2 = 1/2 Gamma . (tu|vw))."""
    nmo = FI.shape[0]
    act = slice(ncore, ncore + ncas)
    F = np.zeros((nmo, nmo))
    F[:ncore] = 2.0 * (FI[:ncore] + FA[:ncore])
    F[act] = gamma @ FI[act] + np.einsum("tuvw,puvw->tp", Gamma, puvw, optimize=True)
    return F


def rotation_pairs(nmo, ncore, ncas):
    """(p, q), p < q, of the non-redundant rotations: core-active, core-virtual, active-virtual."""
    nocc = ncore + ncas
    kind = np.zeros(nmo, dtype=int)
    kind[ncore:nocc] = 1
    kind[nocc:] = 2
    p, q = np.triu_indices(nmo, 1)
    keep = kind[p] != kind[q]
    return p[keep], q[keep]


def orbital_gradient(F, ncore, ncas):
    """g[p, q] = 2 (F[p, q] - F[q, p]) on the non-redundant blocks, exactly zero elsewhere (antisymmetric [nmo, nmo]).  For
    p < q it is dE/dx of the rotation `rotate(C, x)` with kappa[q, p] = x = -kappa[p, q]."""
    nmo = F.shape[0]
    p, q = rotation_pairs(nmo, ncore, ncas)
    g = np.zeros((nmo, nmo))
    g[p, q] = 2.0 * (F[p, q] - F[q, p])
    g[q, p] = -g[p, q]
    return g


def pack(g, ncore, ncas):
    p, q = rotation_pairs(g.shape[0], ncore, ncas)
    return g[p, q].copy()


def kappa_matrix(x, nmo, ncore, ncas):
    """Antisymmetric generator of the packed parameters: kappa[q, p] = x, kappa[p, q] = -x for the pairs p < q."""
    p, q = rotation_pairs(nmo, ncore, ncas)
    K = np.zeros((nmo, nmo))
    K[q, p] = x
    K[p, q] = -np.asarray(x)
    return K


def expm_antisym(K):
    """exp(K) of a real antisymmetric K through the eigendecomposition of the Hermitian i K: orthogonal to rounding."""
    w, V = np.linalg.eigh(1j * K)
    return np.real((V * np.exp(-1j * w)[None, :]) @ V.conj().T)


def rotate(C, x, ncore, ncas):
    """C exp(kappa(x))."""
    return C @ expm_antisym(kappa_matrix(x, C.shape[1], ncore, ncas))


def hessian_diagonal(FI, FA, F, gamma, ncore, ncas):
    """Diagonal orbital-Hessian estimate from Fock diagonals for the packed pairs (preconditioner only: any positive numbers
    give a convergent safeguarded iteration), f = F^I + F^A:
         core-virtual    4 (f_aa - f_ii)
         active-virtual  2 gamma_tt f_aa - 2 F_tt
         core-active     4 (f_tt - f_ii) + 2 gamma_tt f_ii - 2 F_tt
    taken in absolute value and floored at HDIAG_FLOOR."""
    nmo = FI.shape[0]
    nocc = ncore + ncas
    f = np.diag(FI) + np.diag(FA)
    Fd = np.diag(F)
    gd = np.zeros(nmo)
    gd[ncore:nocc] = np.diag(gamma)
    p, q = rotation_pairs(nmo, ncore, ncas)
    h = np.empty(len(p))
    cv = (p < ncore) & (q >= nocc)
    av = (p >= ncore) & (q >= nocc)
    ca = (p < ncore) & (q < nocc)
    h[cv] = 4.0 * (f[q[cv]] - f[p[cv]])
    h[av] = 2.0 * gd[p[av]] * f[q[av]] - 2.0 * Fd[p[av]]
    h[ca] = 4.0 * (f[q[ca]] - f[p[ca]]) + 2.0 * gd[q[ca]] * f[p[ca]] - 2.0 * Fd[q[ca]]
    return np.maximum(np.abs(h), HDIAG_FLOOR)


def lbfgs_direction(g, hdiag, S, Y):
    """-H g of the L-BFGS two-loop recursion with the diagonal H0 = 1 / hdiag; S, Y: lists of steps and gradient changes."""
    q = g.copy()
    al = []
    for s, y in zip(reversed(S), reversed(Y)):
        rho = 1.0 / float(y @ s)
        a = rho * float(s @ q)
        al.append((a, rho, s, y))
        q -= a * y
    r = q / hdiag
    for a, rho, s, y in reversed(al):
        b = rho * float(y @ r)
        r += (a - b) * s
    return -r


def lowest_eigenpair(matvec, hdiag, tol=1e-4, below=None, max_space=24, seed=0):
    """Lowest eigenpair of a symmetric operator known through `matvec` (Davidson with Olsen's correction, preconditioner hdiag - theta), from a seeded
    random start (every element non-zero, so no symmetry of the problem is absent from the search space).  Returns (theta, x, done): `done` is True
    when the residual |A x - theta x| fell below `tol` or the space is the whole space.  With `below` set, the search also ends
    as soon as theta < below with a residual under |theta| / 2: the direction is then good enough to step along."""
    hdiag = np.asarray(hdiag, dtype=np.float64)
    n = hdiag.size
    b = np.random.default_rng(seed).standard_normal(n) / np.maximum(np.abs(hdiag), 1e-2)     # weighted towards the soft rotations
    B, AB = [], []
    theta, x = 0.0, b / np.linalg.norm(b)
    while True:
        for _ in range(2):                             # orthogonalise twice: the second pass removes the first one's rounding
            for c in B:
                b = b - float(c @ b) * c
        nb = float(np.linalg.norm(b))
        if nb < 1e-8:
            return theta, x, True
        B.append(b / nb)
        AB.append(np.asarray(matvec(B[-1]), dtype=np.float64))
        Bm, ABm = np.array(B).T, np.array(AB).T
        M = Bm.T @ ABm
        w, U = np.linalg.eigh(0.5 * (M + M.T))
        theta, x = float(w[0]), Bm @ U[:, 0]
        r = ABm @ U[:, 0] - theta * x
        rn = float(np.linalg.norm(r))
        if rn < tol or len(B) == n:
            return theta, x, True
        if below is not None and theta < below and rn < 0.5 * abs(theta):
            return theta, x, False
        if len(B) >= max_space:
            return theta, x, False
        den = hdiag - theta
        den = np.where(np.abs(den) < 1e-2, np.copysign(1e-2, den), den)
        mr, mx = r / den, x / den                      # Olsen's correction: the preconditioned residual made orthogonal to x,
        b = -mr + (float(x @ mr) / float(x @ mx)) * mx     # which does not stall where the diagonal is the whole operator


# ---- driver -----------------------------------------------------------------------------------------------------------------------
class CASSCF(CASCI):
    conv_tol = 1e-7
    conv_tol_grad = None       # None: sqrt(conv_tol)
    max_cycle_macro = 50
    max_stepsize = 0.3         # largest |kappa| element of one step
    ci_conv_tol = 1e-13        # the CI is converged well below the orbital thresholds: its residual enters the gradient linearly
    stability_check = True     # at convergence, look for a negative Hessian eigenvalue and leave the saddle along its vector
    stability_tol = 5e-6       # Hartree: curvature above -stability_tol counts as a minimum (the probes' own noise is ~1e-6)
    stability_probe = 1e-3     # |kappa| of the central-difference gradient probes

    def __init__(self, mf, ncas, nelecas, ncore=None):
        require(mf, "CASSCF")
        if mf.mo_coeff is None:
            raise NotImplementedError("CASSCF: the reference has no orbitals; run mf.kernel() first")
        super().__init__(mf, ncas, nelecas, ncore)
        self.weights = None
        self.e_states = None
        self.macro_iterations = 0
        self.stability_evaluations = 0
        self.stable = None

    # ---- state averaging ------------------------------------------------------------------------------------------------------
    def state_average_(self, weights=(0.5, 0.5)):
        w = check_weights(weights)
        self.weights = w
        self.fcisolver.nroots = int(w.size)
        return self

    def state_average(self, weights=(0.5, 0.5)):
        new = copy.copy(self)
        new.fcisolver = copy.copy(self.fcisolver)
        return new.state_average_(weights)

    # ---- one macro iteration --------------------------------------------------------------------------------------------------
    def _macro(self, mo, ci0):
        """Energy, CI, densities and generalised Fock matrix at the orbitals `mo`."""
        mf = self._scf
        eng = mf.engine
        nc, ncore = self.ncas, self.ncore
        nocc = ncore + nc
        C = torch.as_tensor(np.ascontiguousarray(mo), dtype=torch.float64, device=eng.device)
        Ca = C[:, ncore:nocc].contiguous()
        Jp = eng.active_pair_j(Ca)                                         # [npair, N, N]
        puvw = unpack_pairs(torch.matmul(C.T, torch.matmul(Jp, Ca)).cpu().numpy(), nc).transpose(2, 3, 0, 1)   # [p, u, v, w]
        del Jp
        eri = symmetrize8(torch.from_numpy(puvw[ncore:nocc].copy())).numpy()    # the store is screened
        FI, e_core = core_fock(mf, C, ncore)
        FI_mo = (C.T @ FI @ C).cpu().numpy()
        FI_mo = 0.5 * (FI_mo + FI_mo.T)
        h_act = FI_mo[ncore:nocc, ncore:nocc].copy()
        sol = self.fcisolver
        e, ci = sol.kernel(h_act, eri, nc, self.nelecas, ci0=ci0, ecore=e_core)
        if self.weights is None:
            if isinstance(ci, list):
                raise NotImplementedError("CASSCF: fcisolver.nroots > 1 needs state_average(weights); state-specific excited "
                                          "states are not implemented")
            gamma, Gamma = sol.make_rdm12(ci, nc, self.nelecas)
            e_states, e_tot = None, float(e)
        else:
            cis = ci if isinstance(ci, list) else [ci]
            if len(cis) != self.weights.size:
                raise NotImplementedError(f"CASSCF: {self.weights.size} state-average weights but the active space has only "
                                          f"{len(cis)} states")
            gamma, Gamma = average_rdms(self.weights, [sol.make_rdm12(c, nc, self.nelecas) for c in cis])
            e_states = np.atleast_1d(np.asarray(e, dtype=np.float64)).copy()
            e_tot = float(self.weights @ e_states)
            ci = cis
        gamma = 0.5 * (gamma + gamma.T)
        Da = Ca @ torch.as_tensor(gamma, dtype=torch.float64, device=eng.device) @ Ca.T
        J, K = mf._jk(Da)
        FA = J - 0.5 * K
        FA_mo = (C.T @ FA @ C).cpu().numpy()
        FA_mo = 0.5 * (FA_mo + FA_mo.T)
        F = generalized_fock(FI_mo, FA_mo, gamma, Gamma, puvw, ncore, nc)
        g = pack(orbital_gradient(F, ncore, nc), ncore, nc)
        return dict(mo=np.array(mo), e_tot=e_tot, e_states=e_states, e_core=e_core, ci=ci, gamma=gamma, Gamma=Gamma, F=F, g=g,
                    hdiag=hessian_diagonal(FI_mo, FA_mo, F, gamma, ncore, nc), fock_ao=FI + FA, h_act=h_act, eri=eri,
                    ci_converged=bool(np.all(sol.converged)))

    # ---- driver ---------------------------------------------------------------------------------------------------------------
    def kernel(self, mo_coeff=None, ci0=None):
        mf = self._scf
        resident_engine(mf, "CASSCF")
        if not getattr(mf, "converged", True):
            self._log(2, "CASSCF: the reference SCF is not converged")
        if mo_coeff is None:
            mo_coeff = self.mo_coeff if self.mo_coeff is not None else mf.mo_coeff
        mo = np.array(mo_coeff, dtype=np.float64)
        n, nmo = mo.shape
        ncore, nc = self.ncore, self.ncas
        nocc = ncore + nc
        if n != mf.engine.nao or nocc > nmo:
            raise ValueError(f"CASSCF: mo_coeff of shape {mo.shape} for {mf.engine.nao} AOs, ncore + ncas = {nocc}")
        tol_g = float(self.conv_tol_grad) if self.conv_tol_grad is not None else float(np.sqrt(self.conv_tol))
        sol = self.fcisolver
        sol.conv_tol = min(sol.conv_tol, self.ci_conv_tol)
        npar = len(rotation_pairs(nmo, ncore, nc)[0])
        self._log(4, f"CASSCF: ncore = {ncore}, ncas = {nc}, nelecas = {self.nelecas}, {npar} rotations, conv_tol = {self.conv_tol:g}, "
                     f"conv_tol_grad = {tol_g:g}")
        cur = self._macro(mo, ci0)
        it = 1
        self.stability_evaluations = 0
        self.stable = None
        converged = npar == 0 or float(np.abs(cur["g"]).max()) < tol_g
        self._log(4, f"CASSCF macro {it}: E = {cur['e_tot']:.12f}  max|g| = {np.abs(cur['g']).max() if npar else 0.0:.3e}")
        first = True
        while True:
            if not converged:
                if first and self.stability_check:      # negative curvature at the start: take it before descending, so that the
                    lam, v, _ = self._lowest_curvature(cur)     # descent does not first converge onto the saddle it leads away from
                    self._log(4, f"CASSCF start: lowest Hessian eigenvalue {lam:.3e} after {self.stability_evaluations} probes")
                    if lam < -self.stability_tol:
                        cur, it, _ = self._leave_saddle(cur, it, v if float(v @ cur["g"]) <= 0.0 else -v)
                cur, it, converged = self._descend(cur, it, tol_g)
            first = False
            if not converged or not self.stability_check or npar == 0:
                break
            lam, v, done = self._lowest_curvature(cur)
            self._log(4, f"CASSCF stability: lowest Hessian eigenvalue {lam:.3e} after {self.stability_evaluations} probes"
                         f"{'' if done else ' (search not converged)'}")
            if lam >= -self.stability_tol:
                self.stable = True if done else None
                if not done:
                    self._log(2, "CASSCF: the search for the lowest Hessian eigenvalue did not converge; no negative curvature found")
                break
            self.stable = False
            cur, it, left = self._leave_saddle(cur, it, v)
            if not left:
                self._log(2, f"CASSCF: Hessian eigenvalue {lam:.3e} but no lower energy along its vector; staying")
                break
            converged = False
        self.macro_iterations = it
        return self._finish(cur, converged, nmo)

    def _descend(self, cur, it, tol_g):
        """Safeguarded L-BFGS from the accepted point `cur`: (last accepted point, macro iterations so far, converged)."""
        ncore, nc = self.ncore, self.ncas
        S, Y = [], []
        scale = 1.0
        converged = False
        while not converged and it < int(self.max_cycle_macro):
            step = lbfgs_direction(cur["g"], cur["hdiag"], S, Y)
            if float(step @ cur["g"]) >= 0.0:           # not a descent direction: drop the history
                S, Y = [], []
                step = -cur["g"] / cur["hdiag"]
            big = float(np.abs(step).max())
            if big > self.max_stepsize:
                step *= self.max_stepsize / big
            step *= scale
            if float(np.abs(step).max()) < 1e-9:
                self._log(2, "CASSCF: the step shrank to nothing without lowering the energy")
                break
            new = self._macro(rotate(cur["mo"], step, ncore, nc), cur["ci"])
            it += 1
            dE = new["e_tot"] - cur["e_tot"]
            gmax = float(np.abs(new["g"]).max())
            self._log(4, f"CASSCF macro {it}: E = {new['e_tot']:.12f}  dE = {dE:.3e}  max|g| = {gmax:.3e}  max|step| = {np.abs(step).max():.3e}")
            if dE > RISE_NOISE:                         # a rise: back to the last accepted point with half the step
                scale *= 0.5
                S, Y = [], []
                continue
            y = new["g"] - cur["g"]
            if float(y @ step) > 1e-14:
                S.append(step)
                Y.append(y)
                S, Y = S[-LBFGS_HISTORY:], Y[-LBFGS_HISTORY:]
            scale = min(1.0, 2.0 * scale)
            cur = new
            converged = gmax < tol_g and abs(dE) < self.conv_tol
        return cur, it, converged

    def _lowest_curvature(self, cur):
        """Lowest eigenpair of the orbital Hessian of E(C) = min_ci E(C, ci) at `cur`.  H v is the central difference of the
        gradient at C exp(+-d v) (two probes, CI re-solved in each, so the CI's relaxation is in H); the probes move no orbitals
        and are counted in `stability_evaluations`, not as macro iterations."""
        ncore, nc = self.ncore, self.ncas
        d = float(self.stability_probe)

        def hv(v):
            gp = self._macro(rotate(cur["mo"], d * v, ncore, nc), cur["ci"])["g"]
            gm = self._macro(rotate(cur["mo"], -d * v, ncore, nc), cur["ci"])["g"]
            self.stability_evaluations += 2
            return (gp - gm) / (2.0 * d)

        return lowest_eigenpair(hv, cur["hdiag"], below=-self.stability_tol)

    def _leave_saddle(self, cur, it, v):
        """Step along +-v (zero gradient, negative curvature), the largest element `max_stepsize` and halved until the energy
        falls: (new accepted point, macro iterations so far, True), or (`cur`, ..., False) if no such step lowers the energy."""
        ncore, nc = self.ncore, self.ncas
        t = self.max_stepsize / float(np.abs(v).max())
        while t * float(np.abs(v).max()) >= float(self.stability_probe) and it < int(self.max_cycle_macro):
            for sign in (1.0, -1.0):
                new = self._macro(rotate(cur["mo"], sign * t * v, ncore, nc), cur["ci"])
                it += 1
                dE = new["e_tot"] - cur["e_tot"]
                self._log(4, f"CASSCF macro {it}: E = {new['e_tot']:.12f}  dE = {dE:.3e}  leaving a saddle, max|step| = "
                             f"{t * np.abs(v).max():.3e}")
                if dE < -RISE_NOISE:
                    return new, it, True
            t *= 0.5
        return cur, it, False

    mc1step = mc2step = kernel

    def _finish(self, cur, converged, nmo):
        """Final orbitals: core and virtual blocks diagonalise F^I + F^A within the block, the active block keeps the optimised
        orbitals (or becomes natural orbitals, occupations descending, with the CI solved again in them as CASCI does)."""
        mf = self._scf
        ncore, nc = self.ncore, self.ncas
        nocc = ncore + nc
        act = slice(ncore, nocc)
        mo = cur["mo"].copy()
        Fao = cur["fock_ao"].cpu().numpy()
        for blk in (slice(0, ncore), slice(nocc, nmo)):
            if blk.stop - blk.start > 0:
                fb = mo[:, blk].T @ Fao @ mo[:, blk]
                _, U = np.linalg.eigh(0.5 * (fb + fb.T))
                mo[:, blk] = mo[:, blk] @ U
        e_tot, ci, e_states, gamma = cur["e_tot"], cur["ci"], cur["e_states"], cur["gamma"]
        ci_ok = cur["ci_converged"]
        sol = self.fcisolver
        # occupations of the optimised orbitals: the diagonal of the solver's own `make_rdm1` of the returned vector(s)
        if self.weights is None:
            occ = np.diag(sol.make_rdm1(ci, nc, self.nelecas)).copy()
        else:
            occ = sum(w * np.diag(sol.make_rdm1(c, nc, self.nelecas)) for w, c in zip(self.weights, ci))
        if self.natorb:
            w, U = np.linalg.eigh(-gamma)
            U = U * np.where(U[np.abs(U).argmax(axis=0), np.arange(nc)] < 0, -1.0, 1.0)[None, :]
            mo[:, act] = mo[:, act] @ U
            h_act = U.T @ cur["h_act"] @ U
            eri = np.einsum("pqrs,pt,qu,rv,sw->tuvw", cur["eri"], U, U, U, U, optimize=True)
            e, ci = sol.kernel(h_act, eri, nc, self.nelecas, ecore=cur["e_core"])
            ci_ok = bool(np.all(sol.converged))
            if self.weights is None:
                e_tot = float(e)
            else:
                ci = ci if isinstance(ci, list) else [ci]
                e_states = np.atleast_1d(np.asarray(e, dtype=np.float64)).copy()
                e_tot = float(self.weights @ e_states)
            occ = -w
        mo_occ = np.zeros(nmo)
        mo_occ[:ncore] = 2.0
        mo_occ[act] = occ
        self.e_tot, self.e_core, self.e_cas = e_tot, cur["e_core"], e_tot - cur["e_core"]
        self.e_states = e_states
        self.ci = ci
        self.mo_coeff, self.mo_occ = mo, mo_occ
        self.mo_energy = np.einsum("pi,pq,qi->i", mo, Fao, mo)
        self.converged = bool(converged and ci_ok)
        self._log(3, f"CASSCF {'converged' if self.converged else 'NOT converged'} in {self.macro_iterations} macro iterations: "
                     f"E = {e_tot:.12f}  E(CAS) = {self.e_cas:.12f}")
        return self.e_tot, self.e_cas, self.ci, self.mo_coeff, self.mo_energy

    def make_rdm1(self, mo_coeff=None, ci=None, state=None):
        """Total AO density matrix: of one state, or (state-averaged object, `state` None) the weighted average."""
        if self.ci is None and ci is None:
            self.kernel()
        if self.weights is None or state is not None:
            return super().make_rdm1(mo_coeff, ci, state or 0)
        return sum(w * super(CASSCF, self).make_rdm1(mo_coeff, ci, s) for s, w in enumerate(self.weights))
