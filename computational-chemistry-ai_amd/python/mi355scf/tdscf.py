"""Closed-shell linear response: TDA (CIS) and full TDHF / TDDFT (RPA), singlets and triplets, behind `pyscf.tdscf` /
`gpu4pyscf.tdscf` (templates/calculate_uv_spectrum.py: `tdscf.TDDFT(mf)`, `td.kernel()`, `td.analyze()`,
`td.oscillator_strength()`, `td.xy`).

Trial vectors x [nocc, nvir] enter the AO basis as D_x = C_o x C_v^T, split into D_s = (D_x + D_x^T)/2 and
D_a = (D_x - D_x^T)/2.  All J/K of one Davidson iteration go through one `Engine.get_jk_multi` call (every resident ERI tile
read once per launch of up to 8 densities by default, 16 at most).  The XC response dV[D_s] is analytic: per grid point the
second derivatives of the functional at the ground-state density (`Engine.xc_fxc_prep`, once per run), then per batch of trial
vectors rho1 from one batched D_s.ao GEMM, the linearised potential (`Engine.xc_fxc_apply`) and the SCF's V_xc fold.
`xc_response = "fd"` keeps the central difference of the XC potential as the independent check.

  A x     = de x + [2 J[D_x] - c_x K[D_x] + 2 dV_S[D_s]]_ov            (triplet: [-c_x K[D_x] + 2 dV_T[D_s]]_ov)
  (A+B) t = de t + [4 J[D_s] - 2 c_x K[D_s] + 4 dV_S[D_s]]_ov          (triplet: [-2 c_x K[D_s] + 4 dV_T[D_s]]_ov)
  (A-B) t = de t - 2 c_x [K[D_a]]_ov

  dV_S[M] = d/dh V_a(D_a = D_b = (D0 + h M)/2) = d/dh V_xc,RKS(D0 + h M),  dV_T[M] = d/dh V_a(D_a = (D0 + h M)/2, D_b = (D0 - h M)/2)

Range-separated hybrids (CAM-B3LYP): every c_x K above is hyb K + (alpha - hyb) K_LR (dft.rsh_coeff), K_LR from the same batched
K-only passes over the SCF object's long-range store (dft.lr_engine).

Outputs follow PySCF: `e` ascending in Hartree, `xy[n] = (X, Y)` of shape [nocc, nvir] with X.X - Y.Y = 1/2, oscillator
strengths f = 2/3 w |2 sum_ia (X+Y)_ia <i|r|a>|^2 (length gauge).
"""
import sys
import time
import warnings

import numpy as np
import torch

from .ao2mo import resident_engine
from .reference import require

HARTREE2EV = 27.211386245988
HARTREE2NM = 45.56335252907954   # nm * Hartree: lambda = 45.563... / E
# Batches of symmetric densities below this size take the looped single-density build: measured per density on
# benzene/cc-pVTZ (4.9 GB store), looped vs batched 1.00 vs 1.79 ms at n = 1, 0.89 vs 0.91 at 2, 0.90 vs 0.67 at 4.
# Antisymmetric densities always need the batched kernel (the single-density one assumes D = D^T).
JK_MULTI_MIN = 4


# =================================================================================================
# Davidson solvers (torch: CPU tensors or device tensors)
# =================================================================================================
def initial_guess(diag, nstates, tol=1e-5):
    """Unit vectors on the `nstates` lowest diagonal elements, plus every further element degenerate (within `tol`) with the
    last one, so that a degenerate pair is never split by the guess."""
    order = torch.argsort(diag)
    n = min(nstates, diag.numel())
    last = diag[order[n - 1]]
    while n < diag.numel() and abs(float(diag[order[n]] - last)) < tol:
        n += 1
    V = torch.zeros(n, diag.numel(), dtype=diag.dtype, device=diag.device)
    V[torch.arange(n), order[:n]] = 1.0
    return V


def _orthonormal_add(V, new, lindep=1e-12):
    """Rows of `new` orthogonalised against V (two Gram-Schmidt passes) and each other; near-dependent rows dropped."""
    basis = V
    for r in new:
        for _ in range(2):
            if basis is not None and basis.shape[0]:
                r = r - basis.T @ (basis @ r)
        nr = torch.linalg.norm(r)
        if nr > lindep:
            r = (r / nr).unsqueeze(0)
            basis = r if basis is None else torch.cat([basis, r])
    return basis


def davidson_tda(matvec, diag, nstates, conv_tol=1e-9, max_cycle=100, max_space=None, guess=None, log=None):
    """Lowest `nstates` eigenpairs of a symmetric operator given by `matvec(V[m, n]) -> A V^T as [m, n]`.
    Returns (w [nstates], X [nstates, n], converged [nstates] bool)."""
    dim = diag.numel()
    nstates = min(nstates, dim)
    max_space = max_space or max(40, 12 * nstates)
    V = _orthonormal_add(None, guess if guess is not None else initial_guess(diag, nstates))
    AV = matvec(V)
    w_old = None
    conv = torch.zeros(nstates, dtype=torch.bool)
    for it in range(max_cycle):
        H = V @ AV.T
        H = 0.5 * (H + H.T)
        e, c = torch.linalg.eigh(H)
        w, c = e[:nstates], c[:, :nstates]
        X = c.T @ V
        R = c.T @ AV - w[:, None] * X
        rn = torch.linalg.norm(R, dim=1)
        dw = torch.full_like(w, float("inf")) if w_old is None or w_old.numel() != w.numel() else (w - w_old).abs()
        conv = ((rn < conv_tol ** 0.5) & (dw < conv_tol)).cpu() | (V.shape[0] >= dim)
        if log:
            log(f"TDA Davidson it {it}: space {V.shape[0]}, max |r| {float(rn.max()):.3e}, converged {int(conv.sum())}/{nstates}")
        if bool(conv.all()):
            break
        w_old = w
        todo = ~conv.to(R.device)
        denom = diag[None, :] - w[todo, None]
        denom = torch.where(denom.abs() < 1e-8, torch.full_like(denom, 1e-8), denom)
        T = R[todo] / denom
        if V.shape[0] + T.shape[0] > max_space:   # restart from the Ritz vectors
            V = _orthonormal_add(None, X)
            AV = c.T @ AV
        Vn = _orthonormal_add(V, T)
        if Vn.shape[0] == V.shape[0]:
            break
        AV = torch.cat([AV, matvec(Vn[V.shape[0]:])])
        V = Vn
    return w, X, conv


def davidson_rpa(apb, amb, diag, nstates, conv_tol=1e-9, max_cycle=100, max_space=None, guess=None, log=None):
    """Lowest positive roots of [[A, B], [-B, -A]] from the products apb(V) = (A+B) V^T and amb(V) = (A-B) V^T (rows).
    One orthonormal trial space for both; the projected problem (A-B)(A+B) u = w^2 u is solved through the Cholesky factor
    of the projected A-B (positive definite for a stable reference).  Returns (w, X, Y, converged)."""
    dim = diag.numel()
    nstates = min(nstates, dim)
    max_space = max_space or max(40, 12 * nstates)
    V = _orthonormal_add(None, guess if guess is not None else initial_guess(diag, nstates))
    PV, MV = apb(V), amb(V)
    w_old = None
    warned = False
    for it in range(max_cycle):
        P = V @ PV.T
        M = V @ MV.T
        P, M = 0.5 * (P + P.T), 0.5 * (M + M.T)
        L = torch.linalg.cholesky(M)
        e2, z = torch.linalg.eigh(L.T @ P @ L)
        pos = e2 > 0
        if not bool(pos.all()) and not warned:
            warnings.warn("TDHF/TDDFT: non-positive RPA roots dropped (unstable reference)")
            warned = True
        e2, z = e2[pos], z[:, pos]
        k = min(nstates, e2.numel())
        w = torch.sqrt(e2[:k])
        u = L @ z[:, :k]                 # subspace coefficients of X+Y
        v = (P @ u) / w[None, :]          # of X-Y
        XpY, XmY = u.T @ V, v.T @ V
        R1 = u.T @ PV - w[:, None] * XmY
        R2 = v.T @ MV - w[:, None] * XpY
        rn = torch.sqrt(torch.linalg.norm(R1, dim=1) ** 2 + torch.linalg.norm(R2, dim=1) ** 2)
        dw = torch.full_like(w, float("inf")) if w_old is None or w_old.numel() != w.numel() else (w - w_old).abs()
        conv = ((rn < conv_tol ** 0.5) & (dw < conv_tol)).cpu() | (V.shape[0] >= dim)
        if log:
            log(f"RPA Davidson it {it}: space {V.shape[0]}, max |r| {float(rn.max()):.3e}, converged {int(conv.sum())}/{k}")
        if bool(conv.all()) and k == nstates or V.shape[0] >= dim:
            break
        w_old = w
        todo = ~conv.to(R1.device)
        denom = diag[None, :] - w[todo, None]
        denom = torch.where(denom.abs() < 1e-8, torch.full_like(denom, 1e-8), denom)
        T = torch.cat([R1[todo] / denom, R2[todo] / denom])
        if V.shape[0] + T.shape[0] > max_space:
            V = _orthonormal_add(None, torch.cat([XpY, XmY]))
            PV, MV = apb(V), amb(V)
        Vn = _orthonormal_add(V, T)
        if Vn.shape[0] == V.shape[0]:
            break
        new = Vn[V.shape[0]:]
        PV, MV = torch.cat([PV, apb(new)]), torch.cat([MV, amb(new)])
        V = Vn
    # X.X - Y.Y = (X+Y).(X-Y) = 1/2
    s = (XpY * XmY).sum(dim=1)
    scale = torch.sqrt(0.5 / s)
    XpY, XmY = XpY * scale[:, None], XmY * scale[:, None]
    conv = conv[:k] if conv.numel() >= k else torch.ones(k, dtype=torch.bool)
    return w, 0.5 * (XpY + XmY), 0.5 * (XpY - XmY), conv


def oscillator_strengths(e, xy, dip_ov, singlet=True):
    """f_n = 2/3 w_n |mu_0n|^2 with mu_0n = 2 sum_ia (X+Y)_ia <i|r|a> (states normalised to X.X - Y.Y = 1/2).
    `dip_ov`: [3, nocc, nvir] dipole integrals between occupied and virtual orbitals.  Triplets are dark."""
    dip_ov = np.asarray(dip_ov)
    if not singlet:
        return np.zeros(len(e))
    tdm = np.array([2.0 * np.einsum("xia,ia->x", dip_ov, np.asarray(x) + np.asarray(y)) for x, y in xy]).reshape(-1, 3)
    return 2.0 / 3.0 * np.asarray(e) * (tdm ** 2).sum(axis=1)


# =================================================================================================
# Response classes
# =================================================================================================
class _TDBase:
    nstates = 3
    singlet = True
    conv_tol = 1e-5
    max_cycle = 100
    max_space = None
    fd_step = 1e-4            # step of the central difference of the XC potential (xc_response = "fd")
    xc_response = "analytic"  # "analytic": fxc kernels (Engine.xc_fxc_prep / xc_fxc_apply); "fd": central difference of V_xc
    xc_rho_batch_bytes = 2e9  # bound on the D_s.ao0 products [m, nao, ng] formed by one batched GEMM

    def __init__(self, mf):
        from .dft import parse_xc, rsh_coeff
        xc = require(mf, "TDA/TDDFT").xc
        self._omega, self._alpha = 0.0, 0.0
        if xc is None:
            self._hyb, self._dft = 1.0, False
        else:
            hyb, _, level = parse_xc(xc)
            if level >= 2:
                raise NotImplementedError(f"TDDFT: the meta-GGA kernel of {xc} is not supported")
            self._hyb, self._dft = float(hyb), True
            omega, alpha, _h = rsh_coeff(xc)
            if omega != 0.0:           # exact exchange hyb K + (alpha - hyb) K_LR
                self._omega, self._alpha = float(omega), float(alpha)
        self._scf = mf
        self.verbose = mf.verbose
        self.stdout = getattr(mf, "stdout", None) or sys.stdout
        self.e = self.xy = self.converged = None
        self.nstates = type(self).nstates
        self.stats = {}
        self._fxc = None

    @property
    def mol(self):
        return self._scf.mol

    def _log(self, level, msg):
        if self.verbose >= level:
            (self.stdout or sys.stdout).write(msg + "\n")

    def _setup(self):
        mf = self._scf
        if mf.mo_coeff is None:
            mf.kernel()
        eng = resident_engine(mf, "TDA/TDDFT")
        if self._omega != 0.0:
            from .dft import check_rsh_scf
            check_rsh_scf(mf)
        dev = eng.device
        occ = np.asarray(mf.mo_occ)
        C = torch.as_tensor(np.asarray(mf.mo_coeff), dtype=torch.float64, device=dev)
        eps = torch.as_tensor(np.asarray(mf.mo_energy), dtype=torch.float64, device=dev)
        self._nocc = int((occ > 0).sum())
        self._Co, self._Cv = C[:, :self._nocc], C[:, self._nocc:]
        self._nvir = self._Cv.shape[1]
        self._de = (eps[None, self._nocc:] - eps[:self._nocc, None]).reshape(-1)
        if self._dft:
            self._D0 = torch.as_tensor(np.asarray(mf.make_rdm1()), dtype=torch.float64, device=dev)
        self._fxc = None
        self.stats = {"n_jk_densities": 0, "n_matvec": 0}

    # --- AO-basis pieces -------------------------------------------------------------------------
    def _ao(self, V):
        """Rows [m, nov] -> D_x [m, N, N] = C_o x C_v^T."""
        x = V.reshape(-1, self._nocc, self._nvir)
        return self._Co @ x @ self._Cv.T

    def _ov(self, M):
        """[m, N, N] -> rows [m, nov] of C_o^T M C_v."""
        return (self._Co.T @ M @ self._Cv).reshape(M.shape[0], -1)

    def _jk(self, dms, sym, with_j, with_k=True):
        """J, K of the batch; for a range-separated hybrid K is already K_eff = hyb K + (alpha - hyb) K_LR (the long-range K
        from the same batch over the long-range store)."""
        self.stats["n_jk_densities"] += dms.shape[0]
        J, K = self._jk_one(self._scf.engine, dms, sym, with_j, with_k)
        if with_k and self._omega != 0.0:
            from .dft import lr_engine
            _j, Klr = self._jk_one(lr_engine(self._scf), dms, sym, False, True)
            K = self._hyb * K + (self._alpha - self._hyb) * Klr
        return J, K

    @staticmethod
    def _jk_one(eng, dms, sym, with_j, with_k):
        if all(s > 0 for s in sym) and len(sym) < JK_MULTI_MIN:
            return eng.get_jk(dms, with_j, with_k)     # few symmetric densities: the single-density kernel is faster
        return eng.get_jk_multi(dms, sym, with_j=with_j, with_k=with_k)

    def _dvxc(self, Ds, triplet=False):
        """XC response at h = 0 for each symmetric M of Ds [m, N, N]: dV_S[M] = d/dh Vxc_RKS(D0 + h M) (singlet), or
        dV_T[M] = d/dh V_alpha(D_a = (D0 + h M)/2, D_b = (D0 - h M)/2) (triplet).  Analytic, or with xc_response = "fd" the
        central difference (step fd_step / max|M|).  A functional without semilocal terms (xc = "HF") gives zero."""
        from .dft import parse_xc
        t0 = time.perf_counter()
        if not parse_xc(self._scf.xc)[1]:
            out = torch.zeros_like(Ds)
        elif self.xc_response == "analytic":
            out = self._dvxc_analytic(Ds, triplet)
        elif self.xc_response == "fd":
            out = self._dvxc_fd(Ds, triplet)
        else:
            raise ValueError(f"xc_response must be 'analytic' or 'fd', not {self.xc_response!r}")
        if out.is_cuda:
            torch.cuda.synchronize(out.device)
        self.stats["xc_seconds"] = self.stats.get("xc_seconds", 0.0) + time.perf_counter() - t0
        self.stats["xc_vectors"] = self.stats.get("xc_vectors", 0) + Ds.shape[0]
        return out

    def _dvxc_fd(self, Ds, triplet):
        mf = self._scf
        out = torch.empty_like(Ds)
        for m in range(Ds.shape[0]):
            M = Ds[m]
            h = self.fd_step / max(float(M.abs().max()), 1e-300)
            if triplet:
                Dp, Dm = 0.5 * (self._D0 + h * M), 0.5 * (self._D0 - h * M)
                vp, vm = self._vxc_alpha(Dp, Dm), self._vxc_alpha(Dm, Dp)
            else:
                vp = mf.nr_rks(self._D0 + h * M)[2]
                vm = mf.nr_rks(self._D0 - h * M)[2]
            out[m] = (vp - vm) / (2.0 * h)
        return out

    def _vxc_alpha(self, Da, Db):
        """V_xc of spin alpha of the spin densities (Da, Db) on the SCF's grid: the SCF's block body (dft.KSMixin) with the
        spin-polarised functional, of which only the alpha matrix is folded."""
        mf = self._scf
        xcf = mf._xc_functional()
        gga = xcf[2]
        vmat = torch.zeros_like(Da)
        for w, ao in mf._ao_blocks(gga):
            dens = [mf._block_density(ao, dm, None, gga) for dm in (Da, Db)]
            _e, (wva, _wvb) = mf._block_functional(xcf, [d[0] for d in dens], [d[1] for d in dens], w)
            mf._block_vmat(ao, wva, gga, vmat)
        return vmat + vmat.T

    def _fxc_blocks(self, triplet):
        """[(rho0, coef)] per grid block: the ground-state density and its XC kernel coefficients for the channel, made once
        per run (Engine.xc_fxc_prep)."""
        if self._fxc is None or self._fxc[0] != bool(triplet):
            mf = self._scf
            eng = mf.engine
            _hyb, terms, gga, params = mf._xc_functional()
            blocks = []
            for w, ao in mf._ao_blocks(gga):
                rho0, _tau = mf._block_density(ao, self._D0, None, gga)
                blocks.append((rho0, eng.xc_fxc_prep(terms, rho0, w, gga, triplet=triplet, params=params)))
            self._fxc = (bool(triplet), blocks)
        return self._fxc[1]

    def _dvxc_analytic(self, Ds, triplet):
        """Per grid block: C = Ds.ao0 for as many vectors as xc_rho_batch_bytes allows (one batched GEMM), rho1 of each, wv1
        of the whole batch in one launch, then the V_xc fold (xc_aow + xc_vmat) of each vector."""
        from .dft import parse_xc
        mf = self._scf
        eng = mf.engine
        gga = parse_xc(mf.xc)[2]
        deriv, nc = (1, 4) if gga else (0, 1)
        m, n = Ds.shape[0], Ds.shape[1]
        vmat = torch.zeros_like(Ds)
        for (w, ao), (rho0, coef) in zip(mf._ao_blocks(gga), self._fxc_blocks(triplet)):
            ng = ao.shape[-1]
            mc = max(1, min(m, int(self.xc_rho_batch_bytes // (8.0 * n * ng))))
            for j0 in range(0, m, mc):
                j1 = min(j0 + mc, m)
                C = torch.matmul(Ds[j0:j1], ao[0])
                rho1 = torch.empty(j1 - j0, nc, ng, dtype=torch.float64, device=Ds.device)
                for j in range(j1 - j0):
                    eng.xc_rho(ao, C[j], deriv, out=rho1[j])
                del C
                wv1 = eng.xc_fxc_apply(rho0, coef, rho1, gga)
                for j in range(j1 - j0):
                    eng.xc_vmat(ao[0], eng.xc_aow(ao, wv1[j], gga), vmat[j0 + j])
        return vmat + vmat.transpose(1, 2)

    def _need_k(self):
        return abs(self._hyb) > 1e-12 or self._alpha != 0.0

    def _kx(self):
        """Factor of K in the products: c_x of a global hybrid, 1 for a range-separated one (K is K_eff already, see _jk)."""
        return 1.0 if self._omega != 0.0 else self._hyb

    # --- products --------------------------------------------------------------------------------
    def _tda_matvec(self, V):
        self.stats["n_matvec"] += V.shape[0]
        Dx = self._ao(V)
        Ds, Da = 0.5 * (Dx + Dx.transpose(1, 2)), 0.5 * (Dx - Dx.transpose(1, 2))
        m = V.shape[0]
        cx = self._kx()
        out = self._de[None, :] * V
        if self._need_k():
            J, K = self._jk(torch.cat([Ds, Da]), [1] * m + [-1] * m, with_j=self.singlet)
            F = -cx * (K[:m] + K[m:])
            if self.singlet:
                F = F + 2.0 * J[:m]
        elif self.singlet:
            J, _ = self._jk(Ds, [1] * m, with_j=True, with_k=False)   # pure functional: no exchange
            F = 2.0 * J
        else:
            F = torch.zeros_like(Ds)                                  # triplet of a pure functional: neither J nor K
        if self._dft:
            F = F + 2.0 * self._dvxc(Ds, triplet=not self.singlet)
        return out + self._ov(F)

    def _rpa_products(self, V):
        """((A+B) V^T, (A-B) V^T) as rows, all J/K in one batched call."""
        self.stats["n_matvec"] += V.shape[0]
        Dx = self._ao(V)
        Ds, Da = 0.5 * (Dx + Dx.transpose(1, 2)), 0.5 * (Dx - Dx.transpose(1, 2))
        m = V.shape[0]
        cx = self._kx()
        apb = self._de[None, :] * V
        amb = self._de[None, :] * V
        if self._need_k():
            J, K = self._jk(torch.cat([Ds, Da]), [1] * m + [-1] * m, with_j=self.singlet)
            F = -2.0 * cx * K[:m]
            if self.singlet:
                F = F + 4.0 * J[:m]
            amb = amb - 2.0 * cx * self._ov(K[m:])
        elif self.singlet:
            J, _ = self._jk(Ds, [1] * m, with_j=True, with_k=False)   # pure functional: no exchange
            F = 4.0 * J
        else:
            F = torch.zeros_like(Ds)
        if self._dft:
            F = F + 4.0 * self._dvxc(Ds, triplet=not self.singlet)
        return apb + self._ov(F), amb

    # --- properties ------------------------------------------------------------------------------
    def _dip_ov(self):
        eng = self._scf.engine
        dip = eng.int1e(with_dipole=True)[3]
        return (self._Co.T @ dip @ self._Cv).cpu().numpy()

    def transition_dipole(self):
        """<0|r|n> (a.u.) for every state: 2 sum_ia (X+Y)_ia <i|r|a>; zero for triplets."""
        if self.xy is None:
            self.kernel()
        if not self.singlet:
            return np.zeros((len(self.e), 3))
        d = self._dip_ov()
        return np.array([2.0 * np.einsum("xia,ia->x", d, x + y) for x, y in self.xy]).reshape(-1, 3)

    def oscillator_strength(self, gauge="length", **kw):
        if gauge != "length":
            raise NotImplementedError("oscillator_strength: only the length gauge is implemented")
        if self.xy is None:
            self.kernel()
        return oscillator_strengths(self.e, self.xy, self._dip_ov(), self.singlet)

    def analyze(self, verbose=None):
        verbose = self.verbose if verbose is None else verbose
        if self.xy is None:
            self.kernel()
        f = self.oscillator_strength()
        if verbose < 1:
            return self
        mult = "Singlet" if self.singlet else "Triplet"
        out = self.stdout or sys.stdout
        for n, (w, (x, y)) in enumerate(zip(self.e, self.xy)):
            out.write(f"Excited State {n + 1:3d}: {mult} {w * HARTREE2EV:10.5f} eV {HARTREE2NM / w:9.2f} nm  f={f[n]:.4f}\n")
            if verbose >= 3:
                for i, a in zip(*np.nonzero(np.abs(x) > 0.1)):
                    out.write(f"    {i + 1:4d} -> {a + self._nocc + 1:4d} {x[i, a]:12.5f}\n")
        return self

    def _guess(self, x0):
        """Trial vectors [m, nov] from `x0` (a previous `td.xy`, or arrays [m, nocc, nvir]): X of every state and Y where it is
        not zero.  None when x0 is None or does not fit the current orbital spaces (the default unit-vector guess is used)."""
        if x0 is None:
            return None
        rows = []
        for item in x0:
            parts = item if isinstance(item, (tuple, list)) else (item,)
            for p in parts:
                p = np.asarray(p, dtype=np.float64)
                if p.size != self._nocc * self._nvir:
                    return None
                if np.abs(p).max() > 0.0:
                    rows.append(p.ravel())
        if not rows:
            return None
        V = torch.as_tensor(np.array(rows), dtype=torch.float64, device=self._de.device)
        if V.shape[0] < min(int(self.nstates), self._de.numel()):      # fewer vectors than roots: topped up with unit vectors
            V = torch.cat([V, initial_guess(self._de, int(self.nstates))])
        return V

    # --- nuclear gradients (tdscf_grad.py) ----------------------------------------------------------
    def nuc_grad_method(self):
        from .tdscf_grad import Gradients
        return Gradients(self)

    Gradients = nuc_grad_method

    def _finish(self, w, X, Y, conv):
        no, nv = self._nocc, self._nvir
        self.e = w.cpu().numpy()
        Xn = X.cpu().numpy().reshape(-1, no, nv)
        Yn = np.zeros_like(Xn) if Y is None else Y.cpu().numpy().reshape(-1, no, nv)
        self.xy = [(Xn[n], Yn[n]) for n in range(len(self.e))]
        self.converged = np.asarray(conv.cpu().numpy()[:len(self.e)], dtype=bool)
        if not self.converged.all():
            self._log(1, f"{type(self).__name__}: {int((~self.converged).sum())} root(s) not converged")
        return self.e, self.xy


class TDA(_TDBase):
    """Tamm-Dancoff approximation (CIS for an RHF reference)."""

    def kernel(self, nstates=None, x0=None):
        if nstates is not None:
            self.nstates = nstates
        self._setup()
        dim = self._nocc * self._nvir
        n = min(int(self.nstates), dim)
        self.nstates = n
        w, X, conv = davidson_tda(self._tda_matvec, self._de, n, self.conv_tol, self.max_cycle, self.max_space,
                                  guess=self._guess(x0), log=(lambda s: self._log(4, s)))
        # X.X = 1/2 (PySCF's normalisation of restricted states)
        X = X * np.sqrt(0.5)
        return self._finish(w, X, None, conv)


class TDHF(_TDBase):
    """Full linear response (RPA): TDHF for an RHF reference, TDDFT for an RKS one."""

    def kernel(self, nstates=None, x0=None):
        if nstates is not None:
            self.nstates = nstates
        self._setup()
        dim = self._nocc * self._nvir
        n = min(int(self.nstates), dim)
        self.nstates = n
        cache = {}

        def apb(V):
            P, M = self._rpa_products(V)
            cache[id(V)] = M
            return P

        def amb(V):
            M = cache.pop(id(V), None)
            return M if M is not None else self._rpa_products(V)[1]

        w, X, Y, conv = davidson_rpa(apb, amb, self._de, n, self.conv_tol, self.max_cycle, self.max_space,
                                     guess=self._guess(x0), log=(lambda s: self._log(4, s)))
        return self._finish(w, X, Y, conv)


TDDFT = TDHF
RPA = TDHF
CIS = TDA
