"""Analytic nuclear gradients of closed-shell singlet TDA / TDHF / TDDFT excited states behind `td.nuc_grad_method()`
(`tdscf.TDA`, `tdscf.TDHF`), in the Z-vector formulation of Furche and Ahlrichs, J. Chem. Phys. 117, 7433 (2002).

With u = X + Y, v = X - Y ([nocc, nvir], u.v = 1/2 as `td.xy` is normalised; TDA: u = v = X) the excitation energy is

    w = sum_ia de_ia (u_ia^2 + v_ia^2) + 4 (U|U) - 2 c_x ex(U, U) - 2 c_x ex(V, V) + 4 tr(U dV[U])

    U = sym(C_o u C_v^T),  V = asym(C_o v C_v^T),  ex(A, B) = sum_ijkl (ik|jl) A_ij B_kl,  dV[M] = d/dh V_xc(D0 + h M)

(`tdscf.py`: (A+B), (A-B)).  E_SCF + w is made stationary in the orbitals by the Lagrangian multipliers Z (occupied-virtual
rotations) and W (orthonormality).  In the order of `relaxed_state`:

  1. T = C_o doo C_o^T + C_v dvv C_v^T, doo = -(u u^T + v v^T), dvv = u^T u + v^T v: the unrelaxed difference density (tr = 0).
  2. H+[T] = 2 J[T] - c_x K[T] + 2 dV[T] + 8 d2V[U, U],  H+[U] = 4 J[U] - 2 c_x K[U] + 4 dV[U],  H-[V] = 2 c_x K[V]
     (d2V[M, M] = d2/dh2 V_xc(D0 + h M): the third derivative of the functional, `third_order`), one batched J/K pass;
     R_ia = 2 H+[T]_ia - 2 (H+[U]_oo u)_ia + 2 (u H+[U]_vv)_ia - 2 (H-[V]_oo v)_ia + 2 (v H-[V]_vv)_ia.
  3. (A+B) z = -R by preconditioned conjugate gradients (`solve_z`), Z = sym(C_o z C_v^T).
  4. P = T + Z (relaxed difference density), W (energy-weighted density, ground state included).
  5. one-electron part: `mi_grad_1e` of (D0 + P, W).
  6. two-electron part, with D = D0 + P completing the square of the cross terms (`two_particle_terms`):

         E2 = [1/2 (D|D) - c_x/4 ex(D, D)] - 1/2 (P|P) + 4 (U|U) + c_x/4 ex(P, P) - 2 c_x ex(U, U) - 2 c_x ex(V, V)

     ONE pass of `mi_grad_eri_xpairs` (pairs Q = (P, U), s = (-1, 8); exchange pairs R = (P, U, V), t = c_x (1/4, -2, -2),
     sym = (+1, +1, -1)).  `algorithm = "loop"` evaluates the same terms one per pass: the plain kernel for the bracket and for
     every symmetric matrix (ex(R, R) = -4 [g(R, hyb = 1) - g(R, hyb = 0)]), and, because no older entry point takes an
     antisymmetric matrix, one exchange-pair call with D = 0 for V alone.
  7. XC part (no grid-weight response, as the ground-state gradient): with f(M; wv) = int wv . d rho_M / dR (`grad._add_xc_force`)
         f(D0 + P; wv0) + f(D0; wv1[P] + 4 wv2[U, U]) + 8 f(U; wv1[U]),
     wv0 the ground-state potential, wv1[M] = f_xc rho_M (`xc_fxc_apply`), wv2 the third-order term.
  8. third order: wv2[U, U] = (wv1_{rho0 + e rho_U}[U] - wv1_{rho0 - e rho_U}[U]) / (2 e), e = `xc3_step` / max |U|.

Refused (NotImplementedError): triplets, the references of row "TDA/TDDFT gradients" of `reference.SUPPORT`, sharded or direct-mode
engines, a state above nstates, unconverged roots.
"""
import time
import warnings

import numpy as np
import torch

from .grad import _GradScanner, _add_xc_force, assemble, log_gradient, xc_force
from .reference import require

ALGORITHMS = ("onepass", "loop")
FOLLOW_MIN_OVERLAP = 0.7   # the scanner warns when the followed state overlaps the previous one by less than this


# ---- plain algebra (NumPy in, NumPy out) ------------------------------------------------------------------------------------------
def difference_density(x, y):
    """(doo, dvv) of the unrelaxed difference density T from X, Y [nocc, nvir] normalised to X.X - Y.Y = 1/2:
    doo = -(u u^T + v v^T), dvv = u^T u + v^T v with u = X + Y, v = X - Y; tr doo + tr dvv = 0, tr dvv = 2 (X.X + Y.Y)."""
    u, v = np.asarray(x) + np.asarray(y), np.asarray(x) - np.asarray(y)
    return -(u @ u.T + v @ v.T), u.T @ u + v.T @ v


def two_particle_terms(D0, P, U, V, hyb):
    """(D, Q, s, R, t, sym) of `Engine.grad_eri(D, hyb, g, pairs=(Q, s), xpairs=(R, t, sym))` for the two-particle density of an
    excited state: ground-state density D0, relaxed difference density P, U = sym(X+Y), V = asym(X-Y) (AO matrices).

        1/2 (D0|D0) - hyb/4 ex(D0, D0) + (P|D0) - hyb/2 ex(P, D0) + 4 (U|U) - 2 hyb ex(U, U) - 2 hyb ex(V, V)
      = [1/2 (D|D) - hyb/4 ex(D, D)]_{D = D0 + P} - 1/2 (P|P) + 4 (U|U) + hyb/4 ex(P, P) - 2 hyb ex(U, U) - 2 hyb ex(V, V)

    hyb = 0: no exchange term."""
    D0, P, U, V = (np.asarray(a, dtype=np.float64) for a in (D0, P, U, V))
    D = D0 + P
    Q, s = np.stack([P, U]), np.array([-1.0, 8.0])
    if hyb == 0.0:
        n = D0.shape[0]
        return D, Q, s, np.zeros((0, n, n)), np.zeros(0), np.zeros(0, dtype=np.intc)
    R = np.stack([P, U, V])
    t = hyb * np.array([0.25, -2.0, -2.0])
    return D, Q, s, R, t, np.array([1, 1, -1], dtype=np.intc)


# ---- device algebra (torch; `td` supplies _Co, _Cv, _jk, _dvxc, _ao, _ov) ------------------------------------------------------------
def _sym(M):
    return 0.5 * (M + M.transpose(-1, -2))


def _apb(td, V):
    """(A+B) V^T as rows: only the symmetric part of the trial densities enters (no K of the antisymmetric part, which the
    Davidson's `_rpa_products` builds for A-B)."""
    Ds = _sym(td._ao(V))
    m = V.shape[0]
    out = td._de[None, :] * V
    if td._need_k():
        J, K = td._jk(Ds, [1] * m, with_j=True)
        F = 4.0 * J - 2.0 * td._kx() * K
    else:
        J, _ = td._jk(Ds, [1] * m, with_j=True, with_k=False)
        F = 4.0 * J
    if td._dft:
        F = F + 4.0 * td._dvxc(Ds)
    return out + td._ov(F)


def solve_z(td, rhs, conv_tol=1e-9, max_cycle=60, log=None):
    """(A+B) z = rhs by conjugate gradients preconditioned with the orbital-energy differences; one product per iteration.
    Returns (z, converged, iterations, |residual|)."""
    b = rhs.reshape(1, -1)
    Minv = 1.0 / td._de[None, :]
    z = Minv * b
    r = b - _apb(td, z)
    y = Minv * r
    p = y.clone()
    ry = float((r * y).sum())
    rn = float(torch.linalg.norm(r))
    it = 0
    while rn > conv_tol and it < max_cycle:
        Ap = _apb(td, p)
        alpha = ry / float((p * Ap).sum())
        z = z + alpha * p
        r = r - alpha * Ap
        y = Minv * r
        ry_new = float((r * y).sum())
        p = y + (ry_new / ry) * p
        ry = ry_new
        rn = float(torch.linalg.norm(r))
        it += 1
        if log:
            log(f"Z-vector CG it {it}: |r| = {rn:.3e}")
    return z.reshape(rhs.shape), rn <= conv_tol, it, rn


def _wv2(eng, xcf, rho0, rho1, w, eps):
    """Third-order term wv2 = d/de wv1_{rho0 + e rho1}[rho1] by a central difference (layout of xc_eval's wv)."""
    _hyb, terms, gga, params = xcf
    nc = 4 if gga else 1
    out = None
    for sgn in (1.0, -1.0):
        rd = (rho0[:nc] + sgn * eps * rho1).contiguous()
        coef = eng.xc_fxc_prep(terms, rd, w, gga, params=params)
        wv = eng.xc_fxc_apply(rd, coef, rho1.unsqueeze(0).contiguous(), gga)[0]
        out = sgn * wv if out is None else out + sgn * wv
    return out / (2.0 * eps)


def third_order(td, U, step):
    """d2V[U, U] = d2/dh2 V_xc(D0 + h U) (AO matrix) on the SCF's grid blocks."""
    mf = td._scf
    eng = mf.engine
    xcf = mf._xc_functional()
    gga = xcf[2]
    eps = step / max(float(U.abs().max()), 1e-300)
    vmat = torch.zeros_like(U)
    for w, ao in mf._ao_blocks(gga):
        rho0, _tau = mf._block_density(ao, td._D0, None, gga)
        rho1 = eng.xc_rho(ao, U @ ao[0], deriv=1 if gga else 0)
        eng.xc_vmat(ao[0], eng.xc_aow(ao, _wv2(eng, xcf, rho0, rho1, w, eps), gga), vmat)
    return vmat + vmat.T


def relaxed_state(td, x, y, conv_tol=1e-9, max_cycle=60, xc3_step=1e-3, log=None):
    """Steps 1-4 of the module docstring for one state.  `td` has been set up (`_setup`): _Co, _Cv, _de, _jk, _dvxc.
    Returns dict(P, W, U, V, z, converged, niter, residual): AO matrices on td's device; W includes the ground state's."""
    mf = td._scf
    Co, Cv = td._Co, td._Cv
    dev = dict(dtype=torch.float64, device=Co.device)
    no, nv = Co.shape[1], Cv.shape[1]
    eps_mo = torch.as_tensor(np.asarray(mf.mo_energy), **dev)
    eo, ev = eps_mo[:no], eps_mo[no:]
    x, y = torch.as_tensor(np.asarray(x), **dev), torch.as_tensor(np.asarray(y), **dev)
    u, v = x + y, x - y
    doo, dvv = -(u @ u.T + v @ v.T), u.T @ u + v.T @ v
    T = Co @ doo @ Co.T + Cv @ dvv @ Cv.T
    Nu, Nv = Co @ u @ Cv.T, Co @ v @ Cv.T
    U, V = 0.5 * (Nu + Nu.T), 0.5 * (Nv - Nv.T)
    cx = td._kx()
    if td._need_k():
        J, K = td._jk(torch.stack([T, U, V]), [1, 1, -1], with_j=True)
        G0 = 2.0 * J[0] - cx * K[0]
        Gp = 4.0 * J[1] - 2.0 * cx * K[1]
        Gm = 2.0 * cx * K[2]
    else:
        J, _ = td._jk(torch.stack([T, U]), [1, 1], with_j=True, with_k=False)
        G0, Gp, Gm = 2.0 * J[0], 4.0 * J[1], torch.zeros_like(T)
    if td._dft:
        dv = td._dvxc(torch.stack([T, U]))
        G0 = G0 + 2.0 * dv[0] + 8.0 * third_order(td, U, xc3_step)
        Gp = Gp + 4.0 * dv[1]
    C = torch.cat([Co, Cv], dim=1)
    Gp_mo, Gm_mo = C.T @ Gp @ C, C.T @ Gm @ C
    o, vv = slice(0, no), slice(no, no + nv)
    xpy, xmy = u.T, v.T                      # [nvir, nocc]
    wvo = 2.0 * (Cv.T @ G0 @ Co)
    wvo = wvo - 2.0 * torch.einsum("ki,ai->ak", Gp_mo[o, o], xpy) + 2.0 * torch.einsum("ac,ai->ci", Gp_mo[vv, vv], xpy)
    wvo = wvo - 2.0 * torch.einsum("ki,ai->ak", Gm_mo[o, o], xmy) + 2.0 * torch.einsum("ac,ai->ci", Gm_mo[vv, vv], xmy)
    z, conv, nit, res = solve_z(td, -wvo.T.contiguous(), conv_tol, max_cycle, log)
    z1 = z.T                                 # [nvir, nocc]
    Z = _sym(Co @ z @ Cv.T)
    # response of the Fock matrix to Z, then the energy-weighted density
    if td._need_k():
        Jz, Kz = td._jk(Z.unsqueeze(0), [1], with_j=True)
        Gz = 2.0 * Jz[0] - cx * Kz[0]
    else:
        Jz, _ = td._jk(Z.unsqueeze(0), [1], with_j=True, with_k=False)
        Gz = 2.0 * Jz[0]
    if td._dft:
        Gz = Gz + 2.0 * td._dvxc(Z.unsqueeze(0))[0]
    nmo = no + nv
    im0 = torch.zeros(nmo, nmo, **dev)
    im0[o, o] = Co.T @ (G0 + Gz) @ Co
    im0[o, o] += torch.einsum("ak,ai->ki", Gp_mo[vv, o], xpy) + torch.einsum("ak,ai->ki", Gm_mo[vv, o], xmy)
    im0[vv, vv] = torch.einsum("ci,ai->ac", Gp_mo[vv, o], xpy) + torch.einsum("ci,ai->ac", Gm_mo[vv, o], xmy)
    im0[vv, o] = 2.0 * torch.einsum("ki,ai->ak", Gp_mo[o, o], xpy) + 2.0 * torch.einsum("ki,ai->ak", Gm_mo[o, o], xmy)
    zeta = 0.5 * (eps_mo[:, None] + eps_mo[None, :])
    zeta[vv, o] = eo[None, :]
    zeta[o, vv] = ev[None, :]
    dm1 = torch.zeros(nmo, nmo, **dev)
    dm1[o, o] = doo + 2.0 * torch.eye(no, **dev)
    dm1[vv, vv] = dvv
    dm1[vv, o] = z1
    W = _sym(C @ (im0 + zeta * dm1) @ C.T)
    return dict(P=(T + Z).contiguous(), W=W.contiguous(), U=U.contiguous(), V=V.contiguous(), z=z, converged=bool(conv),
                niter=nit, residual=res)


# ---- driver -----------------------------------------------------------------------------------------------------------------------
def _refuse(td):
    if not td.singlet:
        raise NotImplementedError("TDA/TDDFT gradients: triplet states are not implemented (closed-shell singlets only)")
    require(td._scf, "TDA/TDDFT gradients")


class Gradients:
    """Analytic gradient of one TDA / TDHF / TDDFT singlet state on the MI355X engine.  `state` counts from 1; 0 is the
    ground state."""
    conv_tol = 1e-9       # |residual|_2 of the Z-vector equations
    max_cycle = 60
    xc3_step = 1e-3       # step of the central difference of the third-order XC term, relative to max |U|

    def __init__(self, td, algorithm="onepass"):
        _refuse(td)
        self.base = td
        self.mol = td.mol
        self.de = None
        self.state = 1
        self.converged = False
        self.timing = {}
        self.niter = None
        self.verbose = td.verbose
        self._algorithm = None
        self.algorithm = algorithm

    @property
    def algorithm(self):
        return self._algorithm

    @algorithm.setter
    def algorithm(self, name):
        if name not in ALGORITHMS:
            raise ValueError(f"TDA/TDDFT gradients: algorithm must be one of {ALGORITHMS}, got {name!r}")
        self._algorithm = name

    def _grad_eri(self, eng, D0, st, hyb, g2):
        dev = dict(dtype=torch.float64, device=eng.device)
        D, Q, s, R, t, sym = two_particle_terms(D0.cpu().numpy(), st["P"].cpu().numpy(), st["U"].cpu().numpy(),
                                                st["V"].cpu().numpy(), hyb)
        D, Q, R = (torch.as_tensor(a, **dev).contiguous() for a in (D, Q, R))
        if self.algorithm == "onepass":
            eng.grad_eri(D, hyb, g2, pairs=(Q, s), xpairs=(R, t, sym))
            return
        eng.grad_eri(D, hyb, g2)
        tmp = torch.zeros_like(g2)

        def plain(M, h):
            tmp.zero_()
            eng.grad_eri(M.contiguous(), h, tmp)
            return tmp.clone()
        for k in range(len(s)):
            g2 += float(s[k]) * plain(Q[k], 0.0)
        for m in range(len(t)):
            if sym[m] > 0:
                g2 += -4.0 * float(t[m]) * (plain(R[m], 1.0) - plain(R[m], 0.0))
            else:   # no older entry point takes an antisymmetric matrix: this term alone through the new one
                tmp.zero_()
                eng.grad_eri(torch.zeros_like(D), 0.0, tmp, xpairs=(R[m:m + 1].contiguous(), t[m:m + 1], sym[m:m + 1]))
                g2 += tmp

    def _grad_xc(self, D0, st):
        td = self.base
        mf = td._scf
        eng = mf.engine
        xcf = mf._xc_functional()
        _hyb, terms, gga, params = xcf
        nc = 4 if gga else 1
        P, U = st["P"], st["U"]
        eps = self.xc3_step / max(float(U.abs().max()), 1e-300)
        DP = D0 + P

        def body(fmu, ao, w):
            C0, CP, CU = D0 @ ao[0], P @ ao[0], U @ ao[0]
            rho0, tau = mf._block_density(ao, D0, None, gga, C0)
            _e, (wv0,) = mf._block_functional(xcf, [rho0], [tau], w)
            rho0 = rho0[:nc].contiguous()
            rhoP = eng.xc_rho(ao, CP, deriv=1 if gga else 0)
            rhoU = eng.xc_rho(ao, CU, deriv=1 if gga else 0)
            coef = eng.xc_fxc_prep(terms, rho0, w, gga, params=params)
            wv1 = eng.xc_fxc_apply(rho0, coef, torch.stack([rhoP, rhoU]).contiguous(), gga)
            wv2 = _wv2(eng, xcf, rho0, rhoU, w, eps)
            _add_xc_force(fmu, ao, DP, C0 + CP, wv0, gga)
            _add_xc_force(fmu, ao, D0, C0, wv1[0] + 4.0 * wv2, gga)
            _add_xc_force(fmu, ao, U, CU, 8.0 * wv1[1], gga)
        return xc_force(mf, body)

    def kernel(self, xy=None, state=None, atmlst=None):
        from .ao2mo import resident_engine
        from .dft import parse_xc
        td = self.base
        _refuse(td)
        if state is not None:
            self.state = int(state)
        state = self.state
        mf = td._scf
        if state == 0:
            g = mf.nuc_grad_method()
            self.de = g.kernel()
            self.converged = bool(mf.converged)
            self.timing = dict(getattr(g, "timing", {}))
            return self.de
        if xy is None and (td.xy is None or td.e is None):
            td.kernel()
        if state < 0 or state > len(td.e):
            raise NotImplementedError(f"TDA/TDDFT gradients: state {state} is above nstates = {len(td.e)} (states count from 1; "
                                      "0 is the ground state)")
        if xy is None and not bool(np.asarray(td.converged)[state - 1]):
            raise NotImplementedError(f"TDA/TDDFT gradients: root {state} of the excited-state solver is not converged")
        eng = resident_engine(mf, "TDA/TDDFT gradients")
        if getattr(td, "_Co", None) is None or td._Co.device != eng.device or td._Co.shape[0] != eng.nao:
            td._setup()
        x, y = td.xy[state - 1] if xy is None else xy
        is_ks = td._dft
        hyb = td._hyb if is_ks else 1.0
        semilocal = bool(is_ks and parse_xc(mf.xc)[1])
        mol = mf.mol
        dev = dict(dtype=torch.float64, device=eng.device)
        tm = {}
        t0 = time.time()
        D0 = torch.as_tensor(np.asarray(mf.make_rdm1()), **dev).contiguous()
        if is_ks:
            td._D0 = D0
        st = relaxed_state(td, x, y, self.conv_tol, self.max_cycle, self.xc3_step, log=lambda s: td._log(4, s))
        torch.cuda.synchronize()
        tm["zvector"] = time.time() - t0
        self.converged, self.niter = st["converged"], st["niter"]
        if not st["converged"]:
            raise RuntimeError(f"TDA/TDDFT gradients: the Z-vector equations did not converge in {self.max_cycle} iterations "
                               f"(|r| = {st['residual']:.2e}, conv_tol = {self.conv_tol:.1e})")
        self.timing = tm
        self.de = de = assemble(eng, mol, (D0 + st["P"]).contiguous(), st["W"], lambda g2: self._grad_eri(eng, D0, st, hyb, g2),
                                (lambda: self._grad_xc(D0, st)) if semilocal else None, tm)
        log_gradient(td._log, mol, de, self.verbose >= 4, tm, f"TD gradient (state {state}, {self.algorithm}, Z-vector {st['niter']} iterations)",
                     f"--------------- gradients of excited state {state} ---------------")
        return de

    grad = kernel

    def as_scanner(self, state=None):
        if state is not None:
            self.state = int(state)
        return _TDGradScanner(self)


class _TDGradScanner(_GradScanner):
    """(E_SCF + w_n, de) at a new geometry: the SCF from the previous density, the Davidson from the previous vectors (`x0`), the
    state followed by its overlap sum_ia X_ia X'_ia / (|X| |X'|) with the previous X.  Below FOLLOW_MIN_OVERLAP it warns and
    keeps the best match: the state is never switched silently."""

    def __init__(self, g):
        super().__init__(g)
        self.state = g.state
        self.overlap = None

    def _energy(self, mol, dm0):
        g = self.g
        td = g.base
        mf = td._scf
        prev = td.xy if (td.xy is not None and self.state > 0) else None
        e0 = self._run_scf(mol, dm0)
        g.state = self.state          # what `g.kernel()` differentiates
        self.converged = bool(mf.converged)
        if self.state == 0:
            return e0
        td.kernel(x0=prev)
        n = self.state
        if prev is not None and self.state <= len(prev):
            xp = np.asarray(prev[self.state - 1][0]).ravel()
            ov = np.array([abs(float(xp @ np.asarray(x).ravel())) / (np.linalg.norm(xp) * np.linalg.norm(x) + 1e-300)
                           for x, _y in td.xy]) if all(np.asarray(x).size == xp.size for x, _y in td.xy) else None
            if ov is not None:
                n = int(np.argmax(ov)) + 1
                self.overlap = float(ov[n - 1])
                if self.overlap < FOLLOW_MIN_OVERLAP:
                    warnings.warn(f"TD gradient scanner: the best overlap with the followed state is {self.overlap:.2f} "
                                  f"(< {FOLLOW_MIN_OVERLAP}); continuing with state {n}, which may be a different state")
                elif n != self.state:
                    td._log(3, f"TD gradient scanner: following the state from root {self.state} to root {n} "
                               f"(overlap {self.overlap:.2f})")
                g.state = self.state = n
        self.converged = bool(mf.converged and np.asarray(td.converged)[n - 1])
        return e0 + float(td.e[n - 1])

    def __call__(self, mol_or_geom):
        e, de = super().__call__(mol_or_geom)
        self.converged = bool(self.converged and self.g.converged)   # the Z-vector solve of the gradient as well
        return e, de
