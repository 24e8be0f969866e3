"""Nuclear gradients behind `mf.nuc_grad_method()` (used by `optimize`,
`templates/optimize_geometry.py:99`).

`Gradients` is analytic: dE/dR = 1e term (`mi_grad_1e`: D.dh - W.dS + Hellmann-Feynman) + 2e term
(`mi_grad_eri`: derivative ERIs contracted with the two-particle density) + XC term (HIP AO second
derivatives + device contractions, no grid-weight response, as PySCF's default `grid_response=False` [MEM])
+ nuclear repulsion.  `FDGradients` (central finite differences of the SCF energy) is kept as the
independent check used by the tests.

The pieces every analytic gradient driver shares live here (`casscf_grad.py` and `tdscf_grad.py` use them too): `assemble` (1e +
2e + nuclear + XC parts under their timers), `log_gradient`, `xc_force` (the grid-block loop of the XC term) and the scanner base `_GradScanner`.
"""
import time

import numpy as np
import torch

from .mole import Mole
from .reference import require


def grad_nuc(mol):
    z = mol.atom_charges().astype(np.float64)
    R = mol.atom_coords()
    g = np.zeros_like(R)
    for i in range(mol.natm):
        for j in range(mol.natm):
            if i != j:
                d = R[i] - R[j]
                g[i] -= z[i] * z[j] * d / np.linalg.norm(d) ** 3
    return g


_D2 = {(0, 0): 4, (0, 1): 5, (0, 2): 6, (1, 1): 7, (1, 2): 8, (2, 2): 9}   # component of eval_ao(deriv=2) holding d_j d_k phi, j <= k


def _add_xc_force(fmu, ao, dm, C, wv, gga, pt=None):
    """fmu[mu] += -2 D_mu,nu int [v_rho dphi_mu phi_nu + 2 v_sigma grad rho . grad(dphi_mu phi_nu)] (+ the tau term) over one
    grid block, for one density `dm` (closed shell, or one spin) with C = dm.ao0 and the weighted derivatives `wv` of the
    functional that belong to it.  pt [3, points of the block] (grid response): += the same integrand summed over the AOs at
    each point, i.e. -w grad_r e of this density's part."""
    T1 = 2.0 * wv[0] * C
    if gga:
        Ck = [dm @ ao[1 + j] for j in range(3)]
        for j in range(3):
            T1 += wv[1 + j] * Ck[j]
        for k in range(3):
            t2 = sum(wv[1 + j] * ao[_D2[(min(j, k), max(j, k))]] for j in range(3))
            p1, p2 = ao[1 + k] * T1, t2 * C
            fmu[:, k] += -2.0 * (p1.sum(dim=1) + p2.sum(dim=1))
            if pt is not None:
                pt[k] += -2.0 * (p1.sum(dim=0) + p2.sum(dim=0))
            if gga == 2:   # d tau / d A_x = - sum_k (d_x d_k phi_mu) (D d_k phi)_mu ; wv[4] = w/4 de/dtau
                p3 = [ao[_D2[(min(j, k), max(j, k))]] * (wv[4] * Ck[j]) for j in range(3)]
                fmu[:, k] += -4.0 * sum(p.sum(dim=1) for p in p3)
                if pt is not None:
                    pt[k] += -4.0 * sum(p.sum(dim=0) for p in p3)
    else:
        for k in range(3):
            p1 = ao[1 + k] * T1
            fmu[:, k] += -2.0 * p1.sum(dim=1)
            if pt is not None:
                pt[k] += -2.0 * p1.sum(dim=0)


def xc_force(mf, body, grid_response=False):
    """XC gradient per atom: `body(fmu, ao, w)` adds one grid block's forces to fmu [nao, 3] (`_add_xc_force`), `ao` the AO values
    with the derivatives the force needs and `w` the block's weights, over this rank's share of the SCF grid.

    grid_response: the quadrature E_xc = sum_g w_g(R) e(r_g(R)) is differentiated as well.  `body(fmu, ao, w, pt)` then also adds
    the per-point AO sums of its integrand to pt [3, points] and returns the block's unweighted energy density e.  Because e at
    a point depends on r - R_B only, -pt is w grad_r e: booked to the point's parent atom it is the moving-point term, and
    `engine.becke_weights_grad` adds sum_g e_g dw_g/dR.  Both are O(1) Ha/Bohr and cancel to three or four digits, so both take
    the SAME e (the evaluator's own density floor) and are summed in FP64.  They sit behind fmu in one buffer: one all-reduce."""
    eng = mf.engine
    gga = mf._xc_functional()[2]
    grids = mf.grids
    coords, weights = grids.coords, grids.weights
    lo, hi = mf._grid_range(coords.shape[0])
    nao, natm = eng.nao, mf.mol.natm
    fmu = torch.zeros(nao + (natm if grid_response else 0), 3, dtype=torch.float64, device=eng.device)
    B = max(4096, mf.grid_block // 4)
    for p0 in range(lo, hi, B):
        p1 = min(p0 + B, hi)
        ao = eng.eval_ao(coords[p0:p1], deriv=2 if gga else 1)
        if not grid_response:
            body(fmu, ao, weights[p0:p1])
            continue
        pt = torch.zeros(3, p1 - p0, dtype=torch.float64, device=eng.device)
        e = body(fmu[:nao], ao, weights[p0:p1], pt)
        resp = fmu[nao:]
        resp.index_add_(0, grids.atom_of_dev[p0:p1].long(), pt.T, alpha=-1.0)
        eng.becke_weights_grad(coords[p0:p1], grids.atom_of_dev[p0:p1], grids.vol[p0:p1], grids.adjust, e.contiguous(), out=resp)
    if mf._nranks > 1:
        from . import parallel
        parallel.all_reduce_sum(fmu, mf._pg)
    f = fmu.cpu().numpy()
    sl = mf.mol.aoslice_by_atom()
    de = np.array([f[sl[ia, 2]:sl[ia, 3]].sum(axis=0) for ia in range(natm)])
    return de + f[nao:] if grid_response else de


def assemble(eng, mol, D, W, two_electron, xc=None, timing=None, ranks=None):
    """de [natm, 3] = `grad_1e` of (D, W) + the two-electron part + nuclear repulsion (+ the XC part `xc()`), each under its timer
    (`timing`: grad_1e, grad_eri, grad_xc).  `two_electron(g2)` accumulates into the zeroed device array g2 or returns its own.
    ranks = (nranks, process group) of a caller whose `two_electron` evaluates this rank's share only: g2 is summed over the ranks
    and rank 0's result becomes everybody's."""
    tm = {} if timing is None else timing
    t0 = time.time()
    g = torch.zeros(mol.natm, 3, dtype=torch.float64, device=eng.device)
    eng.grad_1e(D, W, g)
    torch.cuda.synchronize()
    tm["grad_1e"] = time.time() - t0
    t0 = time.time()
    g2 = torch.zeros_like(g)
    out = two_electron(g2)
    g2 = g2 if out is None else out
    torch.cuda.synchronize()
    tm["grad_eri"] = time.time() - t0
    nranks, pg = ranks if ranks is not None else (1, None)
    if nranks > 1:   # derivative-quartet batches are dealt round-robin to ranks inside mi_grad_eri
        from . import parallel
        parallel.all_reduce_sum(g2, pg)
    de = (g + g2).cpu().numpy() + grad_nuc(mol)
    if xc is not None:
        t0 = time.time()
        de = de + xc()
        torch.cuda.synchronize()
        tm["grad_xc"] = time.time() - t0
    if nranks > 1:
        dt = torch.as_tensor(de, device=eng.device)
        parallel.broadcast0(dt, pg)
        de = dt.cpu().numpy()
    return de


def log_gradient(log, mol, de, table, timing=None, header="gradient", title="--------------- gradients ---------------"):
    """The timing line and (table: the caller's verbosity asks for it) the per-atom table, through `log(level, text)`."""
    if timing is not None:
        log(4, f"{header} timings (s): " + ", ".join(f"{k} {v:.3f}" for k, v in timing.items()))
    if table:
        log(4, title)
        for ia in range(mol.natm):
            log(4, "%d %s  %16.10f %16.10f %16.10f" % (ia, mol.atom_pure_symbol(ia), *de[ia]))


class Gradients:
    """Analytic RHF/RKS gradient on the MI355X engine."""
    # True (PySCF's switch): the XC term is the derivative of the quadrature the SCF energy is made of -- the points move with
    # their atoms and the Becke weights are differentiated (`xc_force`); the scanner carries it with this object
    grid_response = False

    def __init__(self, mf):
        require(mf, "nuclear gradients")
        self.base = mf
        self.mol = mf.mol
        self.de = None
        self.verbose = mf.verbose

    def grad_xc(self, dm):
        """XC gradient of RKS: `_add_xc_force` of the closed-shell density over this rank's grid, summed per atom."""
        return self._grad_xc([dm])

    def _grad_xc(self, dms):
        """XC gradient of one density (closed shell) or two (spin): per grid block the densities and the functional of the SCF's
        block body (`dft.KSMixin`), on AO values with second derivatives, then `_add_xc_force` of each (D_s, wv_s)."""
        mf = self.base
        xcf = mf._xc_functional()
        gga = xcf[2]

        def body(fmu, ao, w, pt=None):
            Cs = [dm @ ao[0] for dm in dms]
            dens = [mf._block_density(ao, dm, None, gga, C) for dm, C in zip(dms, Cs)]
            e, wvs = mf._block_functional(xcf, [d[0] for d in dens], [d[1] for d in dens], w)
            for dm, C, wv in zip(dms, Cs, wvs):
                _add_xc_force(fmu, ao, dm, C, wv, gga, pt)
            return e
        return xc_force(mf, body, bool(self.grid_response))

    def _densities(self):
        """What `kernel` contracts, from the converged SCF: (densities of the XC term, total density D, spin density M or None,
        energy-weighted density W, densities handed to the fitted `grad_jk`)."""
        mf = self.base
        dm = mf._dm
        W = 0.5 * dm @ (mf._h1 + mf._vhf) @ dm
        return [dm], dm.contiguous(), None, W.contiguous(), dm

    def kernel(self, mo_energy=None, mo_coeff=None, mo_occ=None, atmlst=None):
        mf = self.base
        if mf._dm is None or not mf.converged:
            mf.kernel()
        eng = mf.engine
        mol = mf.mol
        dms, D, M, W, dm_fit = self._densities()
        is_ks = getattr(mf, "xc", None) is not None and hasattr(mf, "grids")
        hyb = mf._xc_functional()[0] if is_ks else 1.0

        def two_electron(g2):
            if getattr(mf, "with_df", None) is not None:
                return _fitted_tensor(mf).grad_jk(dm_fit, hyb, rank=mf._rank, nranks=mf._nranks)
            eng.grad_eri(D, hyb, g2, spin_density=M, rank=mf._rank, nranks=mf._nranks)
        self.timing = {}
        self.de = de = assemble(eng, mol, D, W, two_electron, (lambda: self._grad_xc(dms)) if is_ks else None, self.timing,
                                (mf._nranks, mf._pg))
        log_gradient(mf._log, mol, de, self.verbose >= 4, self.timing)
        return de

    grad = kernel

    def as_scanner(self):
        return _GradScanner(self)


def _fitted_tensor(mf):
    """The fitted tensor with the WHOLE auxiliary index on this rank: `mf.with_df` itself, or (sharded run: every rank holds a
    slice of the whitened index, and the exchange part of the two-index density couples all slices) one rebuilt here."""
    d = mf.with_df
    if getattr(d, "_nranks_built", 1) == 1 and d._B is not None:
        return d
    from .df import DF
    return DF(mf.mol, d.auxbasis, d.beta).build(mf.engine)


class UGradients(Gradients):
    """Analytic UHF gradient: the restricted pieces with D = Da + Db, W = sum_s Ds Fs Ds, and the exchange part of
    the two-particle density from both spins (`mi_grad_eri_spin`, spin density M = Da - Db)."""

    def _densities(self):
        mf = self.base
        dma, dmb = mf._dm[0], mf._dm[1]
        F = mf._fock
        W = (dma @ F[0] @ dma + dmb @ F[1] @ dmb).contiguous()
        return [dma, dmb], (dma + dmb).contiguous(), (dma - dmb).contiguous(), W, [dma, dmb]

    def grad_xc_spin(self, dm):
        """XC gradient of UKS: `_add_xc_force` per spin with (D_s, wv_s) from the spin-polarised functional."""
        return self._grad_xc([dm[0], dm[1]])


class FDGradients:
    step = 2.0e-3  # Bohr

    def __init__(self, mf):
        require(mf, "nuclear gradients")
        self.base = mf
        self.mol = mf.mol
        self.de = None
        self.verbose = mf.verbose

    def _energy_at(self, coords, dm0):
        mf = self.base
        mol = mf.mol.set_geom_(coords, unit="Bohr", inplace=False)
        mol.verbose = 0
        clone = mf.__class__(mol)
        for k in ("xc", "conv_tol", "max_cycle", "eig_method", "init_guess", "direct_scf_tol", "level_shift", "diis_space",
                  "diis_start_cycle"):
            if hasattr(mf, k):
                setattr(clone, k, getattr(mf, k))
        if hasattr(mf, "grids"):
            clone.grids.level, clone.grids.prune = mf.grids.level, mf.grids.prune
        clone.verbose = 0
        clone.conv_tol = min(mf.conv_tol, 1e-10)
        e = clone.kernel(dm0=dm0)
        if not clone.converged:
            raise RuntimeError("SCF did not converge at a displaced geometry")
        clone._eng = None
        return e

    def kernel(self, mo_energy=None, mo_coeff=None, mo_occ=None, atmlst=None):
        mf = self.base
        if mf.mo_coeff is None or not mf.converged:
            mf.kernel()
        dm0 = mf.make_rdm1()
        R = mf.mol.atom_coords()
        g = np.zeros_like(R)
        h = self.step
        atoms = range(mf.mol.natm) if atmlst is None else atmlst
        for ia in atoms:
            for x in range(3):
                Rp, Rm = R.copy(), R.copy()
                Rp[ia, x] += h
                Rm[ia, x] -= h
                g[ia, x] = (self._energy_at(Rp, dm0) - self._energy_at(Rm, dm0)) / (2 * h)
        self.de = g
        log_gradient(mf._log, mf.mol, g, self.verbose >= 5, title="--------------- gradients (finite difference) ---------------")
        return g

    grad = kernel

    def as_scanner(self):
        return _GradScanner(self)


class _GradScanner:
    """(energy, de) at a new geometry.  `_energy` is what the methods differ in; the rest -- the geometry, the starting density,
    the SCF with the gradient's prefetch, `grad_dtol` (set by `geomopt.optimize`), the gradient -- is here."""

    def __init__(self, g):
        self.g = g
        self.base = g.base
        self.mol = g.mol
        self.converged = True

    @property
    def _scf(self):
        return getattr(self.base, "_scf", self.base)

    def _run_scf(self, mol, dm0):
        mf = self._scf
        mf.reset(mol)
        mf._grad_prefetch = True      # the gradient's host-side set-up overlaps this SCF (engine option `grad_prefetch`)
        e = mf.kernel(dm0=dm0)
        self.g.mol = self.mol = mol
        return e

    def _energy(self, mol, dm0):
        """The energy at `mol` from the starting density dm0 (through `_run_scf`); sets `converged`."""
        e = self._run_scf(mol, dm0)
        self.converged = self._scf.converged
        return e

    def __call__(self, mol_or_geom):
        mf = self._scf
        mol = mol_or_geom if isinstance(mol_or_geom, Mole) else mf.mol.set_geom_(mol_or_geom, unit="Bohr", inplace=False)
        # starting density: the converged AO matrix as it is (the basis functions follow their atoms).  Transporting it in the
        # Cholesky-orthonormal frame instead (D = L_new^-T (L_old^T D L_old) L_new^-1: idempotent and N-electron in the new
        # metric) was measured WORSE -- ibuprofen B3LYP/def2-TZVP optimisation 105 instead of 86 SCF cycles over 12 steps,
        # benzene 20 instead of 14 (tools/opt_variants.py): Gram-Schmidt in AO order drags every later atom's functions along
        dm0 = mf.make_rdm1() if mf.mo_coeff is not None else None
        e = self._energy(mol, dm0)
        if getattr(self, "grad_dtol", None) is not None:
            mf.engine.set_option("grad_dtol", self.grad_dtol)   # density-weighted screening of the derivative quartets
        return e, self.g.kernel()
