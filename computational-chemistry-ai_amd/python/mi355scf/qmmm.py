"""Electrostatic embedding in fixed external charges (`pyscf.qmmm.mm_charge`, `pyscf.qmmm.mm_charge_grad`).

The interface is PySCF's as remembered [MEM]: `mm_charge(mf, coords, charges, radii=None, unit=None)` returns an object of mf's
own kind whose core Hamiltonian carries the potential of the charges, `mf.nuc_grad_method()` on it gives the gradient on the
QM atoms, and `grad_hcore_mm` / `grad_nuc_mm` give the derivatives of the energy with respect to the MM sites.  No PySCF was
available when this was written, so parity with it has not been checked.

  sites        r_k [n, 3] (Bohr inside), charges q_k; `radii` [MEM] selects Gaussian charges of width zeta_k = 1 / radius_k,
               whose potential is g_k(r) = erf(zeta_k r) / r (the C-PCM convention); without radii g_k(r) = 1 / r
  core term    h1 += V_mm,  V_mm[m, n] = -sum_k q_k (m| g_k(|r - r_k|) |n)           (`Engine.pc_fock`, once per geometry)
  nuclear term E_nuc += sum_A sum_k Z_A q_k g_k(|R_A - r_k|)                          (host)
  not included the interaction of the MM charges with each other (as in PySCF [MEM])
  gradient     dE/dR_A += -(d/dR_A) sum_k q_k D.(m|g_k|n) (`Engine.pc_grad`, atom part) + d E_nuc-mm / dR_A; the orbital response is
               in the SCF's energy-weighted density, whose Fock matrix holds V_mm through h1
  sites        dE/dr_k = -(pc_grad's site part) + d E_nuc-mm / dr_k

The embedding is part of h1, so the SCF cycle, its captured graph and the purification see an ordinary core Hamiltonian.  One
rank, no density fitting, no PCM on top; the post-SCF methods that were not checked with an embedded reference refuse it
(the "qmmm" entries of `reference.SUPPORT`), MP2 reads only the orbitals and their energies and is allowed."""
import numpy as np
import torch

from .mole import BOHR
from .reference import require, traits, wrap

NEAR = 1e-8        # Bohr: a point charge this close to a nucleus makes the energy diverge
_TSP = 2.0 / np.sqrt(np.pi)


# ---- host pieces (NumPy / CPU torch: no GPU) -----------------------------------------------------------------------------------
def mm_sites(mol, coords, charges, radii=None, unit=None):
    """(coords [n, 3] in Bohr, charges [n], zeta [n]) of an embedding: `unit` None means the molecule's unit, `radii` (same unit)
    selects Gaussian charges of width zeta = 1 / radius, zeta = 0 marks a point charge."""
    unit = str(mol.unit if unit is None else unit).upper()
    scale = 1.0 if unit.startswith(("B", "AU")) else 1.0 / BOHR
    c = np.asarray(coords, dtype=np.float64).reshape(-1, 3) * scale
    q = np.asarray(charges, dtype=np.float64).reshape(-1)
    if q.size != c.shape[0]:
        raise ValueError(f"mm_charge: {c.shape[0]} coordinates for {q.size} charges")
    if radii is None:
        zeta = np.zeros(q.size)
    else:
        r = np.broadcast_to(np.asarray(radii, dtype=np.float64), q.shape) * scale
        if not (np.isfinite(r).all() and (r >= 0).all()):
            raise ValueError("mm_charge: radii must be finite and not negative")
        zeta = np.where(r > 0, 1.0 / np.where(r > 0, r, 1.0), 0.0)      # radius 0: the zero-width limit, a point charge
    if not (np.isfinite(c).all() and np.isfinite(q).all()):
        raise ValueError("mm_charge: coordinates and charges must be finite")
    return np.ascontiguousarray(c), np.ascontiguousarray(q), np.ascontiguousarray(zeta)


def check_sites(atom_coords, atom_charges, coords, zeta):
    """NotImplementedError when a point charge sits within NEAR of a nucleus (a Gaussian charge may: its potential is finite)."""
    X = np.asarray(atom_coords, dtype=np.float64).reshape(-1, 3)
    point = np.asarray(zeta) <= 0.0
    if X.size == 0 or not point.any():
        return
    real = np.asarray(atom_charges) != 0
    d = np.linalg.norm(X[real][:, None, :] - coords[point][None, :, :], axis=2)
    if d.size and d.min() < NEAR:
        a, k = np.unravel_index(int(d.argmin()), d.shape)
        raise NotImplementedError(f"mm_charge: point charge {np.flatnonzero(point)[k]} lies {d.min():.1e} Bohr from nucleus "
                                  f"{np.flatnonzero(real)[a]}: the energy diverges (give it a radius for a Gaussian charge)")


def _g_dg(r, zeta):
    """g(r) and g'(r) / r of every (atom, site) pair: 1/r or erf(zeta r)/r; the Gaussian kind is finite at r = 0 (g = 2 zeta /
    sqrt(pi), no force)."""
    z = np.broadcast_to(zeta, r.shape)
    gauss = z > 0.0
    safe = np.where(r > 0.0, r, 1.0)
    zr = np.where(gauss, z * safe, 0.0)
    erf = torch.erf(torch.as_tensor(zr)).numpy()
    g = np.where(gauss, erf / safe, 1.0 / safe)
    dg = np.where(gauss, (_TSP * z * np.exp(-zr * zr) * safe - erf) / safe ** 3, -1.0 / safe ** 3)
    at0 = r <= 0.0
    g = np.where(at0 & gauss, _TSP * z, g)
    dg = np.where(at0, 0.0, dg)
    return g, dg


def energy_nuc_mm(atom_coords, atom_charges, coords, charges, zeta):
    """sum_A sum_k Z_A q_k g_k(|R_A - r_k|)."""
    X = np.asarray(atom_coords, dtype=np.float64).reshape(-1, 3)
    Z = np.asarray(atom_charges, dtype=np.float64)
    if len(charges) == 0:
        return 0.0
    r = np.linalg.norm(X[:, None, :] - coords[None, :, :], axis=2)
    g, _dg = _g_dg(r, zeta[None, :])
    return float(Z @ g @ charges)


def grad_nuc_mm(atom_coords, atom_charges, coords, charges, zeta):
    """(d/dR_A [natm, 3], d/dr_k [n, 3]) of `energy_nuc_mm`."""
    X = np.asarray(atom_coords, dtype=np.float64).reshape(-1, 3)
    Z = np.asarray(atom_charges, dtype=np.float64)
    if len(charges) == 0:
        return np.zeros_like(X), np.zeros((0, 3))
    dv = X[:, None, :] - coords[None, :, :]
    r = np.linalg.norm(dv, axis=2)
    _g, dg = _g_dg(r, zeta[None, :])
    t = (Z[:, None] * charges[None, :] * dg)[:, :, None] * dv
    return t.sum(axis=1), -t.sum(axis=0)


# ---- the embedded SCF object ---------------------------------------------------------------------------------------------------
class MMSites:
    """`mf.mm_mol`: the sites in Bohr (`atom_coords()`), their charges (`atom_charges()`) and widths (`zeta`, 0 = point)."""

    def __init__(self, coords, charges, zeta):
        self.coords, self.charges, self.zeta = coords, charges, zeta
        self.natm = len(charges)

    def atom_coords(self, unit="Bohr"):
        return self.coords * (BOHR if str(unit).upper().startswith("ANG") else 1.0)

    def atom_charges(self):
        return self.charges.copy()

    def device_points(self, device):
        pts = np.concatenate([self.coords, self.zeta[:, None]], axis=1)
        return (torch.as_tensor(np.ascontiguousarray(pts), device=device),
                torch.as_tensor(np.ascontiguousarray(self.charges), device=device))


class _QMMMMixin:
    """Methods an embedded SCF object gains (the class is made at run time: `mm_charge(mf, ...)`)."""
    _qmmm = True

    @property
    def mm_coords(self):
        return self.mm_mol.coords

    @property
    def mm_charges(self):
        return self.mm_mol.charges

    def _check_embedding(self):
        require(self, "embedded SCF")
        mm = self.mm_mol
        check_sites(self.mol.atom_coords(), self.mol.atom_charges(), mm.coords, mm.zeta)

    def _v_mm(self, out=None, accumulate=False):
        eng = self.engine
        pts, q = self.mm_mol.device_points(eng.device)
        if out is None:
            out = torch.zeros(eng.nao, eng.nao, dtype=torch.float64, device=eng.device)
        return eng.pc_fock(pts, q, out, scale=-1.0, accumulate=accumulate)   # electrons carry -1

    def _setup(self):
        self._check_embedding()
        super()._setup()
        self._h1 = self._h1.contiguous()
        self._v_mm(self._h1, accumulate=True)      # once per geometry: everything downstream sees an ordinary h1

    def get_hcore(self, mol=None):
        self._check_embedding()
        return super().get_hcore(mol) + self._v_mm().cpu().numpy()

    def energy_nuc(self):
        mm, mol = self.mm_mol, self.mol
        self._check_embedding()
        return super().energy_nuc() + energy_nuc_mm(mol.atom_coords(), mol.atom_charges(), mm.coords, mm.charges, mm.zeta)

    def nuc_grad_method(self):
        return _embedded_gradients(super().nuc_grad_method(), self.mm_mol)

    Gradients = nuc_grad_method


_CLASSES = {}


def mm_charge(mf, coords, charges, radii=None, unit=None):
    """`qmmm.mm_charge(mf, coords, charges)`: mf embedded in the charges (an instance of a subclass of mf's class made at run
    time, sharing mf's state).  RHF / UHF / ROHF / RKS / UKS / ROKS on one rank."""
    require(mf, "qmmm.mm_charge")
    sites = MMSites(*mm_sites(mf.mol, coords, charges, radii, unit))
    check_sites(mf.mol.atom_coords(), mf.mol.atom_charges(), sites.coords, sites.zeta)
    new = mf if isinstance(mf, _QMMMMixin) else wrap(mf, _QMMMMixin, "QMMM", _CLASSES)   # (again: the sites are replaced)
    new.mm_mol = sites
    new._h1 = None          # the core Hamiltonian of the bare molecule is no longer this object's
    return new


# ---- gradients -------------------------------------------------------------------------------------------------------------------
class _QMMMGradMixin:
    """What a gradient object of an embedded SCF gains: the MM terms on the QM atoms and the derivatives on the sites."""
    _qmmm = True

    def _total_density(self, dm=None):
        mf = self.base
        if dm is None:
            if mf._dm is None or not mf.converged:
                mf.kernel()
            return self._densities()[1]
        d = torch.as_tensor(np.asarray(dm), dtype=torch.float64, device=mf.engine.device)
        if d.dim() == 3:
            d = d[0] + d[1]
        return d

    def _pc_grad(self, dm=None):
        mf, mm = self.base, self.mm_mol
        D = self._total_density(dm)
        D = (0.5 * (D + D.T)).contiguous()
        pts, q = mm.device_points(mf.engine.device)
        ga, gp = mf.engine.pc_grad(pts, q, D)
        return -ga.cpu().numpy(), -gp.cpu().numpy()          # electrons carry -1

    def grad_hcore_mm(self, dm=None):
        """dE/dr_k [nmm, 3] of the electron-charge attraction for the density `dm` (None: the converged one)."""
        return self._pc_grad(dm)[1]

    def grad_nuc_mm(self):
        """dE/dr_k [nmm, 3] of the nucleus-charge interaction."""
        mm, mol = self.mm_mol, self.base.mol
        return grad_nuc_mm(mol.atom_coords(), mol.atom_charges(), mm.coords, mm.charges, mm.zeta)[1]

    def kernel(self, mo_energy=None, mo_coeff=None, mo_occ=None, atmlst=None):
        de = super().kernel(mo_energy, mo_coeff, mo_occ, atmlst)
        mm, mol = self.mm_mol, self.base.mol
        de = de + self._pc_grad()[0] + grad_nuc_mm(mol.atom_coords(), mol.atom_charges(), mm.coords, mm.charges, mm.zeta)[0]
        self.de = de
        return de

    grad = kernel


_GRAD_CLASSES = {}


def _embedded_gradients(g, sites):
    if isinstance(g, _QMMMGradMixin):
        g.mm_mol = sites
        return g
    return wrap(g, _QMMMGradMixin, "QMMM", _GRAD_CLASSES, mm_mol=sites)


def mm_charge_grad(grad_obj, coords, charges, radii=None, unit=None):
    """`qmmm.mm_charge_grad(mf.nuc_grad_method(), coords, charges)` [MEM]: the gradient object with the MM terms.  Its SCF
    must be embedded in the same charges (the energy-weighted density needs the embedded Fock matrix)."""
    mf = grad_obj.base
    if not traits(mf).qmmm:
        raise NotImplementedError("qmmm.mm_charge_grad: the SCF object behind the gradient is not embedded (use qmmm.mm_charge first)")
    if not all(hasattr(grad_obj, a) for a in ("_densities", "kernel")):
        raise NotImplementedError(f"qmmm.mm_charge_grad: {type(grad_obj).__name__} is not an analytic SCF gradient of this engine")
    c, q, z = mm_sites(mf.mol, coords, charges, radii, unit)
    mm = mf.mm_mol
    if c.shape != mm.coords.shape or not (np.allclose(c, mm.coords, atol=1e-12) and np.array_equal(q, mm.charges)
                                          and np.allclose(z, mm.zeta, atol=1e-12)):
        raise ValueError("qmmm.mm_charge_grad: the charges differ from the ones the SCF object is embedded in")
    return _embedded_gradients(grad_obj, mm)
