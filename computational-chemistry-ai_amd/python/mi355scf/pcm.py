"""C-PCM implicit solvation for closed-shell SCF (`pyscf.solvent.PCM`, `templates/calculate_solvent_effect.py`).

The model is the one PySCF documents as its default `solvent.PCM` [MEM]: conductor-like screening with Gaussian-smeared
surface charges (York and Karplus, J. Phys. Chem. A 103, 11060 (1999)) on switched Lebedev spheres (SWIG switching function of
Lange and Herbert, J. Chem. Phys. 133, 244111 (2010)).  Every default below was written from memory: no PySCF and no paper
were available when it was entered, so parity with PySCF has not been checked.

  surface      per atom J: Lebedev sphere of radius R_J (scaled Bondi radius), switching value swf_i = prod_{J != owner} h(d_iJ)
  S            S_ij = erf(zeta_ij r_ij) / r_ij, zeta_ij = zeta_i zeta_j / sqrt(zeta_i^2 + zeta_j^2); S_ii = zeta_i sqrt(2/pi) / swf_i
  potential    v = v_n - v_e, v_e,g = sum_mn D_mn B_g,mn  (B: one-electron integrals against the Gaussian charges, HIP kernels)
  charges      q = -f S^-1 v, f = (eps - 1) / eps (C-PCM), (eps - 1) / (eps + 1/2) (COSMO), 1 for a conductor
  energy       E_pcm = 1/2 q.v;  Fock term V_pcm = -sum_g q_g B_g  (variational: dE_pcm / dD = V_pcm)

B lives in HBM for the whole geometry ([n_points, ld] FP64, ld >= nao (nao + 1) / 2).  Each SCF cycle streams it twice
(`mi_pcm_potential`, `mi_pcm_fock`); the surface, S and its inverse, the nuclear potential and the host terms of the gradient
(dS/dx, dv_n/dx) are torch / NumPy."""
import math

import numpy as np
import torch

from .grids import lebedev
from .mole import BOHR
from .reference import require, wrap

# ---- the defaults, all [MEM] (entered from memory; not checked against PySCF or the papers) -------------------------------
DEFAULTS = {
    "method": "C-PCM",        # [MEM] PySCF's default; 'COSMO' differs only in f
    "eps": 78.3553,           # [MEM] water
    "lebedev_order": 29,      # [MEM] -> 302 points per atom
    "vdw_scale": 1.2,         # [MEM]
    "r_probe": 0.0,           # [MEM] Angstrom, added to the scaled radius
}
LEBEDEV_ORDER = {17: 110, 23: 194, 29: 302, 35: 434, 41: 590}   # [MEM] algebraic order -> points (the grids tabulated here)
# York-Karplus exponent factors xi_N per Lebedev grid [MEM]
XI = {110: 4.89825187392, 194: 4.90498088169, 302: 4.89752803365, 434: 4.89461452742, 590: 4.89548317724}
# Bondi van der Waals radii in Angstrom, H set to 1.10 ("modified Bondi") [MEM]
MODIFIED_BONDI = {1: 1.10, 2: 1.40, 3: 1.82, 5: 1.92, 6: 1.70, 7: 1.55, 8: 1.52, 9: 1.47, 10: 1.54, 11: 2.27, 12: 1.73,
                  14: 2.10, 15: 1.80, 16: 1.80, 17: 1.75, 18: 1.88, 19: 2.75, 35: 1.85, 36: 2.02, 53: 1.98, 54: 2.16}
SWF_DROP = 1e-16              # [MEM] points whose weight w_i R^2 swf_i is at or below this are dropped
METHODS = ("C-PCM", "CPCM", "COSMO")
REFUSED = ("IEF-PCM", "IEFPCM", "SS(V)PE", "SSVPE", "SMD")
BLOCK = 64                    # points per workgroup of the HIP kernels (one owning atom per block)


def scaling_factor(eps, method="C-PCM"):
    """f of the conductor-like screening: 1 for a conductor (eps = inf), 0 for vacuum (eps = 1)."""
    m = _method(method)
    eps = float(eps)
    if math.isinf(eps):
        return 1.0
    if m == "COSMO":
        return (eps - 1.0) / (eps + 0.5)
    return (eps - 1.0) / eps


def _method(method):
    key = str(method).upper().replace("_", "-")
    if key in REFUSED:
        raise NotImplementedError(f"solvent method '{method}' is not implemented (C-PCM and COSMO only)")
    if key not in METHODS:
        raise ValueError(f"unknown solvent method '{method}' (have C-PCM, COSMO)")
    return "COSMO" if key == "COSMO" else "C-PCM"


def switch_h(d):
    """SWIG switching polynomial h(d) = d^3 (10 - 15 d + 6 d^2) on [0, 1], clamped outside."""
    d = np.clip(d, 0.0, 1.0)
    return d ** 3 * (10.0 - 15.0 * d + 6.0 * d * d)


def switch_dh(d):
    inside = (d > 0.0) & (d < 1.0)
    return np.where(inside, 30.0 * d * d * (1.0 - d) ** 2, 0.0)


def switch_params(radii, ngrid):
    """(R_sw, R_in) per sphere for the switching function of an N-point sphere."""
    R = np.asarray(radii, dtype=np.float64)
    rsw = R * np.sqrt(14.0 / ngrid)
    alpha = 0.5 + R / rsw - np.sqrt((R / rsw) ** 2 - 1.0 / 28.0)
    return rsw, R - alpha * rsw


class Surface:
    """Switched Lebedev cavity: points `coords` [n,3] (Bohr), `owner` [n], `weight` (4 pi-normalised Lebedev weight),
    `swf`, `area` = weight R^2 swf, `zeta` (Gaussian exponent factor); `blocks` [nblk,3] = (first, count <= 64, owner)."""

    def __init__(self, atom_coords, radii, ngrid=302):
        if ngrid not in XI:
            raise NotImplementedError(f"Lebedev grid of {ngrid} points: no York-Karplus factor tabulated (have {sorted(XI)})")
        X = np.asarray(atom_coords, dtype=np.float64).reshape(-1, 3)
        R = np.asarray(radii, dtype=np.float64)
        self.atom_coords, self.radii, self.ngrid = X, R, ngrid
        unit, w = lebedev(ngrid)
        w = 4.0 * np.pi * np.asarray(w)
        rsw, rin = switch_params(R, ngrid)
        self.rsw, self.rin = rsw, rin
        pts, own, wt, sw, ze = [], [], [], [], []
        for ia in range(len(R)):
            p = X[ia] + R[ia] * unit                                # [N,3]
            r = np.linalg.norm(p[:, None, :] - X[None, :, :], axis=2)   # [N,natm]
            d = (r - rin[None, :]) / rsw[None, :]
            h = switch_h(d)
            h[:, ia] = 1.0
            swf = np.prod(h, axis=1)
            keep = w * R[ia] ** 2 * swf > SWF_DROP
            pts.append(p[keep]); own.append(np.full(int(keep.sum()), ia)); wt.append(w[keep]); sw.append(swf[keep])
            ze.append(XI[ngrid] / (R[ia] * np.sqrt(w[keep])))
        self.coords = np.concatenate(pts)
        self.owner = np.concatenate(own).astype(np.int64)
        self.weight = np.concatenate(wt)
        self.swf = np.concatenate(sw)
        self.zeta = np.concatenate(ze)
        self.area = self.weight * R[self.owner] ** 2 * self.swf
        blocks = []
        for ia in range(len(R)):
            idx = np.nonzero(self.owner == ia)[0]
            for s in range(0, idx.size, BLOCK):
                blocks.append((int(idx[s]), int(min(BLOCK, idx.size - s)), ia))
        self.blocks = np.asarray(blocks, dtype=np.int32).reshape(-1, 3)

    @property
    def npts(self):
        return self.coords.shape[0]


# ---- host pieces (torch: on the device in the SCF, on the CPU in the tests) ------------------------------------------------
_SQ2PI = math.sqrt(2.0 / math.pi)
_TSP = 2.0 / math.sqrt(math.pi)


def s_matrix(coords, zeta, swf):
    c = torch.as_tensor(coords, dtype=torch.float64)
    z = torch.as_tensor(zeta, dtype=torch.float64, device=c.device)
    s = torch.as_tensor(swf, dtype=torch.float64, device=c.device)
    r = torch.cdist(c, c)
    zz = z[:, None] * z[None, :] / torch.sqrt(z[:, None] ** 2 + z[None, :] ** 2)
    n = c.shape[0]
    eye = torch.eye(n, dtype=torch.bool, device=c.device)
    S = torch.erf(zz * r) / torch.where(eye, torch.ones_like(r), r)
    S[eye] = z * _SQ2PI / s
    return S


def _dphi(zeta, r):
    """d/dr [erf(zeta r) / r]."""
    return (_TSP * zeta * torch.exp(-(zeta * r) ** 2) * r - torch.erf(zeta * r)) / (r * r)


def v_nuc(coords, zeta, atom_coords, charges):
    """v_n,g = sum_A Z_A erf(zeta_g r_Ag) / r_Ag."""
    c = torch.as_tensor(coords, dtype=torch.float64)
    z = torch.as_tensor(zeta, dtype=torch.float64, device=c.device)
    X = torch.as_tensor(atom_coords, dtype=torch.float64, device=c.device)
    Z = torch.as_tensor(charges, dtype=torch.float64, device=c.device)
    r = torch.cdist(c, X)
    return (torch.erf(z[:, None] * r) / r) @ Z


def grad_vnuc(surf, charges, q, device="cpu"):
    """sum_g q_g dv_n,g / dR [natm,3]: the nuclei and the points (rigidly attached to their owners)."""
    c = torch.as_tensor(surf.coords, device=device)
    z = torch.as_tensor(surf.zeta, device=device)
    X = torch.as_tensor(surf.atom_coords, device=device)
    Z = torch.as_tensor(np.asarray(charges, dtype=np.float64), device=device)
    qq = torch.as_tensor(q, dtype=torch.float64, device=device)
    dv = X[None, :, :] - c[:, None, :]                          # R_A - s_g
    r = torch.linalg.norm(dv, dim=2)
    t = (qq[:, None] * Z[None, :] * _dphi(z[:, None], r) / r)[:, :, None] * dv   # d/dR_A of q_g Z_A phi(r_Ag)
    g = t.sum(dim=0)
    own = torch.as_tensor(surf.owner, device=device)
    g = g.index_add(0, own, -t.sum(dim=1))
    return g.cpu().numpy()


def grad_s(surf, q, device="cpu", rows=1024):
    """1/2 q^T (dS/dR) q [natm,3] (without the 1/f): off-diagonal erf terms and the diagonal through swf."""
    c = torch.as_tensor(surf.coords, device=device)
    z = torch.as_tensor(surf.zeta, device=device)
    qq = torch.as_tensor(q, dtype=torch.float64, device=device)
    own = torch.as_tensor(surf.owner, device=device)
    natm = surf.atom_coords.shape[0]
    gpt = torch.zeros(c.shape[0], 3, dtype=torch.float64, device=device)
    for i0 in range(0, c.shape[0], rows):
        i1 = min(i0 + rows, c.shape[0])
        d = c[i0:i1, None, :] - c[None, :, :]                   # s_i - s_j
        r = torch.linalg.norm(d, dim=2)
        zz = z[i0:i1, None] * z[None, :] / torch.sqrt(z[i0:i1, None] ** 2 + z[None, :] ** 2)
        self_ = torch.zeros_like(r, dtype=torch.bool)
        self_[torch.arange(i1 - i0, device=device), torch.arange(i0, i1, device=device)] = True
        rs = torch.where(self_, torch.ones_like(r), r)
        fac = torch.where(self_, torch.zeros_like(r), _dphi(zz, rs) / rs)
        # both S_ij and S_ji move with s_i: 2 x 1/2 q_i q_j dS_ij/ds_i
        gpt[i0:i1] += ((qq[i0:i1, None] * qq[None, :] * fac)[:, :, None] * d).sum(dim=1)
    g = torch.zeros(natm, 3, dtype=torch.float64, device=device).index_add(0, own, gpt).cpu().numpy()
    # diagonal: S_ii = zeta_i sqrt(2/pi) / swf_i, swf_i = prod_J h(d_iJ), d_iJ = (|s_i - R_J| - R_in,J) / R_sw,J
    P, X = surf.coords, surf.atom_coords
    dv = P[:, None, :] - X[None, :, :]
    r = np.linalg.norm(dv, axis=2)
    dd = (r - surf.rin[None, :]) / surf.rsw[None, :]
    h = switch_h(dd)
    dh = switch_dh(dd)
    owner = surf.owner
    h[np.arange(len(owner)), owner] = 1.0
    dh[np.arange(len(owner)), owner] = 0.0
    qn = np.asarray(q, dtype=np.float64)
    dSii_dswf = -surf.zeta * _SQ2PI / surf.swf ** 2
    # d swf_i / d s_i via atom J: swf_i dh/h (1/R_sw,J) (s_i - R_J)/r
    coef = (0.5 * qn ** 2 * dSii_dswf * surf.swf)[:, None] * dh / np.where(h > 0, h, 1.0) / surf.rsw[None, :] / r
    t = coef[:, :, None] * dv                                    # derivative w.r.t. s_i through atom J
    np.add.at(g, owner, t.sum(axis=1))
    g -= t.sum(axis=0)
    return g


def atom_radii_bohr(mol, vdw_scale=1.2, r_probe=0.0, radii_table=None, atom_radii=None):
    """Sphere radii in Bohr.  radii_table: indexed by nuclear charge, Bohr, used as given (vdw_scale and r_probe are not
    applied to it) [MEM]; atom_radii: {symbol: radius in Angstrom} replacing the table entry before scaling [MEM]."""
    out = np.zeros(mol.natm)
    for ia in range(mol.natm):
        zc = int(mol.atom_charge(ia))
        sym = mol.atom_pure_symbol(ia)
        if radii_table is not None:
            out[ia] = float(radii_table[zc])
            continue
        if atom_radii and sym in atom_radii:
            ra = float(atom_radii[sym])
        elif zc in MODIFIED_BONDI:
            ra = MODIFIED_BONDI[zc]
        else:
            raise NotImplementedError(f"no van der Waals radius tabulated for {sym}: set with_solvent.atom_radii")
        out[ia] = (ra * vdw_scale + r_probe) / BOHR
    return out


class PCMSolvent:
    """`mf.with_solvent`: parameters (eps, method, lebedev_order, vdw_scale, r_probe, radii_table, atom_radii) and, after
    `kernel()`, `e` (E_pcm, Hartree) and `q` (surface charges)."""

    def __init__(self, mol):
        self.mol = mol
        for k, v in DEFAULTS.items():
            setattr(self, k, v)
        self.radii_table = None
        self.atom_radii = None
        self.e = None
        self.q = None
        self.surface = None
        self._key = self._fkey = None
        self._B = None

    @property
    def f(self):
        return scaling_factor(self.eps, self.method)

    @property
    def ngrid(self):
        if self.lebedev_order not in LEBEDEV_ORDER:
            raise NotImplementedError(f"lebedev_order {self.lebedev_order}: have {sorted(LEBEDEV_ORDER)}")
        return LEBEDEV_ORDER[self.lebedev_order]

    def _geom_key(self, mol):
        rt = None if self.radii_table is None else tuple(np.asarray(self.radii_table, dtype=float).ravel().tolist())
        ar = None if not self.atom_radii else tuple(sorted(self.atom_radii.items()))
        return (id(mol), mol.atom_coords().tobytes(), self.lebedev_order, self.vdw_scale, self.r_probe, rt, ar)

    def build(self, eng, mol):
        """Surface, B (HIP kernel), S^-1 and v_n for `mol` on `eng`'s device; f S^-1 when eps/method changed."""
        _method(self.method)
        key = self._geom_key(mol)
        if key != self._key:
            self.mol = mol
            self._B = None
            radii = atom_radii_bohr(mol, self.vdw_scale, self.r_probe, self.radii_table, self.atom_radii)
            s = self.surface = Surface(mol.atom_coords(), radii, self.ngrid)
            dev = eng.device
            n = s.npts
            npair = eng.nao * (eng.nao + 1) // 2
            ld = (npair + 31) // 32 * 32
            need = 8 * n * ld
            free, _tot = torch.cuda.mem_get_info(dev)
            if need > 0.9 * free:
                raise NotImplementedError(f"PCM: the surface-charge integral store needs {need / 1e9:.1f} GB but {free / 1e9:.1f} GB "
                                          "of HBM are free (point-blocked recomputation is not implemented)")
            pts = np.concatenate([s.coords, s.zeta[:, None]], axis=1)
            self._pts = torch.as_tensor(np.ascontiguousarray(pts), device=dev)
            self._blk = torch.as_tensor(np.ascontiguousarray(s.blocks), device=dev)
            self._B = torch.empty(n, ld, dtype=torch.float64, device=dev)
            self.ld = ld
            eng.pcm_eval(self._pts, self._blk, ld, self._B)
            self._Sinv = torch.cholesky_inverse(torch.linalg.cholesky(s_matrix(self._pts[:, :3], self._pts[:, 3], torch.as_tensor(s.swf, device=dev))))
            self._vn = v_nuc(self._pts[:, :3], self._pts[:, 3], mol.atom_coords(), mol.atom_charges()).contiguous()
            self._dpack = torch.zeros(ld, dtype=torch.float64, device=dev)
            self._v = torch.empty(n, dtype=torch.float64, device=dev)
            self._part = torch.empty(eng.pcm_fock_chunks(n, ld) * ld, dtype=torch.float64, device=dev)
            self._eng = eng
            self._key, self._fkey = key, None
        fk = (float(self.eps), _method(self.method))
        if fk != self._fkey:
            self._K = (self.f * self._Sinv).contiguous()
            self._fkey = fk
        return self

    @property
    def nbytes(self):
        return 0 if self._B is None else self._B.numel() * 8

    def charges(self, dm):
        """(q, v, E_pcm) for the AO density `dm` (device tensors, no host synchronisation)."""
        eng = self._eng
        dm = dm.contiguous()
        eng.pcm_potential(self._B, self.ld, dm, self._dpack, self._vn, self._v)
        q = -(self._K @ self._v)
        return q, self._v, 0.5 * torch.dot(q, self._v).reshape(1)

    def fock_energy(self, dm, V, scale, accumulate=False):
        """V (+)= scale sum_g q_g B_g with q from `dm`: scale -1 gives V_pcm, -1/2 the unsymmetrised half the fused Fock
        assembly adds as V + V^T.  Returns E_pcm as a one-element device tensor."""
        q, _v, e = self.charges(dm)
        self._q_dev = q
        self._eng.pcm_fock(self._B, self.ld, q, scale, accumulate, self._part, V)
        return e

    def vpcm(self, dm):
        d = torch.as_tensor(dm, dtype=torch.float64, device=self._eng.device).contiguous()
        V = torch.empty_like(d)
        e = self.fock_energy(d, V, -1.0)
        return V, e

    def energy(self, dm):
        d = torch.as_tensor(dm, dtype=torch.float64, device=self._eng.device).contiguous()
        return float(self.charges(d)[2])

    def grad(self, dm):
        """dE_pcm/dR [natm,3] at fixed density: q^T dv/dR + 1/(2f) q^T dS/dR q (the orbital response is in the SCF's W)."""
        mol, s, eng = self.mol, self.surface, self._eng
        f = self.f
        natm = mol.natm
        if f == 0.0:
            return np.zeros((natm, 3))
        d = torch.as_tensor(dm, dtype=torch.float64, device=eng.device).contiguous()
        q, _v, _e = self.charges(d)
        # electronic part: -q_g D_mn dB_g,mn (HIP), per (ordered shell pair, point block); the point's share is minus the AO ones
        pairs = eng.pcm_pairs(ordered=True)
        nblk = s.blocks.shape[0]
        part = torch.empty(pairs.shape[0] * nblk * 3, dtype=torch.float64, device=eng.device)
        eng.pcm_grad(self._pts, self._blk, d, q.contiguous(), part)
        part = part.view(pairs.shape[0], nblk, 3)
        per_pair = part.sum(dim=1).cpu().numpy()
        per_blk = part.sum(dim=0).cpu().numpy()
        g = np.zeros((natm, 3))
        shell_atom = np.asarray(mol._bas[:, 0], dtype=np.int64)
        np.add.at(g, shell_atom[pairs[:, 0]], per_pair)
        np.add.at(g, s.blocks[:, 2].astype(np.int64), -per_blk)
        qh = q.cpu().numpy()
        g += grad_vnuc(s, mol.atom_charges(), qh, device=eng.device)
        g += grad_s(s, qh, device=eng.device) / f
        return g


class _PCMMixin:
    """Methods a PCM-wrapped SCF object gains (the class is made at run time: `PCM(mf)`)."""
    _pcm = True

    # the template sets mf.eps / mf.method on the wrapped object: forwarded to with_solvent (whether PySCF itself forwards
    # them could not be checked offline [MEM])
    @property
    def eps(self):
        return self.with_solvent.eps

    @eps.setter
    def eps(self, v):
        self.with_solvent.eps = v

    @property
    def method(self):
        return self.with_solvent.method

    @method.setter
    def method(self, v):
        self.with_solvent.method = v

    def _setup(self):
        self.with_solvent.build(self.engine, self.mol)      # B is allocated before the ERI planner looks at free HBM
        super()._setup()

    def kernel(self, dm0=None, **kw):
        self._setup_once()
        self.with_solvent.build(self.engine, self.mol)
        e = super().kernel(dm0=dm0, **kw)
        ws = self.with_solvent
        q, _v, ep = ws.charges(self._dm)
        ws.e, ws.q = float(ep), q.cpu().numpy()
        return e

    scf = kernel

    def energy_tot(self, dm=None, h1e=None, vhf=None):
        if dm is None:
            return self.e_tot
        self._setup_once()
        self.with_solvent.build(self.engine, self.mol)
        return super().energy_tot(dm) + self.with_solvent.energy(dm)

    def nuc_grad_method(self):
        return PCMGradients(self)

    Gradients = nuc_grad_method

    def TDA(self):
        raise NotImplementedError("TDA / TDDFT with PCM (non-equilibrium solvation) is not implemented")

    TDHF = TDDFT = TDA

    def PCM(self):
        return self


def _grad_base():
    from .grad import Gradients
    return Gradients


class PCMGradients(_grad_base()):
    """Analytic gradient of a PCM-wrapped RHF/RKS: the vacuum terms (whose W already holds V_pcm through the Fock matrix)
    plus q^T dv/dR + 1/(2f) q^T dS/dR q."""

    def kernel(self, mo_energy=None, mo_coeff=None, mo_occ=None, atmlst=None):
        de = super().kernel(mo_energy, mo_coeff, mo_occ, atmlst)
        mf = self.base
        de = de + mf.with_solvent.grad(mf._dm)
        self.de = de
        return de

    grad = kernel


_CLASSES = {}


def PCM(mf, **params):
    """`solvent.PCM(mf)`: the SCF object wrapped for C-PCM (an instance of a subclass of mf's class made at run time, sharing
    mf's state).  Closed shells (RHF / RKS), one rank."""
    if isinstance(mf, _PCMMixin):
        return mf
    require(mf, "PCM")
    new = wrap(mf, _PCMMixin, "PCM", _CLASSES, with_solvent=PCMSolvent(mf.mol))
    for k, v in params.items():
        setattr(new.with_solvent, k, v)
    _method(new.with_solvent.method)
    return new
