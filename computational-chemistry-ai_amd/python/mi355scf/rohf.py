"""Spin-restricted open-shell SCF behind `pyscf.scf.ROHF` / `gpu4pyscf.scf.ROHF` and `dft.ROKS` (call sites
`templates/calculate_casscf.py:61-64`: `scf.ROHF(mol)` for every molecule with `spin != 0`;
`templates/calculate_reaction_energy.py:167`).

One orbital set C: the first n_beta orbitals are doubly occupied (closed), the next n_alpha - n_beta singly (open), the rest
empty.  Da = C[:, :na] C[:, :na]^T, Db = C[:, :nb] C[:, :nb]^T; the Fock pair (Fa, Fb) and the energy are those of UHF / UKS on
(Da, Db) (`UHF._fock_pair`, `UKS._fock_pair`: one `mi_build_jk(n_dm = 2)` pass, spin V_xc).  What is new is the coupling:
`mi_rohf_fock` turns C^T Fa C and C^T Fb C into Roothaan's effective Fock operator (PySCF's default coefficients)

              closed   open   virtual
    closed      Fc      Fb      Fc                Fc = (Fa + Fb) / 2
    open        Fb      Fc      Fa
    virtual     Fc      Fa      Fc

and into the orbital gradient G (the closed-open block of Fb, the open-virtual block of Fa, the closed-virtual block of Fc, signed
like F n - n F) with the partial sums of |G|^2.  The loop is UHF's plain loop (`UHF._plain_start`, `_plain_step`, `_ufinal`): CDIIS
(`PairDIIS`) extrapolates the one matrix S C F_eff C^T S with the error vector S C G C^T S, and the new orbitals come from one
`eigh` of it per cycle in the Cholesky-orthogonalised basis.  The two nested densities are not purified (DESIGN.md section 14 names
that as the follow-up).

Refused (NotImplementedError, never approximated): rows "ROHF / ROKS", "density_fit()" and "shard()" of `reference.SUPPORT`; the
"rohf" entries of the other rows are the methods that do not take an ROHF reference.  `mcscf.CASCI` accepts ROHF (not ROKS).
"""
import ctypes

import numpy as np
import torch

from . import engine as _engine
from .reference import require
from .uhf import UHF
from .uks import UKS


def rohf_fock(fa, fb, ncore, nopen, nmo=None):
    """(F_eff, G, part) from `mi_rohf_fock` for the MO-basis Fock matrices fa, fb: FP64 device tensors [nmo, ld] with unit column
    stride (views of padded rows are taken as they are).  F_eff and G have the layout of `fa`; columns >= nmo of their rows are not
    written.  part[:nb] holds partial sums of G^2 and part[nb:] partial maxima of |G|, nb = mi_rohf_fock_blocks()."""
    nmo = fa.shape[0] if nmo is None else int(nmo)
    for x in (fa, fb):
        if not (x.is_cuda and x.dtype == torch.float64 and x.dim() == 2 and x.stride(1) == 1):
            raise ValueError("mi_rohf_fock: float64 device matrices with unit column stride are required")
    ld = fa.stride(0)
    if fb.stride(0) != ld or fa.shape != fb.shape or fa.shape[0] < nmo or fa.shape[1] < nmo or ld < nmo:
        raise ValueError("mi_rohf_fock: fa and fb must share shape and leading dimension")
    L = _engine.lib()
    feff = torch.empty_strided(fa.shape, fa.stride(), dtype=fa.dtype, device=fa.device)
    g = torch.empty_strided(fa.shape, fa.stride(), dtype=fa.dtype, device=fa.device)
    part = torch.empty(2 * int(L.mi_rohf_fock_blocks()), dtype=torch.float64, device=fa.device)
    with torch.cuda.device(fa.device):
        stream = ctypes.c_void_p(torch.cuda.current_stream(fa.device).cuda_stream)
        _engine._check(L.mi_rohf_fock(fa.data_ptr(), fb.data_ptr(), ld, int(ncore), int(nopen), nmo, feff.data_ptr(), g.data_ptr(),
                                      part.data_ptr(), stream))
    return feff, g, part


class _MOEnergy(np.ndarray):
    """Eigenvalues of F_eff carrying the per-spin diagonals C^T Fa C, C^T Fb C as `.mo_ea` / `.mo_eb` (as PySCF's ROHF)."""
    mo_ea = mo_eb = None

    def __array_finalize__(self, obj):
        # views and copies of the whole vector keep the diagonals; anything of another length (slices, reductions) drops them
        keep = obj is not None and getattr(obj, "shape", None) == self.shape
        self.mo_ea = getattr(obj, "mo_ea", None) if keep else None
        self.mo_eb = getattr(obj, "mo_eb", None) if keep else None


class ROHF(UHF):
    _rohf = True
    _purify_spins = False    # one `eigh` of F_eff per cycle at every size: the two nested densities are not purified
    # (`_spin_restricted` stays False as for UHF: every consumer that needs a closed shell -- PCM, TDA / TDDFT, CCSD -- refuses)

    # --- densities and occupations --------------------------------------------------------------
    def _classes(self):
        """(ncore, nopen) = (n_beta, n_alpha - n_beta)."""
        na, nb = self.mol.nelec
        return nb, na - nb

    def make_rdm1(self, mo_coeff=None, mo_occ=None):
        """The (Da, Db) stack [2, N, N]."""
        if mo_coeff is None:
            if self._dm is not None:
                return self._dm.cpu().numpy()
            mo_coeff, mo_occ = self.mo_coeff, self.mo_occ
        c, occ = np.asarray(mo_coeff), np.asarray(mo_occ)
        ca, cb = c[:, occ > 0], c[:, occ > 1]
        return np.stack([ca @ ca.T, cb @ cb.T])

    def spin_square(self, mo_coeff=None, s=None):
        """<S^2> = S (S + 1) and 2S + 1 of the high-spin ROHF determinant (exact: the beta orbitals lie in the alpha space)."""
        ncore, nopen = self._classes()
        sz = 0.5 * nopen
        return sz * (sz + 1.0), 2.0 * sz + 1.0

    # --- the plain loop's hooks -----------------------------------------------------------------
    def kernel(self, dm0=None, **kw):
        require(self, "ROHF / ROKS")
        return self._run(dm0, fast=False)

    scf = kernel

    def _udm0(self, dm0):
        """The starting densities must be the nested pair of ONE orbital set (the coupling works in its MO basis): the orbitals
        of the guess's mean Fock matrix (Fa + Fb) / 2, occupied aufbau."""
        na, nb = self.nelec
        F, _ = self._fock_pair(UHF._udm0(self, dm0))
        _e, c = self._uorbitals((0.5 * (F[0] + F[1])).unsqueeze(0))
        ca, cb = c[0][:, :na], c[0][:, :nb]
        return torch.stack([ca @ ca.T, cb @ cb.T])

    def _uorbitals(self, F):
        """Orbitals of the one matrix in `F` ([1, N, N]); they stay on the object as the MO basis of the next coupling."""
        e, c = UHF._uorbitals(self, F)
        self._mo_dev = c[0]
        return e, c

    def _diis_pair(self, F, dm):
        """F_eff and the orbital-gradient error vector of the Fock pair F, both back in the AO basis ([1, N, N] stacks), and
        |G|^2 from the kernel's partial sums.  The MO basis is the orbital set `dm` was made from."""
        C = self._mo_dev
        ncore, nopen = self._classes()
        SC = self._S @ C
        fmo = torch.matmul(C.T.unsqueeze(0), F @ C)
        feff, g, part = rohf_fock(fmo[0], fmo[1], ncore, nopen)
        back = torch.matmul(SC.unsqueeze(0), torch.stack([feff, g]) @ SC.T)
        return back[:1], back[1:], part[:part.numel() // 2].sum()

    def _shift_densities(self, dm):
        return (0.5 * (dm[0] + dm[1])).unsqueeze(0)      # PySCF: the open shell is raised by half the shift

    def _n_rotations(self):
        n = self.engine.nao
        ncore, nopen = self._classes()
        nvir = n - ncore - nopen
        return max(ncore * nopen + nopen * nvir + ncore * nvir, 1)

    def _set_orbitals(self, dm, F, mo_e, mo_c):
        """The one orbital set with occupations 2 / 1 / 0; `mo_energy` carries the per-spin diagonals of the Fock pair F."""
        ncore, nopen = self._classes()
        C = mo_c[0]
        e = mo_e[0].cpu().numpy().view(_MOEnergy)
        e.mo_ea, e.mo_eb = (torch.einsum("pi,spq,qi->si", C, F, C).cpu().numpy())
        self.mo_energy = e
        self.mo_coeff = C.cpu().numpy()
        occ = np.zeros(self.engine.nao)
        occ[:ncore] = 2.0
        occ[ncore:ncore + nopen] = 1.0
        self.mo_occ = occ


class ROKS(ROHF, UKS):
    """Restricted open-shell Kohn-Sham: the ROHF coupling on the UKS Fock pair and energy (`UKS._fock_pair`)."""
