"""Complete-active-space CI behind `pyscf.mcscf.CASCI(mf, ncas, nelecas)` (`templates/calculate_casscf.py:121-137`, the
`--casci-only` branch) for a converged closed-shell RHF, or an ROHF whose singly occupied orbitals all lie in the active block, on
one GPU with the resident, unsharded, full-Coulomb ERI store.

    F^I, E_core                                         frozen-core Fock matrix and energy of the `ncore` doubly occupied
                                                        orbitals, one J/K pass over the resident tiles (`ao2mo.core_fock`)
    h_act  = Ca^T F^I Ca
    (tu|vw)                                             `ao2mo.transform` of the active block, then `ao2mo.symmetrize8`
    E_tot  = E_core + lowest eigenvalue(s) of the active-space Hamiltonian      (`fci.FCISolver`)

`kernel()` returns PySCF's 5-tuple (e_tot, e_cas, ci, mo_coeff, mo_energy); with `fcisolver.nroots > 1` the energies are arrays
and `ci` a list.  `natorb = True` rotates the active block to the natural orbitals of state 0 (occupations descending), solves the
CI again in them (so `ci` belongs to the returned `mo_coeff`) and fills `mo_occ`.  There is no canonicalisation: `mo_energy` is
the diagonal of the reference's Fock matrix in the returned orbitals.

Not implemented (refused with NotImplementedError, never approximated): the references of row "CASCI" of `reference.SUPPORT`, an
open-shell core, direct-mode references.  Orbital optimisation and state averaging are `casscf.CASSCF` (re-exported here).
"""
import sys

import numpy as np
import torch

from . import fci
from .ao2mo import core_fock, resident_engine, symmetrize8, transform
from .reference import require


class CASCI:
    natorb = False

    def __init__(self, mf, ncas, nelecas, ncore=None):
        ref = require(mf, "CASCI")
        self._scf = mf
        self.mol = mf.mol
        self.verbose = mf.verbose
        self.stdout = getattr(mf, "stdout", None)
        self.ncas = int(ncas)
        spin = int(getattr(self.mol, "spin", 0))
        if spin and isinstance(nelecas, (int, np.integer)):
            # PySCF: an electron count on an open-shell molecule takes the molecule's 2 Ms
            if (int(nelecas) + spin) % 2 or int(nelecas) < spin:
                raise ValueError(f"CASCI: {nelecas} active electrons cannot carry the molecule's spin = {spin}")
            nelecas = ((int(nelecas) + spin) // 2, (int(nelecas) - spin) // 2)
        self.nelecas = fci._unpack_nelec(nelecas)
        nel = int(self.mol.nelectron)
        ncore_el = nel - sum(self.nelecas)
        nmo = None if mf.mo_coeff is None else np.asarray(mf.mo_coeff).shape[1]
        if self.ncas < 1 or min(self.nelecas) < 0 or max(self.nelecas) > self.ncas:
            raise NotImplementedError(f"CASCI: {self.nelecas} electrons do not fit in {self.ncas} active orbitals")
        if ncore_el < 0 or ncore_el % 2:
            raise NotImplementedError(f"CASCI: {sum(self.nelecas)} active electrons leave {ncore_el} core electrons of the molecule's "
                                      f"{nel}: the core must be closed-shell")
        if ncore is not None and 2 * int(ncore) != ncore_el:
            raise NotImplementedError(f"CASCI: ncore = {ncore} with {sum(self.nelecas)} active electrons does not give the molecule's "
                                      f"{nel} electrons")
        self.ncore = ncore_el // 2
        if self.ncas > fci.MAX_NORB:
            raise NotImplementedError(f"CASCI: ncas = {self.ncas}; the FCI solver holds at most {fci.MAX_NORB} orbitals")
        if nmo is not None and self.ncore + self.ncas > nmo:
            raise NotImplementedError(f"CASCI: ncore + ncas = {self.ncore + self.ncas} exceeds the {nmo} molecular orbitals")
        if ref.spin == "rohf":
            na, nb = self.mol.nelec
            for i in range(nb, na):          # the core density is built closed-shell: no singly occupied orbital may fall outside
                if not self.ncore <= i < self.ncore + self.ncas:
                    raise NotImplementedError(f"CASCI: the singly occupied orbital {i} of the ROHF reference lies outside the active "
                                              f"block [{self.ncore}, {self.ncore + self.ncas}): an open-shell core is not supported")
        self.fcisolver = fci.FCISolver(self.mol)
        self.e_tot = self.e_cas = self.ci = None
        self.mo_coeff = mf.mo_coeff
        self.mo_energy = mf.mo_energy
        self.mo_occ = None
        self.converged = False
        self.e_core = None

    def _log(self, level, msg):
        if self.verbose >= level:
            (self.stdout or sys.stdout).write(msg + "\n")

    # ---- orbital choice -------------------------------------------------------------------------------------------------------
    def sort_mo(self, caslst, mo_coeff=None, base=1):
        """Orbitals reordered as PySCF's `sort_mo`: the `ncore` lowest orbitals outside `caslst`, then `caslst` (indices counted
        from `base`) as the active block, then the rest."""
        mo = np.asarray(self.mo_coeff if mo_coeff is None else mo_coeff)
        cas = [int(i) - base for i in caslst]
        if len(cas) != self.ncas or len(set(cas)) != len(cas) or min(cas) < 0 or max(cas) >= mo.shape[1]:
            raise ValueError(f"sort_mo: caslst must name {self.ncas} distinct orbitals in [{base}, {mo.shape[1] + base})")
        rest = [i for i in range(mo.shape[1]) if i not in set(cas)]
        order = rest[:self.ncore] + cas + rest[self.ncore:]
        return mo[:, order]

    # ---- integrals ------------------------------------------------------------------------------------------------------------
    def _prepare(self, mo):
        eng = resident_engine(self._scf, "CASCI")
        C = torch.as_tensor(np.ascontiguousarray(mo), dtype=torch.float64, device=eng.device)
        if C.shape[0] != eng.nao or self.ncore + self.ncas > C.shape[1]:
            raise ValueError(f"CASCI: mo_coeff of shape {tuple(C.shape)} for {eng.nao} AOs, ncore + ncas = {self.ncore + self.ncas}")
        Ca = C[:, self.ncore:self.ncore + self.ncas].contiguous()
        heff, e_core = core_fock(self._scf, C, self.ncore)
        h_act = Ca.T @ heff @ Ca
        eri = symmetrize8(transform(eng, Ca, Ca, [(Ca, Ca)])[0])          # (t u|v w); the store is screened
        h_act = 0.5 * (h_act + h_act.T)
        return h_act.cpu().numpy(), eri.cpu().numpy(), e_core, C

    def _fock_diagonal(self, C):
        """Diagonal of the reference's Fock matrix in the orbitals C (the reference's own orbital energies when C is a
        reordering of its orbitals)."""
        mf = self._scf
        D = torch.as_tensor(np.asarray(mf.make_rdm1()), dtype=torch.float64, device=C.device)
        if D.dim() == 3:                     # ROHF: the spin-summed density, RHF-style J - K / 2
            D = (D[0] + D[1]).contiguous()
        J, K = mf._jk(D)
        return torch.einsum("pi,pq,qi->i", C, mf._h1 + J - 0.5 * K, C).cpu().numpy()

    def get_h1eff(self, mo_coeff=None):
        """(h_act, E_core) as PySCF's `CASCI.get_h1eff`."""
        h, _, ec, _ = self._prepare(np.asarray(self.mo_coeff if mo_coeff is None else mo_coeff))
        return h, ec

    def get_h2eff(self, mo_coeff=None):
        """(tu|vw) as a 4-index array."""
        return self._prepare(np.asarray(self.mo_coeff if mo_coeff is None else mo_coeff))[1]

    # ---- driver ---------------------------------------------------------------------------------------------------------------
    def kernel(self, mo_coeff=None, ci0=None):
        mf = self._scf
        if mf.mo_coeff is None:
            mf.kernel()
        if not getattr(mf, "converged", True):
            self._log(2, "CASCI: the reference SCF is not converged")
        if mo_coeff is None:
            mo_coeff = self.mo_coeff if self.mo_coeff is not None else mf.mo_coeff
        mo = np.array(mo_coeff, dtype=np.float64)
        nmo = mo.shape[1]
        if self.ncore + self.ncas > nmo:
            raise NotImplementedError(f"CASCI: ncore + ncas = {self.ncore + self.ncas} exceeds the {nmo} molecular orbitals")
        h_act, eri, e_core, C = self._prepare(mo)
        self._log(4, f"CASCI: ncore = {self.ncore}, ncas = {self.ncas}, nelecas = {self.nelecas}, E_core = {e_core:.12f}")
        sol = self.fcisolver
        e_tot, ci = sol.kernel(h_act, eri, self.ncas, self.nelecas, ci0=ci0, ecore=e_core)
        act = slice(self.ncore, self.ncore + self.ncas)
        mo_occ = None
        if self.natorb:
            c0 = ci[0] if isinstance(ci, list) else ci
            occ, U = np.linalg.eigh(-sol.make_rdm1(c0, self.ncas, self.nelecas))
            U = U * np.where(U[np.abs(U).argmax(axis=0), np.arange(self.ncas)] < 0, -1.0, 1.0)[None, :]
            mo[:, act] = mo[:, act] @ U
            h_act = U.T @ h_act @ U
            eri = np.einsum("pqrs,pt,qu,rv,sw->tuvw", eri, U, U, U, U, optimize=True)
            e_tot, ci = sol.kernel(h_act, eri, self.ncas, self.nelecas, ecore=e_core)
            mo_occ = np.zeros(nmo)
            mo_occ[:self.ncore] = 2.0
            mo_occ[act] = -occ
            C = torch.as_tensor(mo, dtype=torch.float64, device=C.device)
        mo_energy = self._fock_diagonal(C)
        self.e_tot, self.ci, self.e_core = e_tot, ci, e_core
        self.e_cas = e_tot - e_core
        self.mo_coeff, self.mo_energy, self.mo_occ = mo, mo_energy, mo_occ
        self.converged = bool(np.all(sol.converged))
        for i, e in enumerate(np.atleast_1d(e_tot)):
            self._log(3, f"CASCI state {i}: E = {e:.12f}  E(CI) = {e - e_core:.12f}")
        return self.e_tot, self.e_cas, self.ci, self.mo_coeff, self.mo_energy

    casci = kernel

    def make_rdm1(self, mo_coeff=None, ci=None, state=0):
        """Total AO density matrix of one state: core 2 Cc Cc^T plus the active-space one-particle density."""
        if self.ci is None and ci is None:
            self.kernel()
        mo = np.asarray(self.mo_coeff if mo_coeff is None else mo_coeff)
        ci = self.ci if ci is None else ci
        c = ci[state] if isinstance(ci, list) else ci
        dm_act = self.fcisolver.make_rdm1(c, self.ncas, self.nelecas)
        Cc, Ca = mo[:, :self.ncore], mo[:, self.ncore:self.ncore + self.ncas]
        return 2.0 * Cc @ Cc.T + Ca @ dm_act @ Ca.T

    # ---- nuclear gradients (casscf_grad.py: state-specific CASSCF only; a CASCI or state-averaged object is refused there) -----
    def nuc_grad_method(self):
        from . import casscf_grad
        return casscf_grad.Gradients(self)

    Gradients = nuc_grad_method


def __getattr__(name):
    """`CASSCF` (orbital optimisation, `casscf.py`) subclasses `CASCI` above, so it is imported on first use."""
    if name == "CASSCF":
        from .casscf import CASSCF
        return CASSCF
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
