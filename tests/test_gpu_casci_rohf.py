"""`mcscf.CASCI` on an engine ROHF reference: the single-determinant space reproduces the ROHF energy, and roots and <S^2> of a
radical agree with the dense determinant Hamiltonian of `test_fci_host.py` built from the oracle's integrals in the engine's
orbitals (energies to 1e-8, <S^2> to 1e-7: the margins of `test_gpu_casci.py`)."""
import functools

import numpy as np
import pytest

from test_fci_host import ref_hamiltonian, ref_s2
from test_rohf_host import O2, OH, mol_of, oracle_integrals

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _rohf(atom, spin):
    from pyscf import scf
    mol = mol_of(atom, "sto-3g" if atom == O2 else "6-31g(d)", spin)
    mf = scf.ROHF(mol)
    mf.conv_tol = 1e-11
    mf.kernel()
    assert mf.converged
    return mol, mf


def test_single_determinant_space_is_the_rohf_state():
    """O2 triplet / STO-3G: CASCI(mf, 2, 2) unpacks to (2, 0), one determinant: E(CASCI) == E(ROHF), <S^2> = 2."""
    from pyscf import mcscf
    mol, mf = _rohf(O2, 2)
    mc = mcscf.CASCI(mf, 2, 2)
    e_tot, e_cas, ci, mo, mo_e = mc.kernel()
    ss, mult = mc.fcisolver.spin_square(ci, 2, mc.nelecas)
    print(f"O2 CAS(2,2): E(CASCI) - E(ROHF) = {e_tot - mf.e_tot:.2e}, <S^2> = {ss:.10f}, CI shape {np.shape(ci)}")
    assert mc.nelecas == (2, 0) and mc.ncore == 7 and np.shape(ci) == (1, 1) and mc.converged
    assert abs(e_tot - mf.e_tot) <= 1e-9 and abs(ss - 2.0) <= 1e-10 and abs(mult - 3.0) <= 1e-10
    # F_eff is (Fa + Fb) / 2 = h + J - K / 2 of the spin-summed density on its diagonal blocks: the Fock diagonal CASCI reports
    assert np.abs(mo_e - np.asarray(mf.mo_energy)).max() < 1e-5


def test_roots_and_spin_of_a_radical():
    """OH / 6-31G(d), CASCI(mf, 4, 3) -> (2, 1), three roots against the dense reference; the ROHF determinant lies in the space."""
    from pyscf import mcscf
    mol, mf = _rohf(OH, 1)
    ncas, nroots = 4, 3
    mc = mcscf.CASCI(mf, ncas, 3)
    mc.fcisolver.nroots = nroots
    e_tot, e_cas, ci, mo, mo_e = mc.kernel()
    assert mc.nelecas == (2, 1) and mc.ncore == 3
    S, h, eri = oracle_integrals(mol)
    mo = np.asarray(mo)
    Cc, Ca = mo[:, :mc.ncore], mo[:, mc.ncore:mc.ncore + ncas]
    Dc = 2.0 * Cc @ Cc.T
    Vc = np.einsum("ijkl,kl->ij", eri, Dc) - 0.5 * np.einsum("ikjl,kl->ij", eri, Dc)
    e_core = mol.energy_nuc() + np.sum(Dc * (h + 0.5 * Vc))
    H = ref_hamiltonian(Ca.T @ (h + Vc) @ Ca, np.einsum("ijkl,it,ju,kv,lw->tuvw", eri, Ca, Ca, Ca, Ca, optimize=True), ncas, mc.nelecas)
    w, U = np.linalg.eigh(H)
    S2 = ref_s2(ncas, mc.nelecas)
    ref_e = w[:nroots] + e_core
    ref_ss = np.array([U[:, i] @ S2 @ U[:, i] for i in range(nroots)])
    ss = np.array([mc.fcisolver.spin_square(c, ncas, mc.nelecas)[0] for c in ci])
    err_e, err_s = np.abs(np.asarray(e_tot) - ref_e).max(), np.abs(ss - ref_ss).max()
    print(f"OH CAS(3,4): E {np.asarray(e_tot)}, worst |E - E_ref| {err_e:.2e}, <S^2> {np.round(ss, 6)} (reference {np.round(ref_ss, 6)}), "
          f"worst error {err_s:.2e}, E_0 - E(ROHF) = {e_tot[0] - mf.e_tot:.2e}")
    assert len(e_tot) == nroots and len(ci) == nroots and abs(e_core - mc.e_core) <= 1e-8
    assert err_e <= 1e-8 and err_s <= 1e-7
    assert e_tot[0] <= mf.e_tot + 1e-10
    assert np.abs(mo_e - np.asarray(mf.mo_energy)).max() < 1e-5


def test_open_shell_core_and_roks_are_refused():
    from pyscf import dft, mcscf
    mol, mf = _rohf(O2, 2)
    with pytest.raises(NotImplementedError, match="singly occupied orbital"):
        mcscf.CASCI(mf, 1, (1, 1))
    ks = dft.ROKS(mol)
    ks.xc = "b3lyp"
    with pytest.raises(NotImplementedError):
        mcscf.CASCI(ks, 2, 2)
    with pytest.raises(NotImplementedError):
        mcscf.CASSCF(mf, 2, 2)
