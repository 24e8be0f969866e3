"""`mcscf.CASCI` on the engine against a reference assembled from the CPU oracle's integrals (`oracle.Oracle(mol).int1e()`,
`eri_full()`) transformed with the engine's own orbitals and diagonalised by the dense determinant reference of
`test_fci_host.py`.  Energies are compared to 1e-8 -- the engine-versus-oracle margin `test_gpu_rsh.py` uses for energies --
and <S^2> to 1e-7.  Molecules come from `conftest.MOLECULES`; H2 (not in that table) is 0.74 Angstrom along z."""
import functools

import numpy as np
import pytest

from conftest import MOLECULES
from test_fci_host import ref_hamiltonian, ref_s2

pytestmark = pytest.mark.gpu

H2 = "H 0 0 0; H 0 0 0.74"


@functools.lru_cache(maxsize=None)
def _rhf(name, basis):
    from pyscf import gto, scf
    mol = gto.M(atom=MOLECULES.get(name, H2), basis=basis, verbose=0)
    mf = scf.RHF(mol)
    mf.conv_tol = 1e-11
    mf.kernel()
    assert mf.converged
    return mol, mf


@functools.lru_cache(maxsize=None)
def _oracle_integrals(name, basis):
    from oracle import oracle as orc
    mol, _ = _rhf(name, basis)
    o = orc.Oracle(mol)
    S, T, V, _ = o.int1e()
    return S, T + V, o.eri_full()


def _reference(name, basis, mo, ncore, ncas, nelecas, nroots):
    """(energies, <S^2>) of the lowest roots from oracle integrals in the orbitals `mo`."""
    mol, _ = _rhf(name, basis)
    S, h, eri = _oracle_integrals(name, basis)
    Cc, Ca = mo[:, :ncore], mo[:, ncore:ncore + ncas]
    Dc = 2.0 * Cc @ Cc.T
    Vc = np.einsum("ijkl,kl->ij", eri, Dc) - 0.5 * np.einsum("ikjl,kl->ij", eri, Dc)
    e_core = mol.energy_nuc() + np.sum(Dc * (h + 0.5 * Vc))
    h_act = Ca.T @ (h + Vc) @ Ca
    e_act = np.einsum("ijkl,it,ju,kv,lw->tuvw", eri, Ca, Ca, Ca, Ca, optimize=True)
    H = ref_hamiltonian(h_act, e_act, ncas, nelecas)
    w, U = np.linalg.eigh(H)
    S2 = ref_s2(ncas, nelecas)
    ss = np.array([U[:, i] @ S2 @ U[:, i] for i in range(min(nroots, len(w)))])
    return w[:nroots] + e_core, ss


@pytest.mark.parametrize("ncas", [2, 4])
def test_fully_occupied_active_space_is_the_rhf_determinant(ncas):
    """CASCI(mf, ncas, 2 ncas) has one determinant: E_core, V_core and the active integrals must add up to the SCF energy."""
    from pyscf import mcscf
    mol, mf = _rhf("h2o", "6-31g(d)")
    mc = mcscf.CASCI(mf, ncas, 2 * ncas)
    e_tot = mc.kernel()[0]
    print(f"ncore {mc.ncore}, ncas {ncas}: E(CASCI) - E(RHF) = {e_tot - mf.e_tot:.2e}")
    assert mc.ncore == 5 - ncas and mc.nelecas == (ncas, ncas) and abs(e_tot - mf.e_tot) <= 1e-9 and mc.converged
    assert abs(mc.e_cas + mc.e_core - e_tot) < 1e-12


def test_full_ci_of_h2():
    from pyscf import mcscf, fci
    mol, mf = _rhf("h2", "6-31g(d,p)")
    nmo = np.asarray(mf.mo_coeff).shape[1]
    mc = mcscf.CASCI(mf, nmo, 2)
    e_tot, e_cas, ci, mo, mo_e = mc.kernel()
    ref, _ = _reference("h2", "6-31g(d,p)", np.asarray(mo), 0, nmo, (1, 1), 1)
    e_fci, ci_fci = fci.FCI(mf).kernel()
    print(f"H2/6-31G(d,p) full CI ({nmo} orbitals): E - E_ref = {e_tot - ref[0]:.2e}, fci.FCI(mf) - E_ref = {e_fci - ref[0]:.2e}, "
          f"correlation energy {e_tot - mf.e_tot:.6f}")
    assert mc.ncore == 0 and abs(e_tot - ref[0]) <= 1e-8 and abs(e_fci - ref[0]) <= 1e-8
    assert e_tot <= mf.e_tot + 1e-10 and ci.shape == (nmo, nmo) == ci_fci.shape
    assert np.abs(mo_e - np.asarray(mf.mo_energy)).max() < 1e-5     # Fock diagonal at the converged density vs the SCF's eigenvalues


CAS_CASES = [("h2o", 4, 4, None), ("h2o", 5, 6, None), ("h2co", 2, 2, (7, 9))]


@pytest.mark.parametrize("name,ncas,nelecas,caslst", CAS_CASES)
def test_cas_roots_spin_and_natural_orbitals(name, ncas, nelecas, caslst):
    from pyscf import mcscf
    basis = "6-31g(d)"
    mol, mf = _rhf(name, basis)
    nroots = 4
    mc = mcscf.CASCI(mf, ncas, nelecas)
    mc.fcisolver.nroots = nroots
    mo0 = mc.sort_mo(caslst) if caslst else None
    e_tot, e_cas, ci, mo, mo_e = mc.kernel(mo0)
    nel = (nelecas // 2, nelecas // 2)
    ref_e, ref_ss = _reference(name, basis, np.asarray(mo), mc.ncore, ncas, nel, nroots)
    ss = np.array([mc.fcisolver.spin_square(c, ncas, mc.nelecas)[0] for c in ci])
    err_e, err_s = np.abs(np.asarray(e_tot) - ref_e).max(), np.abs(ss - ref_ss).max()
    print(f"{name} CAS({nelecas},{ncas}): E {np.asarray(e_tot)}, worst |E - E_ref| {err_e:.2e}, <S^2> {np.round(ss, 6)}, worst error {err_s:.2e}")
    assert len(e_tot) == nroots and len(ci) == nroots and mc.nelecas == nel
    assert err_e <= 1e-8 and err_s <= 1e-7
    assert e_tot[0] <= mf.e_tot + 1e-10                      # the RHF determinant lies in the space
    if caslst:
        picked = np.abs(np.asarray(mo).T @ mf.get_ovlp() @ np.asarray(mf.mo_coeff)).argmax(axis=1)[mc.ncore:mc.ncore + ncas] + 1
        assert tuple(picked) == tuple(caslst)
    # natural orbitals
    mn = mcscf.CASCI(mf, ncas, nelecas)
    mn.fcisolver.nroots = nroots
    mn.natorb = True
    en = mn.kernel(mo0)[0]
    occ = mn.mo_occ[mn.ncore:mn.ncore + ncas]
    dm = mn.make_rdm1()
    ntr = np.sum(dm * mf.get_ovlp())
    again = mcscf.CASCI(mf, ncas, nelecas)
    again.fcisolver.nroots = nroots
    e2 = again.kernel(mn.mo_coeff)[0]
    print(f"natural occupations {np.round(occ, 6)}, Tr[D S] = {ntr:.10f}, natorb vs canonical {np.abs(en - np.asarray(e_tot)).max():.2e}, "
          f"recomputed from the rotated orbitals {np.abs(np.asarray(e2) - en).max():.2e}")
    assert abs(occ.sum() - nelecas) <= 1e-9 and occ.min() >= -1e-12 and occ.max() <= 2 + 1e-12 and np.all(np.diff(occ) <= 1e-12)
    assert np.all(mn.mo_occ[:mn.ncore] == 2) and np.all(mn.mo_occ[mn.ncore + ncas:] == 0)
    assert abs(ntr - mol.nelectron) <= 1e-9
    assert np.abs(en - np.asarray(e_tot)).max() <= 1e-9 and np.abs(np.asarray(e2) - en).max() <= 1e-9


def test_facades_and_solver_settings():
    import gpu4pyscf.mcscf
    from pyscf import mcscf, fci
    from mi355scf import casci, fci as native
    assert gpu4pyscf.mcscf.CASCI is mcscf.CASCI is casci.CASCI
    assert fci.FCISolver is native.FCISolver is fci.direct_spin1.FCISolver and isinstance(fci.direct_spin1.FCI(), native.FCISolver)
    mol, mf = _rhf("h2o", "6-31g(d)")
    assert isinstance(fci.FCI(mol), native.FCISolver) and isinstance(fci.FCI(mf), native.FCISolver)
    mc = mcscf.CASCI(mf, 4, 4)
    mc.fcisolver.nroots = 5                     # the reference script's perform_casci
    out = mc.kernel()
    assert len(out) == 5
    e_casci, e_cas, civec, mo, mo_e = out
    assert isinstance(e_casci, np.ndarray) and e_casci.shape == (5,) and len(civec) == 5 and np.all(np.diff(e_casci) >= -1e-12)
    assert civec[0].shape == (6, 6) and mo.shape == np.asarray(mf.mo_coeff).shape and mo_e.shape == np.asarray(mf.mo_energy).shape
    ss0 = mc.fcisolver.spin_square(civec[0], mc.ncas, mc.nelecas)[0]
    assert abs(ss0) < 1e-7 and mc.e_tot is e_casci and mc.ncas == 4 and mc.nelecas == (2, 2) and mc.ncore == 3


def test_unsupported_references_are_refused():
    from pyscf import gto, scf, dft, mcscf, solvent
    mol = gto.M(atom=MOLECULES["h2o"], basis="6-31g(d)", verbose=0)

    def rks(xc):
        mf = dft.RKS(mol)
        mf.xc = xc
        return mf

    two_ranks = scf.RHF(mol)
    two_ranks._rank, two_ranks._nranks = 0, 2
    cases = {"RKS": rks("b3lyp"), "CAM-B3LYP": rks("camb3lyp"), "UHF": scf.UHF(mol), "density_fit": scf.RHF(mol).density_fit(),
             "PCM": solvent.PCM(scf.RHF(mol)), "two ranks": two_ranks}
    for what, mf in cases.items():
        with pytest.raises(NotImplementedError):
            mcscf.CASCI(mf, 4, 4)
        print(f"{what}: refused")
    with pytest.raises(NotImplementedError):
        mcscf.CASSCF(scf.RHF(mol), 4, 4)
    for ncas, nelecas in ((4, 5), (2, 6), (4, 12), (17, 4)):      # odd core, too many active electrons, more than the molecule has, too large
        with pytest.raises(NotImplementedError):
            mcscf.CASCI(scf.RHF(mol), ncas, nelecas)
    with pytest.raises(NotImplementedError):
        mcscf.CASCI(scf.RHF(mol), 4, 4, ncore=2)
