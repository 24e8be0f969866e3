"""ROHF / ROKS without a GPU: facade identities, object construction, the `nelecas` unpacking of `mcscf.CASCI` on an open-shell
molecule and the refusals.  Also holds the plain numpy Roothaan ROHF that `test_gpu_rohf.py` uses as the independent solution; it
is checked here against the CPU oracle's RHF in the closed-shell limit and for stationarity on a radical."""
import numpy as np
import pytest

OH = "O 0 0 0; H 0 0 0.97"
CH2 = "C 0 0 0; H 0 0.99 0.43; H 0 -0.99 0.43"
O2 = "O 0 0 0; O 0 0 1.21"
H2O = "O 0 0 0; H 0 -0.757 0.587; H 0 0.757 0.587"


def mol_of(atom, basis, spin):
    from pyscf import gto
    m = gto.Mole()
    m.atom, m.basis, m.spin, m.verbose = atom, basis, spin, 0
    m.build()
    return m


# ---- numpy reference (oracle integrals, dense einsum J/K) --------------------------------------------------------------------
def ref_fock_pair(h, eri, Da, Db):
    """(Fa, Fb, E_elec) of the UHF energy functional at (Da, Db)."""
    D = Da + Db
    J = np.einsum("ijkl,kl->ij", eri, D)
    Fa = h + J - np.einsum("ikjl,kl->ij", eri, Da)
    Fb = h + J - np.einsum("ikjl,kl->ij", eri, Db)
    return Fa, Fb, 0.5 * (np.sum(Da * (h + Fa)) + np.sum(Db * (h + Fb)))


def ref_blocks(Fa, Fb, C, ncore, nopen):
    """The three inter-class blocks of the ROHF orbital gradient in the orbitals C: (Fb closed-open, Fa open-virtual, Fc closed-virtual)."""
    fa, fb = C.T @ Fa @ C, C.T @ Fb @ C
    c, o, v = slice(0, ncore), slice(ncore, ncore + nopen), slice(ncore + nopen, None)
    return fb[c, o], fa[o, v], 0.5 * (fa + fb)[c, v]


def ref_roothaan(Fa, Fb, C, ncore, nopen):
    fa, fb = C.T @ Fa @ C, C.T @ Fb @ C
    cls = np.repeat([0, 1, 2], [ncore, nopen, C.shape[1] - ncore - nopen])
    lo, hi = np.minimum.outer(cls, cls), np.maximum.outer(cls, cls)
    return np.where((lo == 0) & (hi == 1), fb, np.where((lo == 1) & (hi == 2), fa, 0.5 * (fa + fb)))


def numpy_rohf(mol, S, h, eri, damp=0.5, tol=1e-12, gtol=1e-8, max_cycle=3000, C0=None):
    """Roothaan ROHF by repeated `eigh` of the effective Fock operator with the Fock pair damped, from the core Hamiltonian's
    orbitals (or C0).  Returns (E_tot, C, cycles, largest orbital-gradient element)."""
    na, nb = mol.nelec
    Li = np.linalg.inv(np.linalg.cholesky(S))

    def orbitals(F):
        return Li.T @ np.linalg.eigh(Li @ F @ Li.T)[1]

    C = orbitals(h) if C0 is None else C0
    e_old, old = 0.0, None
    for it in range(max_cycle):
        Fa, Fb, e = ref_fock_pair(h, eri, C[:, :na] @ C[:, :na].T, C[:, :nb] @ C[:, :nb].T)
        gmax = max([np.abs(b).max() for b in ref_blocks(Fa, Fb, C, nb, na - nb) if b.size] or [0.0])
        if abs(e - e_old) < tol and gmax < gtol:
            break
        e_old = e
        if old is not None:
            Fa, Fb = (1 - damp) * Fa + damp * old[0], (1 - damp) * Fb + damp * old[1]
        old = (Fa, Fb)
        SC = S @ C
        C = orbitals(SC @ ref_roothaan(Fa, Fb, C, nb, na - nb) @ SC.T)
    return e + mol.energy_nuc(), C, it, gmax


def oracle_integrals(mol):
    from oracle import oracle as orc
    o = orc.Oracle(mol)
    S, T, V, _ = o.int1e()
    return S, T + V, o.eri_full()


def test_numpy_rohf_reference_is_sound():
    from oracle import oracle as orc
    h2o = mol_of(H2O, "sto-3g", 0)
    e, _, _, g = numpy_rohf(h2o, *oracle_integrals(h2o))
    assert abs(e - orc.rhf(h2o, conv_tol=1e-11)["e_tot"]) < 1e-9 and g < 1e-8
    oh = mol_of(OH, "sto-3g", 1)
    S, h, eri = oracle_integrals(oh)
    e, C, _, g = numpy_rohf(oh, S, h, eri)
    assert g < 1e-8 and np.abs(C.T @ S @ C - np.eye(C.shape[1])).max() < 1e-10
    Fa, Fb, e_el = ref_fock_pair(h, eri, C[:, :5] @ C[:, :5].T, C[:, :4] @ C[:, :4].T)
    assert abs(e_el + oh.energy_nuc() - e) < 1e-10 and -74.40 < e < -74.33        # OH/STO-3G ROHF lies near -74.36 Ha


# ---- surface -----------------------------------------------------------------------------------------------------------------
def test_facades_are_the_engine_classes():
    import gpu4pyscf
    import gpu4pyscf.hessian
    import pyscf
    from pyscf import dft, hessian, scf
    from mi355scf import rohf, uhf, uks
    assert pyscf.scf.ROHF is gpu4pyscf.scf.ROHF is rohf.ROHF is scf.rohf.ROHF is gpu4pyscf.scf.rohf.ROHF
    assert pyscf.dft.ROKS is gpu4pyscf.dft.ROKS is rohf.ROKS is dft.roks.ROKS is gpu4pyscf.dft.roks.ROKS
    assert isinstance(scf.rohf.ROHF, type) and issubclass(rohf.ROHF, uhf.UHF) and issubclass(rohf.ROKS, (rohf.ROHF, uks.UKS))
    assert hessian.rohf.Hessian is hessian.uhf.Hessian is gpu4pyscf.hessian.rohf.Hessian and hessian.ROKS is hessian.UKS


def test_construction_touches_no_gpu():
    from pyscf import dft, scf
    oh = mol_of(OH, "6-31g(d)", 1)
    mf = scf.ROHF(oh)
    assert mf._eng is None and mf.to_gpu() is mf and mf.to_cpu() is mf and mf.mo_coeff is None and not mf.converged
    assert mf._classes() == (4, 1) and mf.nelec == (5, 4)
    ss, mult = mf.spin_square()
    assert ss == 0.75 and mult == 2.0
    ks = dft.ROKS(oh)
    ks.xc = "b3lyp"
    assert ks._eng is None and ks.grids is not None and isinstance(ks, scf.ROHF)
    assert scf.ROHF(mol_of(O2, "sto-3g", 2)).spin_square() == (2.0, 3.0)
    closed = scf.ROHF(mol_of(H2O, "sto-3g", 0))
    assert closed._classes() == (5, 0) and closed.spin_square() == (0.0, 1.0)
    # the per-spin diagonals ride on mo_energy through views and copies of the whole vector, not onto slices
    from mi355scf.rohf import _MOEnergy
    e = np.arange(6.0).view(_MOEnergy)
    e.mo_ea, e.mo_eb = np.ones(6), np.zeros(6)
    assert e.copy().mo_ea is e.mo_ea and (e + 1.0).mo_eb is e.mo_eb and e[:3].mo_ea is None and np.asarray(e).sum() == 15.0
    # a density from orbitals and occupations 2 / 1 / 0 is the (Da, Db) stack
    C = np.linalg.qr(np.random.default_rng(3).normal(size=(6, 6)))[0]
    dm = mf.make_rdm1(C, np.array([2.0, 2, 1, 1, 0, 0]))
    assert dm.shape == (2, 6, 6) and np.allclose(dm[0], C[:, :4] @ C[:, :4].T) and np.allclose(dm[1], C[:, :2] @ C[:, :2].T)
    # RHF / RKS keep refusing open shells
    with pytest.raises(NotImplementedError):
        scf.RHF(oh)
    with pytest.raises(NotImplementedError):
        dft.RKS(oh)


def test_casci_unpacks_nelecas_with_the_molecules_spin():
    from pyscf import mcscf, scf
    o2 = scf.ROHF(mol_of(O2, "sto-3g", 2))
    mc = mcscf.CASCI(o2, 2, 2)
    assert mc.nelecas == (2, 0) and mc.ncore == 7 and mc._scf is o2
    assert mcscf.CASCI(o2, 4, 6).nelecas == (4, 2) and mcscf.CASCI(o2, 4, (3, 3)).nelecas == (3, 3)
    oh = scf.ROHF(mol_of(OH, "sto-3g", 1))
    mc = mcscf.CASCI(oh, 4, 3)
    assert mc.nelecas == (2, 1) and mc.ncore == 3
    for bad in (4, 0):                             # an even count cannot carry spin 1; fewer electrons than the spin neither
        with pytest.raises(ValueError):
            mcscf.CASCI(oh, 4, bad)
    # closed-shell references unpack as before
    assert mcscf.CASCI(scf.RHF(mol_of(H2O, "sto-3g", 0)), 4, 4).nelecas == (2, 2)


def test_casci_refuses_an_open_shell_core_and_roks():
    from pyscf import dft, mcscf, scf
    o2 = scf.ROHF(mol_of(O2, "sto-3g", 2))
    assert mcscf.CASCI(o2, 2, (1, 1)).ncore == 7  # active block [7, 9) holds both singly occupied orbitals: accepted
    with pytest.raises(NotImplementedError, match="singly occupied orbital 8"):
        mcscf.CASCI(o2, 1, (1, 1))                # ncore = 7, active block [7, 8): orbital 8 is left out
    with pytest.raises(NotImplementedError, match="singly occupied orbital 7"):
        mcscf.CASCI(o2, 1, (0, 0), ncore=8)       # the whole open shell in the core
    ks = dft.ROKS(mol_of(O2, "sto-3g", 2))
    ks.xc = "b3lyp"
    with pytest.raises(NotImplementedError, match="Kohn-Sham"):
        mcscf.CASCI(ks, 2, 2)


def test_methods_without_an_open_shell_form_refuse_rohf():
    from pyscf import cc, dft, mp, scf, solvent, tdscf
    oh = mol_of(OH, "sto-3g", 1)
    mf = scf.ROHF(oh)
    ks = dft.ROKS(oh)
    ks.xc = "camb3lyp"
    with pytest.raises(NotImplementedError, match="range-separated"):
        ks.kernel()
    for what, make in (("PCM", lambda: solvent.PCM(mf)), ("mf.PCM", mf.PCM), ("TDA", lambda: tdscf.TDA(mf)), ("TDDFT", lambda: tdscf.TDDFT(mf)),
                       ("mf.TDA", mf.TDA), ("MP2", lambda: mp.MP2(mf)), ("CCSD", lambda: cc.CCSD(mf)), ("density_fit", mf.density_fit),
                       ("shard", lambda: mf.shard(0, 2))):
        with pytest.raises(NotImplementedError):
            make()
        print(f"{what}: refused")
