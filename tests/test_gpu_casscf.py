"""CASSCF (`pyscf.mcscf.CASSCF` -> `mi355scf.casscf`) against references built in this file from the CPU oracle's dense integrals
and the dense determinant Hamiltonian of test_fci_host.py (`ref_hamiltonian`, `ref_rdm12`): the returned orbitals are checked to
be a stationary point of the oracle-side energy (generalised-Fock gradient from full-MO 1- and 2-RDMs by einsum), a minimum
(finite-difference Hessian), and the energy to equal the dense-FCI energy in those orbitals.  CASSCF objects run with
conv_tol = 1e-10, conv_tol_grad = 1e-5, the RHF with conv_tol = 1e-11.  Molecules come from `conftest.MOLECULES`; H2 is 0.74 A."""
import functools

import numpy as np
import pytest

from conftest import MOLECULES
from test_fci_host import ref_hamiltonian, ref_rdm12

pytestmark = pytest.mark.gpu

H2 = "H 0 0 0; H 0 0 0.74"
TOL_G = 1e-5
G_BOUND = 1.1 * TOL_G + 1e-7      # 1e-7: the 1e-8 engine-oracle integral margin carried through F


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
def _ints(name, basis):
    from oracle import oracle as orc
    o = orc.Oracle(_rhf(name, basis)[0])
    S, T, V, _ = o.int1e()
    return S, T + V, o.eri_full()


def _casscf(mf, ncas, nelecas, **kw):
    from pyscf import mcscf
    mc = mcscf.CASSCF(mf, ncas, nelecas)
    mc.conv_tol, mc.conv_tol_grad = 1e-10, TOL_G
    for k, v in kw.items():
        setattr(mc, k, v)
    return mc


def _mo_integrals(name, basis, mo):
    S, h, eri = _ints(name, basis)
    return mo.T @ h @ mo, np.einsum("pqrs,pi,qj,rk,sl->ijkl", eri, mo, mo, mo, mo, optimize=True)


def _active_problem(hm, em, ncore, ncas):
    c, a = slice(0, ncore), slice(ncore, ncore + ncas)
    e_core = 2.0 * np.trace(hm[c, c]) + 2.0 * np.einsum("iijj->", em[c, c, c, c]) - np.einsum("ijij->", em[c, c, c, c])
    hc = hm[a, a] + 2.0 * np.einsum("tuii->tu", em[a, a, c, c]) - np.einsum("tiui->tu", em[a, c, a, c])
    return e_core, hc, em[a, a, a, a]


def _oracle_side(name, basis, mo, ncore, ncas, nelecas, weights=(1.0,)):
    """(state energies, max |g|) in the orbitals `mo`: dense FCI, then the generalised Fock matrix F_pq = sum_r D_pr h_rq +
    sum_rst G_prst (qr|st) from the full-MO RDMs (core 2 / active gamma; G assembled from its core-core, core-active and
    active-active parts), g = 2 (F - F^T) on the non-redundant blocks."""
    mol = _rhf(name, basis)[0]
    hm, em = _mo_integrals(name, basis, mo)
    nmo = hm.shape[0]
    nocc = ncore + ncas
    e_core, hc, ea = _active_problem(hm, em, ncore, ncas)
    w, V = np.linalg.eigh(ref_hamiltonian(hc, ea, ncas, nelecas))
    gamma = np.zeros((ncas, ncas))
    Gamma = np.zeros((ncas,) * 4)
    for i, wt in enumerate(weights):
        d1, d2 = ref_rdm12(V[:, i], V[:, i], ncas, nelecas)
        gamma += wt * d1
        Gamma += wt * d2
    D = np.zeros((nocc, nocc))
    D[:ncore, :ncore] = 2.0 * np.eye(ncore)
    D[ncore:, ncore:] = gamma
    G = np.zeros((nocc,) * 4)
    G[ncore:, ncore:, ncore:, ncore:] = Gamma
    for i in range(ncore):
        for j in range(ncore):
            G[i, i, j, j] += 4.0
            G[i, j, j, i] -= 2.0
        G[i, i, ncore:, ncore:] += 2.0 * gamma
        G[ncore:, ncore:, i, i] += 2.0 * gamma
        G[i, ncore:, ncore:, i] -= gamma
        G[ncore:, i, i, ncore:] -= gamma
    o = slice(0, nocc)
    F = np.zeros((nmo, nmo))
    F[o] = D @ hm[o] + np.einsum("prst,qrst->pq", G, em[:, o, o, o], optimize=True)
    g = 2.0 * (F - F.T)
    kind = np.zeros(nmo, dtype=int)
    kind[ncore:nocc] = 1
    kind[nocc:] = 2
    g[kind[:, None] == kind[None, :]] = 0.0
    # the assembled RDMs reproduce the energy: guards the G bookkeeping above
    e_chk = np.sum(D * hm[o, o]) + 0.5 * np.sum(G * em[o, o, o, o]) + mol.energy_nuc()
    e_states = w[:len(weights)] + e_core + mol.energy_nuc()
    assert abs(e_chk - float(np.dot(weights, e_states))) < 1e-9
    return e_states, float(np.abs(g).max())


# ---- closed limits ----------------------------------------------------------------------------------------------------------------
def test_fully_occupied_active_space_is_the_rhf_determinant():
    mol, mf = _rhf("h2o", "6-31g(d)")
    mc = _casscf(mf, 2, 4)
    e_tot = mc.kernel()[0]
    print(f"CASSCF(2,4) - RHF = {e_tot - mf.e_tot:.2e}, macro iterations {mc.macro_iterations}")
    assert abs(e_tot - mf.e_tot) <= 1e-9 and mc.converged and mc.macro_iterations == 1


def test_all_orbitals_active_is_full_ci_of_h2():
    from pyscf import fci
    mol, mf = _rhf("h2", "6-31g(d,p)")
    nmo = mf.mo_coeff.shape[1]
    mc = _casscf(mf, nmo, 2)
    e_tot = mc.kernel()[0]
    e_fci = fci.FCI(mf).kernel()[0]
    print(f"H2 CASSCF({nmo},2) - FCI = {e_tot - e_fci:.2e}")
    assert abs(e_tot - e_fci) <= 1e-8 and mc.converged


# ---- stationary point -------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _converged(case):
    from pyscf import mcscf
    name, basis, ncas, nelecas, caslst = case
    mol, mf = _rhf(name, basis)
    mc = _casscf(mf, ncas, nelecas)
    ci = mcscf.CASCI(mf, ncas, nelecas)
    mo0 = np.asarray(mf.mo_coeff)
    if caslst:
        mo0 = mc.sort_mo(list(caslst))
    e_casci = ci.kernel(mo0)[0]
    mc.kernel(mo0)
    return mc, float(e_casci)


CASES = [("h2o", "6-31g(d)", 4, 4, None), ("h2co", "6-31g(d)", 2, 2, (7, 9))]


@pytest.mark.parametrize("case", CASES, ids=["h2o-cas44", "h2co-cas22"])
def test_stationary_point_against_the_oracle(case):
    name, basis, ncas, nelecas, _ = case
    mc, e_casci = _converged(case)
    S = _ints(name, basis)[0]
    e_ref, gmax = _oracle_side(name, basis, mc.mo_coeff, mc.ncore, ncas, (nelecas // 2, nelecas // 2))
    print(f"{name} CAS({nelecas},{ncas}): {mc.macro_iterations} macro iterations, E = {mc.e_tot:.10f}, E - dense FCI = "
          f"{mc.e_tot - e_ref[0]:.2e}, oracle max|g| = {gmax:.2e}, E - E(CASCI/RHF) = {mc.e_tot - e_casci:.3e}")
    assert mc.converged
    assert abs(mc.e_tot - e_ref[0]) <= 1e-8
    assert gmax <= G_BOUND
    assert mc.e_tot <= e_casci + 1e-10
    if ncas == 4:
        assert mc.e_tot < e_casci - 1e-5
    assert abs(mc.e_cas + mc.e_core - mc.e_tot) < 1e-12
    assert np.abs(mc.mo_coeff.T @ S @ mc.mo_coeff - np.eye(mc.mo_coeff.shape[1])).max() < 1e-10
    act = slice(mc.ncore, mc.ncore + ncas)
    assert np.array_equal(mc.mo_occ[act], np.diag(mc.fcisolver.make_rdm1(mc.ci, ncas, mc.nelecas)))
    assert np.all(mc.mo_occ[:mc.ncore] == 2) and np.all(mc.mo_occ[mc.ncore + ncas:] == 0)


def test_restart_converges_at_once():
    mc, _ = _converged(CASES[0])
    e0 = mc.e_tot
    mc2 = _casscf(mc._scf, 4, 4)
    e1 = mc2.kernel(mc.mo_coeff, mc.ci)[0]
    print(f"restart: {mc2.macro_iterations} macro iterations, dE = {e1 - e0:.2e}")
    assert mc2.converged and mc2.macro_iterations <= 2 and abs(e1 - e0) <= 1e-9


def test_minimum_not_saddle():
    """h2o/sto-3g CAS(4,4): 12 rotations.  Finite-difference Hessian (step 1e-3) of the oracle-side E(kappa) = lowest dense-FCI
    eigenvalue in the rotated orbitals, at the engine's converged orbitals.

    From the RHF orbitals the active space is {3a1, 1b1, 4a1, 2b2}; the minimal basis has a single b1 function, so 1b1 has no
    correlating partner, while the core orbital 1b2 would correlate with 2b2.  The 1b2 <-> 1b1 rotation mixes two symmetries, so
    its gradient is zero at every symmetric point: a gradient-only optimiser stops at a saddle (eigenvalue -6.0e-2) and only the
    driver's Hessian-eigenvalue check leaves it."""
    from mi355scf import casscf
    name, basis = "h2o", "sto-3g"
    mol, mf = _rhf(name, basis)
    mc = _casscf(mf, 4, 4)
    mc.kernel()
    assert mc.converged and mc.stable
    nmo, ncore = mc.mo_coeff.shape[1], mc.ncore
    npar = len(casscf.rotation_pairs(nmo, ncore, 4)[0])
    assert npar == 12
    S, h, eri = _ints(name, basis)

    def energy(x):
        mo = casscf.rotate(mc.mo_coeff, x, ncore, 4)
        hm = mo.T @ h @ mo
        em = np.einsum("pqrs,pi,qj,rk,sl->ijkl", eri, mo, mo, mo, mo, optimize=True)
        e_core, hc, ea = _active_problem(hm, em, ncore, 4)
        return np.linalg.eigvalsh(ref_hamiltonian(hc, ea, 4, (2, 2)))[0] + e_core

    d = 1e-3
    e0 = energy(np.zeros(npar))
    ep = np.array([energy(d * np.eye(npar)[k]) for k in range(npar)])
    em_ = np.array([energy(-d * np.eye(npar)[k]) for k in range(npar)])
    H = np.zeros((npar, npar))
    I = np.eye(npar)
    for k in range(npar):
        H[k, k] = (ep[k] - 2 * e0 + em_[k]) / d ** 2
        for l in range(k):                     # symmetric second difference, O(d^2) error
            H[k, l] = H[l, k] = (energy(d * (I[k] + I[l])) + energy(-d * (I[k] + I[l])) - ep[k] - em_[k] - ep[l] - em_[l] + 2 * e0) / (2 * d ** 2)
    wmin = np.linalg.eigvalsh(H)[0]
    print(f"h2o/sto-3g CAS(4,4): {mc.macro_iterations} macro iterations, smallest Hessian eigenvalue {wmin:.4e}")
    assert wmin >= -1e-5


# ---- natural orbitals -------------------------------------------------------------------------------------------------------------
def test_natural_orbitals_and_bookkeeping():
    mc0, _ = _converged(CASES[0])
    mol, mf = _rhf("h2o", "6-31g(d)")
    S = _ints("h2o", "6-31g(d)")[0]
    mc = _casscf(mf, 4, 4, natorb=True)
    mc.kernel()
    occ = mc.mo_occ[mc.ncore:mc.ncore + 4]
    print(f"natural occupations {occ}, E - E(natorb=False) = {mc.e_tot - mc0.e_tot:.2e}")
    assert mc.converged
    assert np.all(np.diff(occ) <= 0) and np.all(occ >= 0) and np.all(occ <= 2) and abs(occ.sum() - 4) <= 1e-9
    assert abs(mc.e_tot - mc0.e_tot) <= 1e-9
    assert abs(np.trace(mc.make_rdm1() @ S) - mol.nelectron) <= 1e-9
    assert np.abs(mc.mo_coeff.T @ S @ mc.mo_coeff - np.eye(mc.mo_coeff.shape[1])).max() < 1e-10
    dm = mc.fcisolver.make_rdm1(mc.ci, 4, mc.nelecas)
    assert np.abs(dm - np.diag(occ)).max() < 1e-6            # the CI belongs to the returned orbitals


# ---- state average ----------------------------------------------------------------------------------------------------------------
def test_state_average():
    from pyscf import mcscf
    mol, mf = _rhf("h2o", "6-31g(d)")
    base = _casscf(mf, 4, 4)
    mc = base.state_average([0.5, 0.5])
    assert mc is not base and base.weights is None and base.fcisolver.nroots == 1 and mc.fcisolver.nroots == 2
    assert base.state_average_([0.5, 0.5]) is base
    mc.kernel()
    ci = mcscf.CASCI(mf, 4, 4)
    ci.fcisolver.nroots = 2
    e_casci = np.asarray(ci.kernel()[0])
    e_ref, gmax = _oracle_side("h2o", "6-31g(d)", mc.mo_coeff, mc.ncore, 4, (2, 2), weights=(0.5, 0.5))
    print(f"SA-CASSCF: {mc.macro_iterations} macro iterations, e_states = {mc.e_states}, oracle max|g| = {gmax:.2e}, "
          f"E - dense = {mc.e_tot - 0.5 * e_ref.sum():.2e}, E - SA-CASCI/RHF = {mc.e_tot - 0.5 * e_casci.sum():.3e}")
    assert mc.converged and len(mc.ci) == 2 and len(mc.e_states) == 2
    assert abs(mc.e_tot - float(np.dot([0.5, 0.5], mc.e_states))) <= 1e-12
    assert np.abs(mc.e_states - e_ref).max() <= 1e-8
    assert gmax <= G_BOUND
    assert mc.e_tot <= 0.5 * e_casci.sum() + 1e-10


# ---- the template's flow ----------------------------------------------------------------------------------------------------------
def test_benzene_template_flow():
    """calculate_casscf.py's default path: RHF -> avas -> CASSCF(6,6) -> analyze_casscf_results' arithmetic.  The fixture's ring
    lies in the xy plane, so the pi system is selected with 'C 2pz'."""
    from pyscf import gto, scf, mcscf
    from pyscf.mcscf import avas
    from mi355scf import smiles_fixtures
    sym, xyz = smiles_fixtures.lookup("c1ccccc1")
    mol = gto.Mole()
    mol.atom = [(s, tuple(x)) for s, x in zip(sym, xyz)]
    mol.basis, mol.unit, mol.verbose = "6-31G*", "Angstrom", 0
    mol.build()
    mf = scf.RHF(mol)
    mf.kernel()
    assert mf.converged
    e_hf = mf.e_tot
    ncas, nelecas, mo = avas.avas(mf, ["C 2pz"])
    assert (ncas, nelecas) == (6, 6) and mo.shape == mf.mo_coeff.shape
    mf.mo_coeff = mo
    mc = mcscf.CASSCF(mf, ncas, nelecas)
    mc.conv_tol = 1e-7
    mc.max_cycle_macro = 100
    mc.kernel()
    cas_occ = mc.mo_occ[mc.ncore:mc.ncore + mc.ncas]
    entropy = -np.sum(cas_occ * np.log(cas_occ + 1e-14) + (2 - cas_occ) * np.log(2 - cas_occ + 1e-14))
    ci_vec = mc.ci.flatten()
    k = np.argmax(np.abs(ci_vec))
    print(f"benzene CAS(6,6): {mc.macro_iterations} macro iterations, E - E(HF) = {mc.e_tot - e_hf:.6f}, occupations {cas_occ}, "
          f"entropy {entropy:.4f}, leading CI weight {ci_vec[k] ** 2:.4f}, {np.sum(np.abs(ci_vec) > 0.1)} significant")
    assert mc.converged and mc.e_tot < e_hf and np.isfinite(entropy) and np.isfinite(mc.e_cas)
    assert abs(cas_occ.sum() - 6) <= 1e-8


# ---- refusals ---------------------------------------------------------------------------------------------------------------------
def test_refusals():
    from pyscf import dft, gto, mcscf, scf, solvent
    mol, mf = _rhf("h2o", "6-31g(d)")
    rohf = scf.ROHF(gto.M(atom=MOLECULES["h2o"], basis="6-31g(d)", charge=1, spin=1, verbose=0))
    ks = dft.RKS(mol)
    ks.xc = "pbe"
    dfm = scf.RHF(mol).density_fit()
    pcm = solvent.PCM(scf.RHF(mol))
    two = scf.RHF(mol)
    two._nranks = 2
    for what, ref in (("ROHF", rohf), ("RKS", ks), ("UHF", scf.UHF(mol)), ("density-fitted", dfm), ("PCM", pcm), ("two-rank", two),
                      ("unrun", scf.RHF(mol))):
        with pytest.raises(NotImplementedError):
            mcscf.CASSCF(ref, 4, 4 if what != "ROHF" else 3)
        print(f"{what}: refused")
    with pytest.raises(ValueError):
        mcscf.CASSCF(mf, 4, 4).state_average([0.7, 0.7])
    plain = mcscf.CASSCF(mf, 4, 4)
    plain.fcisolver.nroots = 2
    with pytest.raises(NotImplementedError):
        plain.kernel()
