"""ROHF / ROKS on the engine (`scf.ROHF`, `dft.ROKS`) against the CPU oracle's integrals, a plain numpy Roothaan ROHF, the
engine's own UHF / RHF / RKS and central differences of its own energies.  OH (spin 1), CH2 (spin 2) and O2 (1.21 Angstrom,
spin 2) in 6-31G(d) unless a test says otherwise; every SCF of a molecule is solved once and shared."""
import functools

import numpy as np
import pytest

from test_rohf_host import CH2, H2O, O2, OH, mol_of, numpy_rohf, oracle_integrals, ref_blocks, ref_fock_pair

pytestmark = pytest.mark.gpu

MOLS = {"oh": (OH, 1), "ch2": (CH2, 2), "o2": (O2, 2)}


@functools.lru_cache(maxsize=None)
def _rohf(name, basis="6-31g(d)"):
    from pyscf import scf
    mol = mol_of(*MOLS[name][:1], basis, MOLS[name][1])
    mf = scf.ROHF(mol).to_gpu()
    mf.conv_tol = 1e-11
    mf.kernel()
    assert mf.converged
    return mol, mf


@functools.lru_cache(maxsize=None)
def _ints(name, basis="6-31g(d)"):
    return oracle_integrals(_rohf(name, basis)[0])


@pytest.mark.parametrize("name", ["oh", "ch2", "o2"])
def test_energy_and_stationarity_on_oracle_integrals(name):
    """The ROHF energy functional at the engine's (Da, Db) with the oracle's integrals (einsum J/K) within 1e-8 of the engine's
    energy, and the oracle's Fock pair in the engine's orbitals stationary: the three orbital-gradient blocks below 1e-5, the
    square root of conv_tol = 1e-11 with room for the gradient test conv_tol_grad = sqrt(conv_tol) applies to a norm."""
    mol, mf = _rohf(name)
    S, h, eri = _ints(name)
    dm = mf.make_rdm1()
    Fa, Fb, e_el = ref_fock_pair(h, eri, dm[0], dm[1])
    e_ref = e_el + mol.energy_nuc()
    na, nb = mol.nelec
    blocks = [np.abs(b).max() if b.size else 0.0 for b in ref_blocks(Fa, Fb, np.asarray(mf.mo_coeff), nb, na - nb)]
    print(f"{name}: E(ROHF) = {mf.e_tot:.10f}, engine - oracle functional = {mf.e_tot - e_ref:.2e}, {mf.cycles} cycles; "
          f"max |Fb_co| {blocks[0]:.2e}, |Fa_ov| {blocks[1]:.2e}, |Fc_cv| {blocks[2]:.2e}")
    assert abs(mf.e_tot - e_ref) <= 1e-8
    assert max(blocks) < 1e-5


@pytest.mark.parametrize("name", ["oh", "o2"])
def test_plain_numpy_roothaan_rohf_reaches_the_same_energy(name):
    """An independent solution: `numpy_rohf` (eigh + damping on the oracle's integrals, from the core Hamiltonian's orbitals) in
    STO-3G must land within 1e-7 of the engine's energy."""
    mol, mf = _rohf(name, "sto-3g")
    e_np, C, cycles, g = numpy_rohf(mol, *_ints(name, "sto-3g"))
    print(f"{name}/STO-3G: engine {mf.e_tot:.10f} ({mf.cycles} cycles), numpy {e_np:.10f} ({cycles} cycles, gradient {g:.1e}), "
          f"difference {mf.e_tot - e_np:.2e}")
    assert g < 1e-8 and abs(mf.e_tot - e_np) <= 1e-7


@pytest.mark.parametrize("name", ["oh", "ch2", "o2"])
def test_invariants(name):
    """<S^2> = S(S+1); the beta space lies in the alpha space (Db S Da = Db); Tr[(Da - Db) S] = n_open; occupations 2 / 1 / 0;
    E(ROHF) >= E(UHF), the UHF started from the ROHF densities so that it relaxes the same state."""
    from pyscf import scf
    mol, mf = _rohf(name)
    na, nb = mol.nelec
    s = 0.5 * (na - nb)
    S = mf.get_ovlp()
    dm = mf.make_rdm1()
    C, occ = np.asarray(mf.mo_coeff), np.asarray(mf.mo_occ)
    nest = np.abs(dm[1] @ S @ dm[0] - dm[1]).max()
    nopen = np.trace((dm[0] - dm[1]) @ S)
    uhf = scf.UHF(mol).to_gpu()
    uhf.conv_tol = 1e-11
    e_uhf = uhf.kernel(dm0=dm)
    print(f"{name}: <S^2> = {mf.spin_square()[0]}, |Db S Da - Db| = {nest:.1e}, Tr[(Da - Db) S] = {nopen:.12f}, "
          f"E(ROHF) - E(UHF) = {mf.e_tot - e_uhf:.3e}, UHF <S^2> = {uhf.spin_square()[0]:.6f}")
    assert abs(mf.spin_square()[0] - s * (s + 1)) <= 1e-10 and abs(mf.spin_square()[1] - (2 * s + 1)) <= 1e-10
    assert nest <= 1e-10 and abs(nopen - (na - nb)) <= 1e-10
    assert C.shape == (mol.nao, mol.nao) and occ.shape == (mol.nao,) and dm.shape == (2, mol.nao, mol.nao)
    assert np.all(occ[:nb] == 2) and np.all(occ[nb:na] == 1) and np.all(occ[na:] == 0)
    assert np.abs(C.T @ S @ C - np.eye(mol.nao)).max() < 1e-10
    assert np.abs(mf.make_rdm1(C, occ) - dm).max() < 1e-10
    e = mf.mo_energy
    assert e.shape == (mol.nao,) and np.all(np.diff(e) >= -1e-12) and e.mo_ea.shape == e.mo_eb.shape == (mol.nao,)
    assert uhf.converged and mf.e_tot >= e_uhf - 1e-9
    from oracle import oracle as orc
    dip = orc.Oracle(mol).int1e()[3]
    mu_ref = -np.einsum("xij,ij->x", dip, dm[0] + dm[1]) + mol.atom_charges() @ mol.atom_coords()
    assert np.abs(mf.dip_moment(unit="au") - mu_ref).max() < 1e-8


def test_closed_shell_limit():
    """Water, spin 0: ROHF == RHF to 1e-9 and ROKS/B3LYP == RKS/B3LYP to 1e-8 (RKS without its density-based grid pruning, which
    the spin-polarised quadrature does not have: the setting `test_gpu_uks.py` uses for UKS == RKS)."""
    from pyscf import dft, scf
    h2o = mol_of(H2O, "6-31g(d)", 0)
    ro, r = scf.ROHF(h2o), scf.RHF(h2o)
    ro.conv_tol = r.conv_tol = 1e-11
    e_ro, e_r = ro.kernel(), r.kernel()
    kro, kr = dft.ROKS(h2o), dft.RKS(h2o)
    kro.xc = kr.xc = "B3LYP"
    kro.conv_tol = kr.conv_tol = 1e-11
    kr.small_rho_cutoff = 0
    e_kro, e_kr = kro.kernel(), kr.kernel()
    print(f"water: ROHF - RHF = {e_ro - e_r:.2e}, ROKS - RKS (B3LYP) = {e_kro - e_kr:.2e}")
    assert ro.converged and kro.converged and np.all(ro.mo_occ[:5] == 2) and ro.mo_occ.sum() == 10
    assert abs(e_ro - e_r) <= 1e-9 and abs(e_kro - e_kr) <= 1e-8


def test_rohf_never_takes_the_purification_branch_of_the_shared_loop():
    """`UHF._plain_density` purifies each spin's Fock matrix from `sp2_min_nao` basis functions on; ROHF has one effective Fock
    matrix and must diagonalise it at every size.  With the threshold lowered to 1 the run must be the default run."""
    from pyscf import scf
    mol, ref = _rohf("oh")
    mf = scf.ROHF(mol)
    mf.conv_tol, mf.sp2_min_nao = 1e-11, 1
    e = mf.kernel()
    print(f"OH ROHF with sp2_min_nao = 1: E - E(default) = {e - ref.e_tot:.2e}, {mf.cycles} cycles (default {ref.cycles})")
    assert mf.converged and mf.eig_method == "sp2" and abs(e - ref.e_tot) <= 1e-10 and mf.cycles == ref.cycles


@pytest.mark.parametrize("name", ["oh", "o2"])
def test_level_shift_reaches_the_same_state(name):
    """`level_shift` (closed shell unshifted, open shell raised by half, virtuals by the whole shift) leaves a converged solution
    unchanged: same energy to 1e-9 (conv_tol = 1e-11 on both runs) and, the final orbitals coming from the unshifted F_eff, the
    same orbital energies."""
    from pyscf import scf
    mol, ref = _rohf(name)
    mf = scf.ROHF(mol)
    mf.conv_tol, mf.level_shift, mf.max_cycle = 1e-11, 0.3, 100
    e = mf.kernel()
    print(f"{name} ROHF with level_shift = 0.3: E - E(unshifted) = {e - ref.e_tot:.2e}, {mf.cycles} cycles (unshifted {ref.cycles})")
    assert mf.converged and abs(e - ref.e_tot) <= 1e-9
    assert np.abs(np.asarray(mf.mo_energy) - np.asarray(ref.mo_energy)).max() < 1e-5      # the final orbitals are unshifted


@pytest.mark.parametrize("name", ["oh", "ch2"])
def test_rohf_gradient_matches_central_differences(name):
    """Analytic ROHF gradient (the UHF path with W = Da Fa Da + Db Fb Db) against central differences (1e-3 bohr) of the engine's own
    ROHF energy, within the 2e-6 `test_gpu_uhf.py` asks of the UHF gradient; translational invariance to 1e-7."""
    from mi355scf.grad import FDGradients
    mol, mf = _rohf(name)
    g = mf.nuc_grad_method().kernel()
    fd = FDGradients(mf)
    fd.step = 1e-3
    g_fd = fd.kernel()
    print(f"{name}: ROHF gradient\n{g}\nworst |analytic - finite difference| = {np.abs(g - g_fd).max():.2e}, "
          f"sum over atoms {np.abs(g.sum(axis=0)).max():.1e}")
    assert np.abs(g - g_fd).max() < 2e-6
    assert np.abs(g.sum(axis=0)).max() < 1e-7


@functools.lru_cache(maxsize=None)
def _roks_oh():
    from pyscf import dft
    mol = mol_of(OH, "6-31g(d)", 1)
    mf = dft.ROKS(mol).to_gpu()
    mf.xc = "B3LYP"
    mf.conv_tol, mf.conv_tol_grad = 1e-11, 1e-7
    mf.kernel()
    assert mf.converged
    return mol, mf


def test_roks_energy_on_the_oracle_functional():
    """The UKS energy functional at the engine's ROKS densities, evaluated by the oracle (its integrals, its grid, its independent
    spin-polarised B3LYP: `oracle.dft.nr_uks`), within the 2e-7 `test_gpu_uks.py` allows between engine and oracle."""
    from oracle import dft as od
    mol, mf = _roks_oh()
    S, h, eri = oracle_integrals(mol)
    dm = mf.make_rdm1()
    coords, weights = od.build_grids(mol, 3)
    nel, exc, _vxc, hyb = od.nr_uks(mol, coords, weights, "B3LYP", dm)
    D = dm[0] + dm[1]
    J = np.einsum("ijkl,kl->ij", eri, D)
    ex = sum(np.sum(d * np.einsum("ikjl,kl->ij", eri, d)) for d in dm)
    e_ref = np.sum(D * h) + 0.5 * np.sum(D * J) - 0.5 * hyb * ex + exc + mol.energy_nuc()
    print(f"OH ROKS/B3LYP: E = {mf.e_tot:.10f}, engine - oracle functional = {mf.e_tot - e_ref:.2e}, grid electrons {nel}, "
          f"{mf.cycles} cycles, <S^2> = {mf.spin_square()[0]}")
    assert len(weights) == mf.grids.size
    assert abs(mf.e_tot - e_ref) < 2e-7
    assert abs(mf.spin_square()[0] - 0.75) <= 1e-10 and np.all(np.asarray(mf.mo_occ)[:5] == [2, 2, 2, 2, 1])


def test_roks_gradient_matches_frozen_grid_differences():
    """Analytic ROKS/B3LYP gradient of OH (no grid response) against central differences (1e-3 bohr) of the ROKS energy on a grid
    frozen in space, within the 3e-6 of `test_gpu_uks.py`; the sum over atoms within the 5e-5 the suite allows a DFT gradient
    without grid-weight response (`test_gpu_configs.py`)."""
    from pyscf import dft
    mol, mf = _roks_oh()
    g = mf.nuc_grad_method().kernel()
    coords, weights, atom_of = mf.grids.coords, mf.grids.weights, mf.grids.atom_of
    R = mol.atom_coords()
    h = 1e-3
    dm0 = mf.make_rdm1()

    def energy_at(Rn):
        m2 = mol.set_geom_(Rn, unit="Bohr", inplace=False)
        m2.verbose = 0
        f2 = dft.ROKS(m2)
        f2.xc, f2.conv_tol, f2.conv_tol_grad = "B3LYP", 1e-11, 1e-7
        f2._setup_once()
        f2.grids.coords, f2.grids.weights, f2.grids.atom_of = coords, weights, atom_of   # frozen grid
        e = f2.kernel(dm0=dm0)
        assert f2.converged
        return e

    worst = 0.0
    for ia, x in ((0, 2), (1, 2), (1, 0)):
        Rp, Rm = R.copy(), R.copy()
        Rp[ia, x] += h
        Rm[ia, x] -= h
        fd = (energy_at(Rp) - energy_at(Rm)) / (2 * h)
        worst = max(worst, abs(fd - g[ia, x]))
        print(f"OH ROKS/B3LYP dE/dR[{ia}, {x}]: analytic {g[ia, x]:.8f}, finite difference {fd:.8f}")
    print(f"worst difference {worst:.2e}, sum over atoms {np.abs(g.sum(axis=0)).max():.1e}")
    assert worst < 3e-6
    assert np.abs(g.sum(axis=0)).max() < 5e-5


def test_optimize_oh_rohf():
    from pyscf import scf
    from pyscf.geomopt.geometric_solver import optimize
    mol = mol_of(OH, "sto-3g", 1)
    mf = scf.ROHF(mol).to_gpu()
    e0 = mf.kernel()
    mol_opt = optimize(mf, maxsteps=30)
    m2 = scf.ROHF(mol_opt)
    e1 = m2.kernel()
    r = np.linalg.norm(np.diff(mol_opt.atom_coords(), axis=0)) * 0.52917721092
    gmax = np.abs(m2.nuc_grad_method().kernel()).max()
    print(f"OH ROHF/STO-3G: E {e0:.8f} -> {e1:.8f}, r(OH) = {r:.4f} Angstrom, largest gradient element {gmax:.1e}")
    assert m2.converged and e1 < e0 - 1e-6 and gmax < 1e-3
