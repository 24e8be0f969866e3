"""TDA / TDHF / TDDFT excited-state gradients (`td.nuc_grad_method()`, mi355scf/tdscf_grad.py) end to end on the GPU:
central finite differences of E_SCF + w_n, the one-pass two-electron kernel against the term-by-term loop, invariances, the ground
state through `state=0`, an excited-state optimisation, and the refusals.

SCF conv_tol = 1e-11.  TD conv_tol = 1e-14: the Davidson stops at |r| < sqrt(conv_tol) = 1e-7, and the gradient is linear in the
residual of the amplitudes (w itself is quadratic), so 1e-7 is below the 5e-6 of the comparison; at the default 1e-5 the residual
(3e-3) is not.  The SCF's orbital gradient is held below conv_tol_grad = 1e-9 as well: w is not variational in the orbitals, so
an orbital residual r moves E_SCF + w by O(r) and the central difference by r / FD_STEP.  conv_tol = 1e-11 alone stops at
|F_ov| = 7e-8 (water), which moved the DIFFERENCE QUOTIENT by 4.3e-5 while the analytic gradient changed by 4e-9; with 1e-9 the
two agree to 5.7e-7 at FD_STEP and 8e-8 at half of it.  Each test prints its figures (pytest -rP shows them)."""
import warnings

import numpy as np
import pytest

from conftest import MOLECULES

pytestmark = pytest.mark.gpu

TD_TOL = 1e-12
SCF_TOL_GRAD = 1e-9
FD_STEP = 2e-3
GRID_LEVEL = 4


def _scf(mol, xc=None, dm0=None):
    from pyscf import dft, scf
    if xc is None:
        mf = scf.RHF(mol)
    else:
        mf = dft.RKS(mol)
        mf.xc = xc
        mf.grids.level = GRID_LEVEL
    mf.conv_tol = 1e-11
    mf.conv_tol_grad = SCF_TOL_GRAD
    mf.kernel(dm0=dm0)
    assert mf.converged
    return mf


def _td(mf, kind, nstates=3, x0=None):
    from pyscf import tdscf
    td = tdscf.TDA(mf) if kind == "tda" else tdscf.TDDFT(mf)
    td.nstates = nstates
    td.conv_tol = TD_TOL
    td.kernel(x0=x0)
    return td


def _directions(R, seed, n=3):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        v = rng.standard_normal(R.shape)
        out.append(v / np.linalg.norm(v))
    return out


def _mol(name, basis="6-31g(d)"):
    from pyscf import gto
    return gto.M(atom=MOLECULES[name], basis=basis, verbose=0)


# (molecule, xc or None, "tda" | "rpa", state)
FD_CASES = {
    "h2o-cis-1": ("h2o", None, "tda", 1), "h2o-tdhf-2": ("h2o", None, "rpa", 2),
    "h2co-cis-1": ("h2co", None, "tda", 1), "h2co-tdhf-1": ("h2co", None, "rpa", 1),
    "h2o-lda-tda-1": ("h2o", "lda", "tda", 1), "h2o-lda-tddft-1": ("h2o", "lda", "rpa", 1),
    "h2o-b3lyp-tda-1": ("h2o", "b3lyp", "tda", 1), "h2co-b3lyp-tddft-1": ("h2co", "b3lyp", "rpa", 1),
}


@pytest.mark.parametrize("case", list(FD_CASES))
def test_gradient_matches_finite_differences_of_the_energy(case):
    """Central differences of E_SCF + w_n along three fixed random directions (the protocol of test_gpu_casscf_grad.py).
    Hartree-Fock references: |analytic - fd| <= 5e-6 max(1, |g|max).  DFT references: the analytic gradients (ground and excited
    state alike) omit the grid-weight response, so the ground-state discrepancy d_gs against the same differences of E_SCF is
    measured alongside and the excited state may miss by 2 d_gs + 5e-6 max(1, |g|max)."""
    name, xc, kind, state = FD_CASES[case]
    mol = _mol(name)
    mf = _scf(mol, xc)
    td = _td(mf, kind)
    assert bool(td.converged[state - 1])
    gaps = np.abs(np.delete(td.e, state - 1) - td.e[state - 1])
    assert gaps.min() > 5e-3, (case, td.e)            # the state is not degenerate
    grad = td.nuc_grad_method()
    assert grad.algorithm == "onepass"
    g = grad.kernel(state=state)
    assert grad.converged and grad.state == state and np.array_equal(grad.de, g)
    loop = td.nuc_grad_method()
    loop.algorithm = "loop"
    g_loop = loop.grad(state=state)
    d_alg = np.abs(g - g_loop).max()
    g_gs = mf.nuc_grad_method().kernel()
    R = mol.atom_coords()
    net, torque = np.abs(g.sum(axis=0)).max(), np.abs(np.cross(R, g).sum(axis=0)).max()
    print(f"{case}: w = {td.e[state - 1]:.8f}, |g|max = {np.abs(g).max():.6f}, Z-vector {grad.niter} iterations, |onepass - loop| = "
          f"{d_alg:.2e}, |sum g| = {net:.2e}, |sum R x g| = {torque:.2e}; timings onepass {grad.timing}, loop 2e "
          f"{loop.timing['grad_eri']:.3f} s")
    assert d_alg < 1e-9
    if xc is None:
        assert net < 1e-8 and torque < 1e-7            # (a DFT grid without weight response is not invariant)
    dm0, xy0 = mf.make_rdm1(), td.xy
    tol0 = 5e-6 * max(1.0, np.abs(g).max())
    for i, u in enumerate(_directions(R, 17)):
        e_gs, e_ex = [], []
        for sign in (1.0, -1.0):
            mol_d = mol.set_geom_(R + sign * FD_STEP * u, unit="Bohr", inplace=False)
            mol_d.verbose = 0
            mf_d = _scf(mol_d, xc, dm0)
            td_d = _td(mf_d, kind, x0=xy0)
            assert bool(td_d.converged[state - 1])
            e_gs.append(mf_d.e_tot)
            e_ex.append(mf_d.e_tot + td_d.e[state - 1])
        fd_gs, fd_ex = (e_gs[0] - e_gs[1]) / (2 * FD_STEP), (e_ex[0] - e_ex[1]) / (2 * FD_STEP)
        d_gs, d_ex = abs(float(np.sum(g_gs * u)) - fd_gs), abs(float(np.sum(g * u)) - fd_ex)
        tol = tol0 if xc is None else 2.0 * d_gs + tol0
        print(f"{case} direction {i}: excited analytic {float(np.sum(g * u)):+.9f}, finite difference {fd_ex:+.9f}, d_ex = {d_ex:.2e}; "
              f"ground state d_gs = {d_gs:.2e}; tol {tol:.1e}")
        assert d_ex <= tol, (case, i, d_ex, d_gs, tol)


def test_state_zero_is_the_ground_state_gradient():
    mol = _mol("h2o")
    mf = _scf(mol)
    td = _td(mf, "tda")
    g0 = td.Gradients().kernel(state=0)
    ref = mf.nuc_grad_method().kernel()
    d = np.abs(g0 - ref).max()
    print(f"state=0 against mf.nuc_grad_method(): {d:.2e}")
    assert d < 1e-10
    assert np.abs(td.nuc_grad_method().kernel(state=1) - ref).max() > 1e-3


def test_optimize_lowest_singlet_of_formaldehyde():
    """CIS/6-31G(d): the n -> pi* state relaxes by lengthening C=O.  `optimize` takes the gradient object and, afterwards, a
    scanner; the state-following warning must stay silent."""
    from pyscf.geomopt.geometric_solver import optimize
    mol = _mol("h2co")
    bond = lambda m: float(np.linalg.norm(m.atom_coords()[0] - m.atom_coords()[1]))
    mf = _scf(mol)
    td = _td(mf, "tda")
    e0 = mf.e_tot + td.e[0]
    seen = {}

    def callback(env):
        seen["scanner"] = env["energy_grad"]
        seen.setdefault("e", []).append(env["e"])
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        mol_opt = optimize(td.nuc_grad_method(), callback=callback)
        assert mol_opt._opt_converged
        sc = seen["scanner"]
        assert sc.converged and sc.state >= 1 and sc.overlap is not None and sc.overlap > 0.7
        e1 = td._scf.e_tot + td.e[sc.state - 1]
        g = td.nuc_grad_method().kernel(state=sc.state)
        # from the optimum, a scanner object goes straight back in and stops at once
        again = optimize(td.nuc_grad_method().as_scanner(state=sc.state))
        assert again._opt_converged and again._opt_steps <= 2
    assert not [w for w in caught if "overlap" in str(w.message)], [str(w.message) for w in caught]
    print(f"H2CO S1 CIS/6-31G(d): {mol_opt._opt_steps} steps, E {e0:.8f} -> {e1:.8f}, r(CO) {bond(mol):.4f} -> {bond(mol_opt):.4f} "
          f"Bohr, max|g| = {np.abs(g).max():.2e}, last overlap {sc.overlap:.3f}")
    assert np.abs(g).max() < 4.5e-4
    assert e1 < e0 and seen["e"][-1] < e0
    assert bond(mol_opt) > bond(mol)


def test_scanner_warns_when_the_state_is_lost():
    """The followed state is compared with the previous X: handed vectors of a different state it warns, and says which root it
    continues with."""
    mol = _mol("h2o")
    mf = _scf(mol)
    td = _td(mf, "tda")
    sc = td.nuc_grad_method().as_scanner(state=1)
    rng = np.random.default_rng(3)
    td.xy = [(rng.standard_normal(x.shape), np.zeros_like(y)) for x, y in td.xy]     # no state resembles these
    with pytest.warns(UserWarning, match="overlap"):
        e, g = sc(mol)
    assert 1 <= sc.state <= 3 and sc.overlap < 0.7 and g.shape == (3, 3)


def test_refusals():
    from pyscf import dft, scf, tdscf
    from mi355scf import tdscf as mtd
    mol = _mol("h2o", "sto-3g")
    mf = _scf(mol)
    td = _td(mf, "tda", nstates=2)
    g = td.nuc_grad_method()
    with pytest.raises(NotImplementedError, match="above nstates"):
        g.kernel(state=3)
    td.converged = np.array([True, False])
    with pytest.raises(NotImplementedError, match="not converged"):
        g.kernel(state=2)
    tt = tdscf.TDA(mf)
    tt.singlet = False
    with pytest.raises(NotImplementedError, match="triplet"):
        tt.nuc_grad_method()
    cam = dft.RKS(mol)
    cam.xc = "CAM-B3LYP"
    with pytest.raises(NotImplementedError, match="range-separated"):
        tdscf.TDDFT(cam).nuc_grad_method()
    with pytest.raises(NotImplementedError, match="PCM"):
        mtd.TDA(scf.RHF(mol).PCM()).nuc_grad_method()
    sharded = scf.RHF(mol)
    sharded._nranks = 2
    ts = mtd.TDA(sharded)
    ts.e, ts.xy, ts.converged = td.e, td.xy, np.array([True, True])
    with pytest.raises(NotImplementedError, match="sharded"):
        ts.nuc_grad_method().kernel(state=1)
    direct = scf.RHF(mol)
    direct.kernel()
    direct._stream_groups = 2
    tdm = mtd.TDA(direct)
    tdm.e, tdm.xy, tdm.converged = td.e, td.xy, np.array([True, True])
    with pytest.raises(NotImplementedError, match="direct mode"):
        tdm.nuc_grad_method().kernel(state=1)
    # the Z-vector solver reports non-convergence instead of returning a gradient
    g1 = td.nuc_grad_method()
    td.converged = np.array([True, True])
    g1.max_cycle = 1
    g1.conv_tol = 1e-14
    with pytest.raises(RuntimeError, match="did not converge"):
        g1.kernel(state=1)
    assert g1.converged is False
