"""C-PCM on the MI355X (mi355scf/pcm.py, `mi_pcm_*` kernels): the surface-charge integrals against the CPU oracle's
McMurchie-Davidson ERIs, the two per-cycle passes against torch products on the same store, the variational Fock term,
PCM-RHF / PCM-RKS energies against a CPU reference SCF, eps = 1, Gauss's law, gradients and the solvent template's flows."""
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

WATER = "O 0 0 0; H 0 -0.757 0.587; H 0 0.757 0.587"
ACETIC = ("C -1.3940 -0.0790 0.0000; C 0.0900 0.1670 0.0000; O 0.6110 1.2560 0.0000; O 0.8140 -0.9740 0.0000; "
          "H -1.9000 0.8860 0.0000; H -1.6730 -0.6530 0.8840; H -1.6730 -0.6530 -0.8840; H 1.7540 -0.7380 0.0000")
H3O = "O 0 0 0.1; H 0 0.94 -0.25; H 0.814 -0.47 -0.25; H -0.814 -0.47 -0.25"


def _mol(atom, basis="6-31G*", charge=0):
    from pyscf import gto
    m = gto.Mole()
    m.atom, m.basis, m.charge, m.verbose = atom, basis, charge, 0
    m.build()
    return m


def _pcm(mol, xc=None, eps=78.3553, **kw):
    from pyscf import dft, scf, solvent
    if xc is None:
        mf = scf.RHF(mol)
    else:
        mf = dft.RKS(mol)
        mf.xc = xc
    for k, v in kw.items():
        setattr(mf, k, v)
    mf = solvent.PCM(mf)
    mf.eps = eps
    return mf


def _with_points(mol, coords, zeta):
    """`mol` plus one normalised s shell of exponent zeta^2/2 at every point: (mn|kk) = B_g,mn exactly."""
    from mi355scf.mole import gto_norm
    atm, bas, env = [mol._atm.copy()], [mol._bas.copy()], list(mol._env)
    natm = mol._atm.shape[0]
    for i, (c, z) in enumerate(zip(coords, zeta)):
        pc = len(env)
        env.extend(list(c) + [0.0])
        a = 0.5 * z * z
        pe = len(env)
        env.extend([a, gto_norm(0, a)])
        atm.append(np.array([[0, pc, 1, 0, 0, 0]], dtype=np.int32))
        bas.append(np.array([[natm + i, 0, 1, 1, 0, pe, pe + 1, 0]], dtype=np.int32))
    return SimpleNamespace(_atm=np.concatenate(atm), _bas=np.concatenate(bas), _env=np.asarray(env), nao=mol.nao + len(zeta))


def _oracle_B(mol, coords, zeta, rows=None):
    """B [len(rows), nao, nao] from the oracle's ERIs."""
    from oracle import oracle as orc
    ext = _with_points(mol, coords, zeta)
    o = orc.Oracle(ext)
    nb = mol._bas.shape[0]
    loc = mol.ao_loc_nr()
    rows = range(len(zeta)) if rows is None else rows
    out = np.zeros((len(rows), mol.nao, mol.nao))
    for r, g in enumerate(rows):
        k = nb + g
        for i in range(nb):
            for j in range(i + 1):
                blk = o.eri_shell(i, j, k, k)[:, :, 0, 0]
                out[r, loc[i]:loc[i + 1], loc[j]:loc[j + 1]] = blk
                out[r, loc[j]:loc[j + 1], loc[i]:loc[i + 1]] = blk.T
    return out


def _unpack(Brow, nao):
    m, n = np.tril_indices(nao)
    M = np.zeros((nao, nao))
    M[m, n] = Brow[m * (m + 1) // 2 + n]
    M[n, m] = M[m, n]
    return M


@pytest.mark.parametrize("basis", ["6-31G(d,p)", "cc-pVTZ"])
def test_B_matches_oracle_eris(basis):
    """Sampled rows of the resident store (smallest and largest zeta included) against (mn|kk) of the oracle."""
    from mi355scf import engine
    mol = _mol(WATER, basis)
    mf = _pcm(mol)
    mf._setup_once()
    ws = mf.with_solvent.build(mf.engine, mol)
    s = ws.surface
    order = np.argsort(s.zeta)
    rows = sorted({int(order[0]), int(order[-1]), int(order[len(order) // 2])} | set(range(0, s.npts, max(1, s.npts // 9))))
    ref = _oracle_B(mol, s.coords[rows], s.zeta[rows])
    B = ws._B[rows].cpu().numpy()
    for r in range(len(rows)):
        err = np.abs(_unpack(B[r], mol.nao) - ref[r]).max()
        assert err < 1e-11, (basis, rows[r], err)
    assert np.all(ws._B[:, mol.nao * (mol.nao + 1) // 2:].cpu().numpy() == 0.0)   # padding columns
    assert isinstance(engine.Engine, type)


def test_per_cycle_passes_match_torch():
    mol = _mol(ACETIC)
    mf = _pcm(mol)
    mf._setup_once()
    ws = mf.with_solvent.build(mf.engine, mol)
    eng, n = mf.engine, mol.nao
    torch.manual_seed(3)
    A = torch.randn(n, n, dtype=torch.float64, device=eng.device)
    D = (A + A.T).contiguous()
    v = torch.empty(ws.surface.npts, dtype=torch.float64, device=eng.device)
    eng.pcm_potential(ws._B, ws.ld, D, ws._dpack, None, v)
    m, k = np.tril_indices(n)
    w = torch.as_tensor(np.where(m == k, 1.0, 2.0), device=eng.device)
    cols = torch.as_tensor(m * (m + 1) // 2 + k, device=eng.device)
    Bp = ws._B[:, cols]
    ref = Bp @ (D[m, k] * w)
    assert (torch.abs(v - ref).max() / torch.abs(ref).max()).item() < 1e-12
    q = torch.randn(ws.surface.npts, dtype=torch.float64, device=eng.device)
    V = torch.empty(n, n, dtype=torch.float64, device=eng.device)
    eng.pcm_fock(ws._B, ws.ld, q, -1.0, False, ws._part, V)
    Vr = torch.zeros(n, n, dtype=torch.float64, device=eng.device)
    Vr[m, k] = -(q @ Bp)
    Vr[k, m] = Vr[m, k]
    assert (torch.abs(V - Vr).max() / torch.abs(Vr).max()).item() < 1e-12
    assert torch.equal(V, V.T)
    V2 = V.clone()
    eng.pcm_fock(ws._B, ws.ld, q, 0.5, True, ws._part, V2)      # accumulate mode
    assert torch.allclose(V2, 0.5 * V, rtol=1e-13, atol=1e-15)


def test_fock_term_is_variational():
    mol = _mol(WATER)
    mf = _pcm(mol)
    mf.kernel()
    ws = mf.with_solvent
    D = mf._dm
    V, _e = ws.vpcm(D)
    rng = np.random.default_rng(5)
    X = rng.normal(size=D.shape)
    dD = torch.as_tensor(1e-4 * (X + X.T), device=D.device)
    h = 1.0
    ep = ws.energy(D + h * dD)
    em = ws.energy(D - h * dD)
    fd = (ep - em) / (2 * h)
    an = float(torch.sum(V * dD))
    assert abs(fd - an) < 1e-9 * max(1.0, abs(an)), (fd, an)


def _cpu_pcm(mol, eps, xc=None):
    """CPU reference: the oracle's SCF loop with the numpy PCM term (B from the oracle ERIs, S / v_n from pcm's host code)."""
    from mi355scf import pcm
    from oracle import oracle as orc
    s = pcm.Surface(mol.atom_coords(), pcm.atom_radii_bohr(mol), 302)
    Bf = _oracle_B(mol, s.coords, s.zeta).reshape(s.npts, -1)
    S = pcm.s_matrix(s.coords, s.zeta, s.swf).numpy()
    K = pcm.scaling_factor(eps) * np.linalg.inv(S)
    vn = pcm.v_nuc(s.coords, s.zeta, mol.atom_coords(), mol.atom_charges()).numpy()
    o = orc.Oracle(mol)
    if xc is None:
        def base(dm):
            J, Kx = o.jk(dm)
            v = J - 0.5 * Kx
            return v, 0.5 * float(np.sum(dm * v))
    else:
        from oracle import dft as odft
        coords, weights = odft.build_grids(mol, 3)

        def base(dm):
            _n, exc, vxc, hyb = odft.nr_rks(mol, coords, weights, xc, dm)
            J, Kx = o.jk(dm)
            v = J + vxc - 0.5 * hyb * Kx
            return v, 0.5 * float(np.sum(dm * J)) + exc - 0.25 * hyb * float(np.sum(dm * Kx))

    def veff(dm):
        v, e2 = base(dm)
        vv = vn - Bf @ dm.ravel()
        q = -K @ vv
        return v - (q @ Bf).reshape(dm.shape), e2 + 0.5 * q @ vv

    return orc.rhf(mol, veff_fn=veff, conv_tol=1e-11, oracle=o)


@pytest.mark.parametrize("atom,xc", [(WATER, None), (ACETIC, None), (WATER, "B3LYP"), (WATER, "PBE")])
def test_energy_matches_cpu_reference(atom, xc):
    mol = _mol(atom)
    mf = _pcm(mol, xc, small_rho_cutoff=0.0) if xc else _pcm(mol)
    mf.conv_tol = 1e-11
    e = mf.kernel()
    assert mf.converged
    ref = _cpu_pcm(mol, 78.3553, xc)
    assert abs(e - ref["e_tot"]) < 1e-8, (e, ref["e_tot"])
    ws = mf.with_solvent
    assert ws.e < 0 and ws.q.shape == (ws.surface.npts,)
    assert abs(mf.energy_tot(mf.make_rdm1()) - e) < 1e-8


def test_eps_one_is_gas_phase():
    from pyscf import scf
    mol = _mol(WATER)
    mf = _pcm(mol, eps=1.0)
    mf.conv_tol = 1e-11
    e = mf.kernel()
    g = scf.RHF(_mol(WATER))
    g.conv_tol = 1e-11
    assert mf.with_solvent.e == 0.0 and abs(e - g.kernel()) < 1e-10
    assert np.abs(mf.nuc_grad_method().kernel() - g.nuc_grad_method().kernel()).max() < 1e-7


def test_gauss_law_for_a_cation():
    """H3O+: the surface holds about -f Q.  Observed outlying charge (1 + sum q / f) is recorded in the assertion message;
    the bound of 2 % covers the electron density outside the cavity and the Lebedev discretisation."""
    mol = _mol(H3O, charge=1)
    mf = _pcm(mol)
    mf.kernel()
    ws = mf.with_solvent
    f = ws.f
    total = ws.q.sum()
    assert abs(total + f * 1.0) < 0.02 * f, (total, -f)


def _fd(mol, xc, ia, x, h=1e-3):
    out = []
    for sg in (1, -1):
        X = mol.atom_coords().copy()
        X[ia, x] += sg * h
        m = mol.set_geom_(X, unit="Bohr", inplace=False)
        m.verbose = 0
        mf = _pcm(m, xc)
        mf.conv_tol = 1e-11
        out.append(mf.kernel())
    return (out[0] - out[1]) / (2 * h)


@pytest.mark.parametrize("xc,tol", [(None, 1e-6), ("B3LYP", 2e-4)])
def test_gradient_matches_finite_differences(xc, tol):
    """B3LYP: test_gpu_grad.py's tolerance (no grid-weight response, as PySCF's default), which also breaks the translational
    invariance of the total at ~1e-5; the solvent terms alone sum to zero in both cases."""
    mol = _mol(WATER)
    mf = _pcm(mol, xc)
    mf.conv_tol = 1e-11
    mf.kernel()
    g = mf.nuc_grad_method().kernel()
    assert np.abs(mf.with_solvent.grad(mf._dm).sum(axis=0)).max() < 1e-7
    if xc is None:
        assert np.abs(g.sum(axis=0)).max() < 1e-7
    for ia, x in ((0, 2), (1, 1), (2, 2)):
        fd = _fd(mol, xc, ia, x)
        assert abs(g[ia, x] - fd) < tol, (ia, x, g[ia, x], fd)


def test_optimize_in_water_moves_the_geometry():
    from pyscf import scf
    from pyscf.geomopt.geometric_solver import optimize
    mol = _mol(WATER)
    m_gas = optimize(scf.RHF(_mol(WATER)), maxsteps=30)
    m_sol = optimize(_pcm(mol), maxsteps=30)
    assert m_gas._opt_converged and m_sol._opt_converged
    assert np.abs(m_sol.atom_coords() - m_gas.atom_coords()).max() > 1e-3


def test_density_fitting_with_pcm():
    mol = _mol(WATER)
    from pyscf import scf, solvent
    gas = scf.RHF(mol).kernel()
    sol = _pcm(mol).kernel()
    dgas = scf.RHF(mol).density_fit().kernel()
    dsol = solvent.PCM(scf.RHF(mol).density_fit())
    dsol.eps = 78.3553
    dsol = dsol.kernel()
    # the solvent term does not depend on the J/K route: the solvation energies differ by less than the fitting error itself
    assert abs((dsol - dgas) - (sol - gas)) < max(1e-6, abs(dgas - gas)), (dsol - dgas, sol - gas, dgas - gas)


@pytest.mark.parametrize("method", ["HF", "B3LYP"])
def test_solvent_template_flows(method):
    """calculate_solvent_effect.py's sequences on acetic acid / 6-31G*: gas phase, then PCM per solvent (mf.eps set on the
    wrapped object), the properties it reads; solvation energies finite, negative and growing in magnitude with f."""
    from pyscf import dft, scf, solvent
    eps = {"hexane": 1.88, "benzene": 2.27, "chloroform": 4.89, "ethanol": 24.55, "water": 78.39}
    mol = _mol(ACETIC)

    def make():
        if method == "HF":
            return scf.RHF(mol)
        mf = dft.RKS(mol)
        mf.xc = method
        return mf

    gas = make()
    e_gas = gas.kernel()
    dsolv = []
    for name in sorted(eps, key=eps.get):
        mf = solvent.PCM(make())
        mf.eps = eps[name]
        e = mf.kernel()
        dip = mf.dip_moment(mf.mol, mf.make_rdm1(), unit="Debye")
        homo = np.where(mf.mo_occ > 0)[0][-1]
        assert np.isfinite(e) and np.all(np.isfinite(dip)) and mf.mo_energy[homo + 1] > mf.mo_energy[homo]
        dsolv.append(e - e_gas)
    dsolv = np.array(dsolv)
    assert np.all(dsolv < 0) and np.all(np.diff(dsolv) < 0), dsolv
