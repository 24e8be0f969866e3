"""Grid-weight response host references (no GPU): a NumPy restatement of the Becke cell functions that accepts COMPLEX
coordinates, and its complex-step derivative with every grid point riding on its parent atom.  The GPU tests
(test_gpu_grid_response.py) check `mi_grid_becke_grad` against `becke_weight_jacobian`, so it is validated here against something
independent: the oracle's weights at zero step, Richardson central differences of the oracle's weights, and -- together with a
NumPy transcription of the XC force -- the identity dE_xc/dR = T1 + T2 + T3 against differences of the oracle's E_xc with the
grid rebuilt at every geometry."""
import numpy as np
import pytest

from conftest import MOLECULES

STEP = 1e-30


def make_mol(atom, basis="sto-3g", spin=0):
    from pyscf import gto
    mol = gto.Mole()
    mol.atom, mol.basis, mol.spin, mol.verbose = atom, basis, spin, 0
    mol.build()
    return mol


def atom_grids(mol, level):
    """(s [ng, 3] point positions relative to the parent atom, vol [ng], atom_of [ng], a [natm, natm]) of the oracle's grid
    (`oracle.dft.build_grids`: same radial and angular rules, same pruning, same order)."""
    from oracle import dft as odft
    zs = mol.atom_charges()
    ss, vs, own = [], [], []
    for ia in range(mol.natm):
        z = int(zs[ia])
        r, dr = odft.treutler_ahlrichs(odft._RAD[level][odft._period(z)], z)
        rw = 4 * np.pi * r * r * dr
        angs = odft.nwchem_prune(z, r, odft._ANG[level][odft._period(z)])
        for n in sorted(set(angs.tolist())):
            x, w = odft.lebedev(n)
            idx = np.where(angs == n)[0]
            ss.append(np.einsum("i,jk->jik", r[idx], x).reshape(-1, 3))
            vs.append(np.einsum("i,j->ji", rw[idx], w).ravel())
            own.append(np.full(len(vs[-1]), ia, dtype=np.int32))
    return np.vstack(ss), np.hstack(vs), np.hstack(own), adjust_matrix(zs)


def adjust_matrix(zs):
    """Treutler's a_ij from the square roots of the Bragg radii, clipped to +-1/2 (antisymmetric to the bit)."""
    from oracle import dft as odft
    rad = np.sqrt(np.array([odft._BRAGG[int(z)] / odft.BOHR for z in zs]))
    rr = rad[:, None] / rad[None, :]
    return np.ascontiguousarray(np.clip(0.25 * (rr.T - rr), -0.5, 0.5))


def _norm(d):
    """sqrt(d . d) along the last axis: analytic in complex arguments (no conjugate, unlike np.linalg.norm)."""
    return np.sqrt((d * d).sum(axis=-1))


def _switch(mu, a):
    """s(nu(mu)): Treutler shift, the three-fold Becke polynomial, s = (1 - f3) / 2; also 1 - s as (1 + f3) / 2."""
    f = mu + a * (1.0 - mu * mu)
    for _ in range(3):
        f = (3.0 - f * f) * f * 0.5
    return 0.5 * (1.0 - f), 0.5 * (1.0 + f)


def switch_matrix(coords, R, a):
    """s[i, j, g] = s(nu_ij) at the points (s[i, i] = 1), so that the cell function P_i is s[i].prod(axis=0)."""
    natm = len(R)
    r = _norm(coords[None, :, :] - R[:, None, :])                       # [natm, ng]
    Rij = _norm(R[:, None, :] - R[None, :, :]) + np.eye(natm)
    mu = (r[:, None, :] - r[None, :, :]) / Rij[:, :, None]
    s, _ = _switch(mu, a[:, :, None])
    s[np.arange(natm), np.arange(natm)] = 1.0
    return s


def becke_partition(coords, atom_of, R, a):
    """P_o / sum_B P_B at the points (real or complex coordinates)."""
    P = switch_matrix(coords, R, a).prod(axis=1)
    return P[atom_of, np.arange(len(atom_of))] / P.sum(axis=0)


def _exclusive_products(s):
    """x[i, c, g] = prod_{k != c} s[i, k, g], division-free (prefix times suffix products)."""
    x = np.ones_like(s)
    x[:, 1:] *= np.cumprod(s, axis=1)[:, :-1]
    x[:, :-1] *= np.cumprod(s[:, ::-1], axis=1)[:, ::-1][:, 1:]
    return x


def becke_weight_jacobian(s_loc, atom_of, R, a, sparse=True):
    """dW[g, C, k] = d [P_o / sum_B P_B](R_o + s_g; R) / dR_Ck by the complex step (1e-30: no subtraction, no step error).
    sparse=False perturbs R_C and evaluates everything again.  sparse=True evaluates the same complex-step expression but
    touches only what R_C enters: the points of atom C (which move) in full, and at the other points the factors s_iC and
    s_Ci, the rest of every product coming from the real exclusive products."""
    natm, ng = len(R), len(s_loc)
    coords = R[atom_of] + s_loc
    dW = np.zeros((ng, natm, 3))
    if sparse:
        r = _norm(coords[None, :, :] - R[:, None, :])
        excl = _exclusive_products(switch_matrix(coords, R, a))
    for C in range(natm):
        mine = np.where(atom_of == C)[0]
        rest = np.where(atom_of != C)[0]
        for k in range(3):
            Rc = R.astype(np.complex128)
            Rc[C, k] += 1j * STEP
            if not sparse:
                dW[:, C, k] = becke_partition(Rc[atom_of] + s_loc, atom_of, Rc, a).imag / STEP
                continue
            if len(mine):
                dW[mine, C, k] = becke_partition(Rc[C] + s_loc[mine], atom_of[mine], Rc, a).imag / STEP
            if len(rest):
                rC = _norm(coords[rest] - Rc[C])
                RiC = _norm(R - Rc[C])
                RiC[C] = 1.0
                s_iC, s_Ci = _switch((r[:, rest] - rC[None, :]) / RiC[:, None], a[:, C][:, None])
                s_iC[C] = s_Ci[C] = 1.0
                P = excl[:, C, :][:, rest] * s_iC
                P[C] = s_Ci.prod(axis=0)
                dW[rest, C, k] = (P[atom_of[rest], np.arange(len(rest))] / P.sum(axis=0)).imag / STEP
    return dW


def becke_grad_reference(s_loc, atom_of, R, a, vol, e, dW=None):
    """out[C, k] = sum_g e_g vol_g dW[g, C, k]: what `mi_grid_becke_grad` adds."""
    dW = becke_weight_jacobian(s_loc, atom_of, R, a) if dW is None else dW
    return np.einsum("g,gck->ck", e * vol, dW)


def richardson(f, R, h=1e-3):
    """d f / d R [natm, 3] from central differences at h and 2 h, extrapolated: (4 D(h) - D(2h)) / 3."""
    out = np.zeros(R.shape)
    for ia in range(R.shape[0]):
        for x in range(3):
            d = []
            for hh in (h, 2 * h):
                Rp, Rm = R.copy(), R.copy()
                Rp[ia, x] += hh
                Rm[ia, x] -= hh
                d.append((f(Rp) - f(Rm)) / (2 * hh))
            out[ia, x] = (4.0 * d[0] - d[1]) / 3.0
    return out


# ---------------------------------------------------------------------------------------------
# the XC force at fixed density: T1 (AO centres move), T2 (points move), the integrand of grad._add_xc_force in NumPy
# ---------------------------------------------------------------------------------------------
_D2 = {(0, 0): 4, (0, 1): 5, (0, 2): 6, (1, 1): 7, (1, 2): 8, (2, 2): 9}


def xc_force_terms(mol, xc, dm, coords, weights, atom_of, rho_cut=1e-10):
    """(T1 [natm, 3], T2 [natm, 3], e [ng]) of a closed-shell LDA / GGA density with the oracle's functional and density floor:
    integrand[g, mu, k] = -2 [dphi_mu (2 wv0 (D phi) + sum_j wv_j (D d_j phi)) + (sum_j wv_j d_j d_k phi_mu) (D phi)_mu];
    T1_C sums it over the AOs of atom C and all points, T2_C = -(sum over all AOs and the points of atom C)."""
    from oracle import dft as odft
    _hyb, terms = odft.parse_xc(xc)
    ao = odft.eval_ao(mol, coords, 2)
    c0 = ao[0] @ dm
    ck = [ao[1 + j] @ dm for j in range(3)]
    rho = np.einsum("gi,gi->g", ao[0], c0)
    grad = np.array([2 * np.einsum("gi,gi->g", ao[1 + k], c0) for k in range(3)])
    ok = rho > rho_cut
    e, vr, vs = odft.eval_xc(terms, np.where(ok, rho, 1.0), np.where(ok, (grad * grad).sum(axis=0), 0.0))
    e, vr, vs = np.where(ok, e, 0), np.where(ok, vr, 0), np.where(ok, vs, 0)
    wv = [0.5 * weights * vr] + [2 * weights * vs * grad[k] for k in range(3)]
    t1 = 2.0 * wv[0][:, None] * c0 + sum(wv[1 + j][:, None] * ck[j] for j in range(3))
    integrand = np.zeros(ao[0].shape + (3,))
    for k in range(3):
        t2 = sum(wv[1 + j][:, None] * ao[_D2[(min(j, k), max(j, k))]] for j in range(3))
        integrand[:, :, k] = -2.0 * (ao[1 + k] * t1 + t2 * c0)
    sl = mol.aoslice_by_atom()
    T1 = np.array([integrand[:, sl[ia, 2]:sl[ia, 3]].sum(axis=(0, 1)) for ia in range(mol.natm)])
    T2 = np.zeros((mol.natm, 3))
    np.subtract.at(T2, atom_of, integrand.sum(axis=1))
    return T1, T2, e


def seeded_density(mol, seed=7):
    """An idempotent closed-shell density (D S D = 2 D) from a seeded random occupied space."""
    from oracle import oracle as orc
    S = orc.Oracle(mol).int1e()[0]
    w, v = np.linalg.eigh(S)
    X = v / np.sqrt(w)
    Q = np.linalg.qr(np.random.default_rng(seed).standard_normal((mol.nao, mol.nao)))[0]
    C = X @ Q[:, :mol.nelectron // 2]
    return 2.0 * C @ C.T


# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,level", [("h2o", 1), ("h2o", 3), ("hf", 1), ("ch4", 1)])
def test_partition_matches_oracle_weights(name, level):
    from oracle import dft as odft
    mol = make_mol(MOLECULES[name])
    s, vol, own, a = atom_grids(mol, level)
    R = mol.atom_coords()
    coords, w = odft.build_grids(mol, level)
    assert np.array_equal(coords, R[own] + s)
    err = np.abs(vol * becke_partition(coords, own, R, a) - w).max()
    print(f"{name} level {level}: {len(w)} points, max |w - w_oracle| = {err:.2e}")
    assert err <= 1e-13


@pytest.mark.parametrize("name", ["h2o", "ch4"])
def test_sparse_complex_step_is_the_plain_one(name):
    mol = make_mol(MOLECULES[name])
    s, _vol, own, a = atom_grids(mol, 0)
    pick = np.random.default_rng(1).choice(len(s), 300, replace=False)
    pick.sort()
    R = mol.atom_coords()
    full = becke_weight_jacobian(s[pick], own[pick], R, a, sparse=False)
    fast = becke_weight_jacobian(s[pick], own[pick], R, a, sparse=True)
    err = np.abs(full - fast).max()
    print(f"{name}: max |dW| = {np.abs(full).max():.3e}, sparse - plain = {err:.2e}")
    assert err <= 1e-14 * np.abs(full).max()
    assert np.abs(full.sum(axis=1)).max() <= 1e-13 * np.abs(full).max()   # the partition is translationally invariant


def test_complex_step_matches_oracle_weight_differences():
    """sum_g c_g dw_g/dR of H2O (level 1) against Richardson central differences of the oracle's weights.  The contraction
    vector is seeded noise in [-1, 1] under the envelope exp(-2 |r - R_parent|) of an energy density: the differences carry
    the rounding of sum_g |c_g w_g| divided by the step, 2e-16 * 10 / 1e-3 = 2e-12 with the envelope, but 1e-9 without it
    (the outermost shells of a level-1 grid weigh 1e3 Bohr^3 a point), which would bury the 1e-10 this test resolves."""
    from oracle import dft as odft
    mol = make_mol(MOLECULES["h2o"])
    s, vol, own, a = atom_grids(mol, 1)
    c = np.random.default_rng(3).uniform(-1.0, 1.0, len(vol)) * np.exp(-2.0 * np.linalg.norm(s, axis=1))
    R = mol.atom_coords()
    got = becke_grad_reference(s, own, R, a, vol, c)

    def contracted(Rd):
        return float(c @ odft.build_grids(mol.set_geom_(Rd, unit="Bohr", inplace=False), 1)[1])
    ref = richardson(contracted, R)
    err = np.abs(got - ref).max()
    print(f"max |component| = {np.abs(ref).max():.3e}, complex step - Richardson = {err:.2e}")
    assert err <= 1e-10


@pytest.mark.parametrize("xc,level", [("B3LYP", 1), ("PBE", 3)])
def test_t1_t2_t3_is_the_derivative_of_exc(xc, level):
    """H2O/STO-3G, seeded idempotent density held fixed: T1 + T2 + T3 against Richardson differences of the oracle's E_xc with
    the grid rebuilt at each geometry.  1e-7 is 4 000 times below the response T2 + T3 it has to resolve."""
    from oracle import dft as odft
    mol = make_mol(MOLECULES["h2o"])
    dm = seeded_density(mol)
    s, vol, own, a = atom_grids(mol, level)
    R = mol.atom_coords()
    coords = R[own] + s
    w = vol * becke_partition(coords, own, R, a)
    T1, T2, e = xc_force_terms(mol, xc, dm, coords, w, own)
    T3 = becke_grad_reference(s, own, R, a, vol, e)

    def exc(Rd):
        m = mol.set_geom_(Rd, unit="Bohr", inplace=False)
        return odft.nr_rks(m, *odft.build_grids(m, level), xc, dm)[1]
    ref = richardson(exc, R)
    err = np.abs(T1 + T2 + T3 - ref).max()
    print(f"{xc} level {level}: |T2| {np.abs(T2).max():.3f} |T3| {np.abs(T3).max():.3f} |T2 + T3| {np.abs(T2 + T3).max():.2e} "
          f"T1 + T2 + T3 - FD = {err:.2e}; sums: T3 {np.abs(T3.sum(axis=0)).max():.1e}, T1 + T2 {np.abs((T1 + T2).sum(axis=0)).max():.1e}")
    assert err <= 1e-7
    assert np.abs(T1 - ref).max() > 1e-5        # without the response the gradient is not the derivative of this energy
