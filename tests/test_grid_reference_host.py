"""Host checks of tests/grid_reference.py, the long-double references of the GPU grid-kernel tests: they agree with the FP64
oracle (oracle/dft.py) to the rounding of FP64 -- which is also the yardstick the GPU bounds are sized from, re-measured here on
the very inputs the GPU tests use -- and the hand-made inputs have the properties the GPU tests rely on.  No GPU.
Each test prints its figures (pytest -rP shows them)."""
import numpy as np
import pytest

import grid_reference as gr
from conftest import MOLECULES

U = 2.0 ** -53
FLOOR = 64 * 2.0 ** -1022
WATER = MOLECULES["h2o"]


def _mol(atom, basis, **kw):
    from mi355scf.mole import Mole
    return Mole(atom=atom, basis=basis, verbose=0, **kw).build()


def _ao_mol(name):
    from test_gpu_pcm_kernels import _synthetic_with_ghost          # 4 centres (one a ghost), one shell of each l = 0..3 on each
    return _synthetic_with_ghost() if name == "synthetic" else _mol(WATER, "cc-pvtz")


@pytest.mark.parametrize("name", ["synthetic", "water"])
def test_ao_reference_agrees_with_oracle_and_yardstick(name):
    """oracle.dft.eval_ao (FP64 NumPy, the same formula) against `ao_reference` on the GPU test's points, all ten components:
    the worst |oracle - ref| / (u majorant + floor / 16) is the yardstick of the GPU bound 16 u majorant + floor.
    Measured: 3.60 on the synthetic molecule (value 3.59, gradient 3.60, second derivatives 3.53), 3.89 on water/cc-pVTZ (value
    and gradient 3.39, second derivatives 3.89).  Asserted below 5: the GPU bound keeps a factor 3 or more over it."""
    from oracle import dft as odft
    mol = _ao_mol(name)
    pts = gr.ao_points(mol)
    ref, maj = gr.ao_reference(mol, pts, 2)
    got = odft.eval_ao(mol, pts, 2)
    ratio = np.abs((got - ref).astype(np.float64)) / (U * maj.astype(np.float64) + FLOOR / 16)
    worst = ratio.reshape(10, -1).max(axis=1)
    print(f"[yardstick] eval_ao {name}: FP64 oracle / (u majorant) per component = {np.round(worst, 2).tolist()}")
    assert worst.max() < 5.0
    for deriv in (0, 1):                       # the lower orders are the leading components of the higher ones
        r, m = gr.ao_reference(mol, pts, deriv)
        n = gr.NCOMP[deriv]
        assert np.array_equal(r, ref[:n]) and np.array_equal(m, maj[:n])
    assert np.all(maj >= np.abs(ref))


@pytest.mark.parametrize("name", ["synthetic", "water"])
def test_ao_points_have_the_stated_properties(name):
    mol = _ao_mol(name)
    pts, R = gr.ao_points(mol), mol.atom_coords()
    assert pts.shape == (gr.NG_FULL, 3) and gr.NG_FULL > 1024
    assert np.array_equal(pts[:mol.natm], R)                                        # on every centre, the ghost included
    off = np.linalg.norm(pts[4] - R[-1])
    assert 0.5e-9 < off < 2e-9
    ref, _ = gr.ao_reference(mol, pts, 0)
    tiny = np.abs(ref[0][gr.AO_TINY].astype(np.float64))
    print(f"[inputs] {name}: |ao| at the tail point in [{tiny.min():.3g}, {tiny.max():.3g}]")
    if name == "synthetic":
        assert tiny.min() > 1e-300 and tiny.max() < 1e-30
    else:
        # cc-pVTZ spans exponents from 0.10 (H s) to 1.43 (O f) on centres 1.8 Bohr apart: where the most diffuse AO is below
        # 1e-30 (r > 26 Bohr) the tightest has underflowed, so no point puts all of them in that window.  At 16 Bohr none has
        # underflowed yet and every one is far down its tail.
        assert tiny.min() > 1e-300 and tiny.max() < 1e-10
    amin = min(float(mol._env[b[5]:b[5] + b[2]].min()) for b in mol._bas)
    r2 = ((pts[gr.AO_FAR] - R) ** 2).sum(axis=1).min()
    assert amin * r2 > 760.0                                                      # exp(-745.2) is the last subnormal
    assert np.abs(ref[0][gr.AO_FAR].astype(np.float64)).max() == 0.0
    if name == "water":                                                           # long contractions with mixed signs
        assert mol._bas[:, 2].max() >= 8
        assert any(np.ptp(np.sign(mol._env[b[6]:b[6] + b[2]])) == 2 for b in mol._bas)


def _becke_fp64(coords, atom_of, vol, R, a):
    """The kernel's formula in FP64 NumPy (every ordered pair): the yardstick of the Becke bound."""
    natm = R.shape[0]
    r = np.sqrt(((coords[:, None, :] - R[None]) ** 2).sum(axis=2))
    Rij = np.sqrt(((R[:, None] - R[None]) ** 2).sum(axis=2))
    P = np.ones_like(r)
    for i in range(natm):
        oth = np.arange(natm) != i
        mu = (r[:, i:i + 1] - r[:, oth]) / Rij[i, oth][None]
        mu = mu + a[i, oth][None] * (1 - mu * mu)
        for _ in range(3):
            mu = (3 - mu * mu) * mu * 0.5
        P[:, i] = np.prod(0.5 * (1 - mu), axis=1)
    return vol * P[np.arange(len(vol)), atom_of] / P.sum(axis=1)


@pytest.mark.parametrize("natm", [85, 86, 100])
def test_becke_case_properties_and_yardstick(natm):
    """Measured: the FP64 evaluation is within 1.31e-15, 1.35e-15, 1.41e-15 vol of the long-double reference at natm = 85, 86,
    100 (the GPU bound 2e-14 vol is 14 times that); the smallest sum_i P_i is 4.5e-2, 1.1e-2, 6.3e-2."""
    coords, atom_of, vol, R, a = gr.becke_case(natm)
    assert coords.shape == (gr.NG_FULL, 3) and R.shape == (natm, 3)
    assert not R[:3, 1:].any() and np.array_equal(R[:3, 0], gr.BECKE_SPACING * np.arange(3))      # exactly collinear
    i, j = gr.BECKE_CLIP
    assert a[i, j] == 0.5 and a[j, i] == -0.5 and np.array_equal(a, -a.T) and np.count_nonzero(np.abs(a) == 0.5) == 2
    near = np.linalg.norm(coords[:, None] - R[None], axis=2).argmin(axis=1)
    assert np.count_nonzero(near != atom_of) > gr.NG_FULL // 4                                    # atom_of is not the nearest atom
    w, psum = gr.becke_reference(coords, atom_of, vol, R, a)
    assert float(psum.min()) > 1e-6
    ratio = float(np.max(np.abs((_becke_fp64(coords, atom_of, vol, R, a) - w).astype(np.float64)) / vol))
    print(f"[yardstick] becke natm={natm}: FP64 / vol = {ratio:.3g}, min sum P = {float(psum.min()):.3g}")
    assert ratio < 2e-14 / 8
    # the hand-placed points: exact results of the reference
    assert w[gr.BECKE_ON_PARENT] == vol[gr.BECKE_ON_PARENT] and atom_of[gr.BECKE_ON_PARENT] == natm - 1
    assert w[gr.BECKE_ON_OTHER] == 0 and w[gr.BECKE_AXIS] == 0
    assert coords[gr.BECKE_AXIS, 0] < 0 and not coords[gr.BECKE_AXIS, 1:].any()
    d = np.linalg.norm(coords[gr.BECKE_PLANE] - R[:2], axis=1)
    assert d[0] == d[1] and 0 < w[gr.BECKE_PLANE] < vol[gr.BECKE_PLANE]
    far = np.linalg.norm(coords[gr.BECKE_FAR] - R, axis=1).min()
    assert 46.0 < far < 50.0 and w[gr.BECKE_FAR] > 0
    dist = np.linalg.norm(coords[5:] - R[near[5:]], axis=1)
    assert dist.min() > 0.01 and np.sort(dist)[len(dist) // 2] < 3.0


def test_becke_reference_single_atom_and_mirror_pair():
    vol = np.array([0.5, 3.0, 1e-7])
    pts = np.array([[0.0, 0.0, 0.0], [1.0, -2.0, 0.5], [30.0, 0.0, 1.0]])
    w, psum = gr.becke_reference(pts, np.zeros(3, dtype=int), vol, np.zeros((1, 3)), np.zeros((1, 1)))
    assert np.array_equal(w, vol) and np.array_equal(psum, np.ones(3))
    R = np.array([[0.0, 0.0, -0.7], [0.0, 0.0, 0.7]])
    p = np.array([[0.3, -0.2, 0.45], [1.0, 2.0, -3.0]])
    both = np.vstack([p, p * [1, 1, -1]])
    w, _ = gr.becke_reference(both, np.zeros(4, dtype=int), np.ones(4), R, np.zeros((2, 2)))
    assert np.abs((w[:2] + w[2:] - 1).astype(np.float64)).max() < 1e-18


def _oracle_grid_inputs(mol, level):
    """(coords, atom_of, vol) of oracle.dft.build_grids, from the oracle's own radial, angular and pruning rules."""
    from oracle import dft as odft
    cs, own, vols = [], [], []
    for ia, z in enumerate(int(v) for v in mol.atom_charges()):
        n_rad, n_ang = odft._RAD[level][odft._period(z)], odft._ANG[level][odft._period(z)]
        r, dr = odft.treutler_ahlrichs(n_rad, z)
        rw = 4 * np.pi * r * r * dr
        angs = odft.nwchem_prune(z, r, n_ang)
        for n in sorted(set(angs.tolist())):
            x, wl = odft.lebedev(n)
            idx = np.where(angs == n)[0]
            c = np.einsum("i,jk->jik", r[idx], x).reshape(-1, 3) + mol.atom_coords()[ia]
            cs.append(c)
            vols.append(np.einsum("i,j->ji", rw[idx], wl).ravel())
            own.append(np.full(len(c), ia))
    return np.vstack(cs), np.hstack(own), np.hstack(vols)


@pytest.mark.parametrize("name", ["h2o", "h2co"])
def test_becke_reference_agrees_with_oracle_grids(name):
    """oracle.dft.build_grids (each unordered pair once, FP64) against `becke_reference` on the same points: within
    5e-15 vol, a quarter of the GPU bound.  Measured: 2.39e-15 (H2O), 2.07e-15 (H2CO)."""
    from oracle import dft as odft
    mol = _mol(MOLECULES[name], "sto-3g")
    coords, atom_of, vol = _oracle_grid_inputs(mol, 1)
    c, w = odft.build_grids(mol, 1)
    assert np.array_equal(c, coords)
    zs = mol.atom_charges()
    rad = np.sqrt(np.array([odft._BRAGG[int(z)] / odft.BOHR for z in zs]))
    rr = rad[:, None] / rad[None, :]
    a = np.clip(0.25 * (rr.T - rr), -0.5, 0.5)
    ref, psum = gr.becke_reference(coords, atom_of, vol, mol.atom_coords(), a)
    ratio = float(np.max(np.abs((w - ref).astype(np.float64)) / np.abs(vol)))
    print(f"[yardstick] becke {name}: oracle grids / vol = {ratio:.3g}")
    assert ratio < 5e-15 and float(psum.min()) > 1e-6


def test_density_references_agree_with_the_density_matrix_formula():
    rng = np.random.default_rng(5)
    nao, ng, rank = 7, 33, 3
    ao = rng.standard_normal((4, nao, ng))
    Z = rng.standard_normal((nao, rank))
    D = Z @ Z.T
    val, maj = gr.rho_reference(ao, Z)
    rho = np.einsum("mg,mn,ng->g", ao[0], D, ao[0])
    grad = 2 * np.einsum("kmg,mn,ng->kg", ao[1:], D, ao[0])
    tau = 0.5 * np.einsum("kmg,mn,kng->g", ao[1:], D, ao[1:])
    assert np.abs((val["rho"][0] - rho).astype(np.float64)).max() < 1e-12
    assert np.abs((val["rho"][1:] - grad).astype(np.float64)).max() < 1e-12
    assert np.abs((val["tau"] - tau).astype(np.float64)).max() < 1e-12
    assert np.all(maj["rho"] >= np.abs(val["rho"])) and np.all(maj["tau"] >= val["tau"])
    v2, m2 = gr.rho_mo_reference(np.einsum("mi,cmg->cig", Z, ao))
    assert np.abs((v2["rho"] - val["rho"]).astype(np.float64)).max() < 1e-12 and np.all(m2["rho"] <= maj["rho"] * (1 + 1e-15))
    r, m = gr.rho_c_reference(ao, D @ ao[0])
    assert np.abs((r - val["rho"]).astype(np.float64)).max() < 1e-12 and np.all(m >= np.abs(r))
    v0, m0 = gr.rho_reference(ao[:1], Z)
    assert v0["tau"] is None and v0["rho"].shape == (1, ng) and np.array_equal(v0["rho"][0], val["rho"][0])


def test_cholesky_solve_reference_matches_numpy_and_lapack_info():
    rng = np.random.default_rng(9)
    for nocc, n in ((1, 1), (2, 63), (63, 64), (64, 65)):
        A = rng.standard_normal((n + nocc, nocc))
        M, W = A.T @ A, rng.standard_normal((n, nocc))
        Zt, info = gr.cholesky_solve_reference(M, W)
        ref = np.linalg.solve(np.linalg.cholesky(M), W.T)
        assert info == 0 and np.abs((Zt - ref).astype(np.float64)).max() < 1e-10 * (1 + np.abs(ref).max())
    for k in (0, 20, nocc - 1):
        Mb = M.copy()
        Mb[k, k] = -1.0 if k else 0.0
        assert gr.cholesky_solve_reference(Mb, W) == (None, k + 1)
    Mb = M.copy()
    Mb[5, 5] = np.nan
    assert gr.cholesky_solve_reference(Mb, W) == (None, 6)
