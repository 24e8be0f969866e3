"""Grid-weight response of the Kohn-Sham gradients (`Gradients.grid_response = True`): the kernel `mi_grid_becke_grad` against the
complex-step reference of test_grid_response_host.py, the XC term at fixed density and the total gradient against differences
of the energy they are supposed to be the derivative of, translational invariance, the Hessian, `optimize`, two ranks.

Every comparison with the response switched on has its twin with the response off asserting that the twin MISSES: the flag
has to be what makes the difference."""
import functools
import os
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from conftest import ROOT, MOLECULES, free_port
from test_grid_response_host import (adjust_matrix, atom_grids, becke_grad_reference, becke_weight_jacobian, make_mol,
                                     richardson)

pytestmark = pytest.mark.gpu
BOHR = 0.52917721092


# ---------------------------------------------------------------------------------------------
# the kernel against the complex-step reference
# ---------------------------------------------------------------------------------------------
def _chain_atoms(n=130):
    """n hydrogens 1.4 Bohr apart along a gentle helix (no three centres collinear)."""
    k = np.arange(n)
    xyz = np.stack([0.3 * np.cos(0.7 * k), 0.3 * np.sin(0.7 * k), 1.4 * k], axis=1) * BOHR
    return "; ".join(f"H {x:.10f} {y:.10f} {z:.10f}" for x, y, z in xyz)


def _ibuprofen_atoms():
    from mi355scf.smiles_fixtures import _ibuprofen
    sym, xyz = _ibuprofen()
    return "; ".join(f"{s} {x:.10f} {y:.10f} {z:.10f}" for s, (x, y, z) in zip(sym, np.asarray(xyz)))


GEOMETRIES = {
    "he": lambda: "He 0 0 0",
    "hf": lambda: MOLECULES["hf"],
    "h2o": lambda: MOLECULES["h2o"],
    "ch4": lambda: MOLECULES["ch4"],
    "h2o_ghost": lambda: MOLECULES["h2o"] + "; Ghost:O 0 0 2.9",
    "ibuprofen": _ibuprofen_atoms,
    "chain": _chain_atoms,
}
# (geometry, points): ng = 1, 255, 256, 257 and 1000 cross one lane, one wave short of a workgroup, a full one, one lane into the
# next and several; "per atom" cases take that many points of every atom
KERNEL_CASES = [("he", 64), ("hf", 257), ("h2o", 1), ("h2o", 255), ("h2o", 256), ("h2o", 257), ("h2o", 1000), ("ch4", 1000),
                ("h2o_ghost", 257), ("ibuprofen", "8 per atom"), ("chain", "4 per atom")]


@functools.lru_cache(maxsize=None)
def _kernel_case(name, npts):
    """(mol, R, a, s, vol, own, dW) of a seeded choice of points of the level-0 grid: computed once, shared by the tests."""
    mol = make_mol(GEOMETRIES[name]())
    s, vol, own, _a = atom_grids(mol, 0)
    rng = np.random.default_rng(11)
    if isinstance(npts, str):
        per = int(npts.split()[0])
        pick = np.concatenate([rng.choice(np.where(own == ia)[0], per, replace=False) for ia in range(mol.natm)])
    else:
        pick = rng.choice(len(s), npts, replace=False)
    pick.sort()
    s, vol, own = s[pick], vol[pick], own[pick]
    R = mol.atom_coords()
    a = adjust_matrix(mol.atom_charges())
    return mol, R, a, s, vol, own, becke_weight_jacobian(s, own, R, a)


def _device_grad(eng, R, a, s, vol, own, e, out=None):
    dev = eng.device
    t = lambda x, dt=torch.float64: torch.as_tensor(np.ascontiguousarray(x), dtype=dt, device=dev)
    g = eng.becke_weights_grad(t(R[own] + s), t(own, torch.int32), t(vol), t(a), t(e), out=out)
    torch.cuda.synchronize()
    return g.cpu().numpy()


RESOLVED = 1e-3


def _energy_vectors(dW):
    """Seeded noise in [-1, 1] (three seeds) and one-hot vectors on a handful of points (they catch a contribution booked to the
    wrong lane, parent or atom, which a sum over points can hide).

    The one-hot points are spread over those whose partition is RESOLVED, max |dW_g| >= 1e-3 / Bohr.  Reason: the weights
    kernel, the kernel under test and the reference all form a cell factor as s = (1 - f3) / 2, which carries an ABSOLUTE
    rounding error of 1e-16 however small s is, and the reference divides by interatomic distances where the kernels multiply
    by a reciprocal square root, so two correct evaluations differ by one unit of rounding in s.  Through d ln P ~ 1e2 that
    is 1e-14 / Bohr in dW_g whatever its size: a bound of 1e-10 RELATIVE to a single point's derivative can be met only where
    that derivative is above 1e-4.  Deep inside a cell (all s of the parent saturated) dW_g is 1e-20 and below, made of nothing
    but that rounding; such points are covered by the seeded vectors, where they weigh what they weigh in a gradient."""
    ng = dW.shape[0]
    for seed in (0, 1, 2):
        yield f"seed {seed}", np.random.default_rng(seed).uniform(-1.0, 1.0, ng)
    resolved = np.where(np.abs(dW).reshape(ng, -1).max(axis=1) >= RESOLVED)[0]
    for g in sorted(set(resolved[np.linspace(0, len(resolved) - 1, 5).astype(int)].tolist())) if len(resolved) else []:
        e = np.zeros(ng)
        e[g] = 1.0
        yield f"one-hot {g}", e


@pytest.mark.parametrize("name,npts", KERNEL_CASES)
def test_kernel_matches_complex_step(name, npts):
    """|kernel - reference| <= 1e-10 max|reference component| (the weights themselves hold 1e-12, `test_becke_grid_matches_oracle`;
    two orders for the division by the interatomic distances and the sum over points), and sum_C out_C <= 1e-12 max|out|."""
    from mi355scf.engine import Engine
    mol, R, a, s, vol, own, dW = _kernel_case(name, npts)
    eng = Engine(mol)
    worst = 0.0
    for label, e in _energy_vectors(dW):
        ref = becke_grad_reference(s, own, R, a, vol, e, dW)
        got = _device_grad(eng, R, a, s, vol, own, e)
        assert np.isfinite(got).all()
        if mol.natm == 1:
            assert np.array_equal(got, np.zeros((1, 3))), got     # one atom: no partition, exactly zero
            continue
        scale = np.abs(ref).max()
        err, tsum = np.abs(got - ref).max() / scale, np.abs(got.sum(axis=0)).max() / np.abs(got).max()
        worst = max(worst, err)
        print(f"{name} {npts} {label}: max |ref| {scale:.3e}, relative error {err:.2e}, sum over atoms {tsum:.2e}")
        assert err <= 1e-10, (label, err)
        assert tsum <= 1e-12, (label, tsum)
    print(f"{name} {npts}: worst relative error {worst:.2e}")


def test_kernel_accumulates_and_is_reproducible():
    """out += : a second call on the same buffer doubles it; two fresh calls agree to the bit (fixed-order reduction)."""
    from mi355scf.engine import Engine
    mol, R, a, s, vol, own, _dW = _kernel_case("ch4", 1000)
    eng = Engine(mol)
    e = np.random.default_rng(5).uniform(-1.0, 1.0, len(vol))
    g1 = _device_grad(eng, R, a, s, vol, own, e)
    g2 = _device_grad(eng, R, a, s, vol, own, e)
    assert np.array_equal(g1, g2)
    buf = torch.as_tensor(g1, device=eng.device).clone()
    assert np.array_equal(_device_grad(eng, R, a, s, vol, own, e, out=buf), 2.0 * g1)


def test_kernel_in_chunks_of_points():
    """More points than one pass holds cell functions for (2^25 doubles / 130 atoms = 258 048 points): the chain's 520 points
    600 times over are two passes, and the answer is 600 times the reference."""
    from mi355scf.engine import Engine
    mol, R, a, s, vol, own, dW = _kernel_case("chain", "4 per atom")
    e = np.random.default_rng(0).uniform(-1.0, 1.0, len(vol))
    ref = 600.0 * becke_grad_reference(s, own, R, a, vol, e, dW)
    rep = lambda x: np.concatenate([x] * 600)
    got = _device_grad(Engine(mol), R, a, rep(s), rep(vol), rep(own), rep(e))
    err = np.abs(got - ref).max() / np.abs(ref).max()
    print(f"{600 * len(vol)} points of the chain: relative error {err:.2e}")
    assert err <= 1e-10


def test_kernel_point_on_a_foreign_nucleus_stays_finite():
    from mi355scf.engine import Engine
    mol, R, a, s, vol, own, _dW = _kernel_case("h2o", 257)
    s = s.copy()
    g = int(np.where(own == 0)[0][0])
    s[g] = R[1] - R[0]                       # a point of the oxygen exactly on a hydrogen
    e = np.zeros(len(vol))
    e[g] = 1.0
    eng = Engine(mol)
    for ev in (e, np.ones(len(vol))):
        got = _device_grad(eng, R, a, s, vol, own, ev)
        assert np.isfinite(got).all(), got
        assert np.abs(got.sum(axis=0)).max() <= 1e-12 * max(np.abs(got).max(), 1e-300)


def test_kernel_guards():
    """Null arguments, more atoms than the kernel's LDS table, ng == 0 (no-op), ng < 0 ("negative")."""
    from mi355scf.engine import Engine, EngineError, _check, lib
    from test_gpu_dense_kernels import assert_guard, guarded
    mol, R, a, s, vol, own, _dW = _kernel_case("h2o", 257)
    eng = Engine(mol)
    dev = eng.device
    t = lambda x, dt=torch.float64: torch.as_tensor(np.ascontiguousarray(x), dtype=dt, device=dev)
    args = [t(R[own] + s), t(own, torch.int32), t(vol), t(np.ones(len(vol)))]
    adj = t(a)
    out = guarded(9)
    call = lambda ng, ptrs, o: lib().mi_grid_becke_grad(eng._h, ptrs[0], ptrs[1], ptrs[2], ptrs[3], ng, ptrs[4], o, eng._stream())
    ptrs = [x.data_ptr() for x in args] + [adj.data_ptr()]
    same = lambda: torch.equal(out.view(torch.int64), sentinel.view(torch.int64))
    sentinel = out.clone()
    assert call(0, ptrs, out.data_ptr()) == 0
    torch.cuda.synchronize()
    assert same()                                          # ng == 0: nothing launched, nothing written
    with pytest.raises(EngineError, match="negative"):
        _check(call(-1, ptrs, out.data_ptr()))
    for k in range(5):
        with pytest.raises(EngineError, match="null"):
            _check(call(len(vol), ptrs[:k] + [None] + ptrs[k + 1:], out.data_ptr()))
    with pytest.raises(EngineError, match="null"):
        _check(call(len(vol), ptrs, None))
    with pytest.raises(EngineError, match="null"):
        _check(lib().mi_grid_becke_grad(None, *ptrs[:4], len(vol), ptrs[4], out.data_ptr(), eng._stream()))
    torch.cuda.synchronize()
    assert same()
    assert_guard(out, 9, "refused calls")
    full = guarded(9, np.zeros(9))
    assert call(len(vol), ptrs, full.data_ptr()) == 0      # natm * 3 doubles and not one more
    torch.cuda.synchronize()
    assert_guard(full, 9, "a full call") 
    assert np.abs(full[:9].cpu().numpy()).max() > 0
    big = make_mol("; ".join(f"H 0 0 {0.8 * k:.1f}" for k in range(1026)))
    with pytest.raises(EngineError, match="too many atoms"):
        _check(lib().mi_grid_becke_grad(Engine(big)._h, *ptrs[:4], len(vol), ptrs[4], out.data_ptr(), eng._stream()))


# ---------------------------------------------------------------------------------------------
# the XC term at fixed density against differences of the oracle's E_xc (grid rebuilt at every geometry)
# ---------------------------------------------------------------------------------------------
def _ks(mol, xc, cls="RKS", conv_tol=1e-10):
    from pyscf import dft
    mf = getattr(dft, cls)(mol)
    mf.xc = xc
    mf.grids.level = 1
    mf.small_rho_cutoff = 0
    mf.conv_tol = conv_tol
    return mf


OH = "O 0 0 0; H 0 0 0.97"


@pytest.mark.parametrize("xc,cls", [("LDA,VWN", "RKS"), ("PBE", "RKS"), ("TPSS", "RKS"), ("B3LYP", "UKS")])
def test_xc_term_is_the_derivative_of_the_quadrature(xc, cls):
    """`grad_xc` / `grad_xc_spin` of the converged density (level 1, no density pruning) with the response: 1e-7 from Richardson
    differences (1e-3, 2e-3 Bohr) of the oracle's E_xc at that density.  Without the response the same comparison misses by more
    than 1e-5."""
    from oracle import dft as odft
    mol = make_mol(MOLECULES["h2o"], "6-31G(d)") if cls == "RKS" else make_mol(OH, "6-31G(d)", spin=1)
    mf = _ks(mol, xc, cls)
    mf.kernel()
    assert mf.converged
    dm = mf._dm
    dm_host = (dm if cls == "RKS" else torch.stack([dm[0], dm[1]])).cpu().numpy()
    nr = {"RKS": odft.nr_rks_mgga if xc == "TPSS" else odft.nr_rks, "UKS": odft.nr_uks}[cls]

    def exc(Rd):
        m = mol.set_geom_(Rd, unit="Bohr", inplace=False)
        return nr(m, *odft.build_grids(m, 1), xc, dm_host)[1]
    ref = richardson(exc, mol.atom_coords())
    g = mf.nuc_grad_method()
    term = (lambda: g.grad_xc(dm)) if cls == "RKS" else (lambda: g.grad_xc_spin(dm))
    off = term()
    g.grid_response = True
    on = term()
    err_on, err_off = np.abs(on - ref).max(), np.abs(off - ref).max()
    print(f"{cls} {xc}: with response {err_on:.2e}, without {err_off:.2e}, sum over atoms {np.abs(on.sum(axis=0)).max():.1e} / "
          f"{np.abs(off.sum(axis=0)).max():.1e}")
    assert err_on <= 1e-7
    assert err_off > 1e-5


# ---------------------------------------------------------------------------------------------
# the total gradient against central differences of the SCF energy
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,coords", [("h2o", [(0, 2), (1, 1), (1, 2)]), ("h2co", [(0, 0), (1, 0), (2, 1)])])
def test_gradient_with_response_is_the_derivative_of_the_scf_energy(name, coords):
    """B3LYP/6-31G(d), level 1, no density pruning, conv_tol 1e-11: 1e-6 (the bar of RHF against energy differences) on three
    coordinates (for water the three that symmetry neither fixes at zero nor repeats), central differences at 1e-3 and 2e-3 Bohr
    extrapolated; without the response the same comparison -- the largest deviation over the same coordinates -- misses by more
    than 1e-5."""
    mol = make_mol(MOLECULES[name], "6-31G(d)")

    def scf_at(m, dm0=None):
        mf = _ks(m, "B3LYP", conv_tol=1e-11)
        mf.conv_tol_grad = 1e-8
        e = mf.kernel(dm0=dm0)
        assert mf.converged
        return mf, e
    mf, _e = scf_at(mol)
    dm0 = mf.make_rdm1()
    g = mf.nuc_grad_method()
    off = g.kernel().copy()
    g.grid_response = True
    on = g.kernel().copy()
    R = mol.atom_coords()
    worst_on, worst_off = 0.0, 0.0
    for ia, x in coords:
        d = []
        for h in (1e-3, 2e-3):
            Rp, Rm = R.copy(), R.copy()
            Rp[ia, x] += h
            Rm[ia, x] -= h
            d.append((scf_at(mol.set_geom_(Rp, unit="Bohr", inplace=False), dm0)[1]
                      - scf_at(mol.set_geom_(Rm, unit="Bohr", inplace=False), dm0)[1]) / (2 * h))
        fd = (4.0 * d[0] - d[1]) / 3.0
        print(f"{name} dE/dR[{ia}, {x}]: differences {fd:.9f}, with response {on[ia, x]:.9f} ({on[ia, x] - fd:.2e}), "
              f"without {off[ia, x]:.9f} ({off[ia, x] - fd:.2e})")
        worst_on, worst_off = max(worst_on, abs(on[ia, x] - fd)), max(worst_off, abs(off[ia, x] - fd))
    assert worst_on <= 1e-6
    assert worst_off > 1e-5


# ---------------------------------------------------------------------------------------------
# translational invariance
# ---------------------------------------------------------------------------------------------
def _translation_case(kind):
    """(Kohn-Sham object, its Hartree-Fock counterpart: same molecule, basis, spin treatment, fitting and solvent)."""
    from pyscf import dft, scf, solvent
    if kind in ("UKS", "ROKS"):
        mol = make_mol(OH, "6-31G(d)", spin=1)
        ks = _ks(mol, "PBE" if kind == "UKS" else "B3LYP", kind)
        hf = (scf.UHF if kind == "UKS" else scf.ROHF)(mol)
    else:
        mol = make_mol(MOLECULES["h2o"], "6-31G(d)")
        ks, hf = _ks(mol, "B3LYP"), scf.RHF(mol)
        if kind == "DF":
            ks, hf = ks.density_fit(), hf.density_fit()
        if kind == "PCM":
            ks, hf = solvent.PCM(ks), solvent.PCM(hf)
    hf.conv_tol = ks.conv_tol = 1e-11
    return ks, hf


@pytest.mark.parametrize("kind", ["RKS", "UKS", "ROKS", "DF", "PCM"])
def test_forces_sum_to_zero_with_response(kind):
    """|sum_A de_A| with the response is what the Hartree-Fock gradient of the same molecule, basis, spin treatment, fitting and
    solvent leaves (twice that, or 1e-8); without it, more than 1e-6 at level 1."""
    ks, hf = _translation_case(kind)
    hf.kernel()
    ks.kernel()
    assert hf.converged and ks.converged
    floor = np.abs(hf.nuc_grad_method().kernel().sum(axis=0)).max()
    g = ks.nuc_grad_method()
    assert g.grid_response is False
    off = np.abs(g.kernel().sum(axis=0)).max()
    g.grid_response = True
    on = np.abs(g.kernel().sum(axis=0)).max()
    print(f"{kind}: |sum of forces| Hartree-Fock {floor:.2e}, with response {on:.2e}, without {off:.2e}")
    assert on <= max(1e-8, 2.0 * floor)
    assert off > 1e-6


def test_default_is_unchanged():
    """A fresh gradient object has the response off, and setting it to False explicitly changes nothing: the XC term -- all the
    flag reaches -- is equal to the bit.  The whole `de` is compared to 1e-13 only: two runs of one default object already
    differ by 4e-16 in components that symmetry makes zero (the two-electron kernel sums with FP64 atomics; with the flag
    off every statement that runs is the one that ran before the flag existed), so `np.array_equal` of two `de` holds for no
    pair of objects."""
    mol = make_mol(MOLECULES["h2o"], "6-31G(d)")
    mf = _ks(mol, "B3LYP")
    mf.kernel()
    g1 = mf.nuc_grad_method()
    assert g1.grid_response is False and type(g1).grid_response is False
    g2 = mf.nuc_grad_method()
    g2.grid_response = False
    assert np.array_equal(g1.grad_xc(mf._dm), g2.grad_xc(mf._dm))
    de1, de2 = g1.kernel(), g2.kernel()
    assert np.abs(de1 - de2).max() <= 1e-13
    assert g1.as_scanner().g.grid_response is False
    g2.grid_response = True
    assert g2.as_scanner().g.grid_response is True       # the scanner carries the setting of its gradient object
    assert not np.array_equal(g2.kernel(), de1)


def test_pruned_grid_keeps_its_volume_elements_and_parents():
    """Density-based pruning (RKS default) drops `vol` and the parent index with the points; the response is that of the kept
    set, so the forces still sum to zero."""
    mol = make_mol(MOLECULES["h2o"], "6-31G(d)")
    mf = _ks(mol, "B3LYP")
    mf.small_rho_cutoff = 1e-7
    mf.kernel()
    gr = mf.grids
    ng = gr.weights.numel()
    assert gr.vol.numel() == ng and gr.atom_of_dev.numel() == ng and len(gr.atom_of) == ng and gr.coords.shape[0] == ng
    assert ng < len(atom_grids(mol, 1)[1])
    assert np.array_equal(gr.atom_of_dev.cpu().numpy(), gr.atom_of)
    g = mf.nuc_grad_method()
    g.grid_response = True
    assert np.abs(g.kernel().sum(axis=0)).max() <= 1e-8


# ---------------------------------------------------------------------------------------------
# Hessian, optimize
# ---------------------------------------------------------------------------------------------
def test_hessian_of_consistent_gradients_is_symmetric_and_obeys_the_sum_rule():
    """H2O, B3LYP/STO-3G, level 1: the differenced gradients with the response give a raw (unsymmetrised) Hessian as symmetric
    and as translationally invariant as the RHF one of the same molecule (within a factor two); without the response both
    figures are at least ten times larger.

    The sum rule has a floor of 1e-10 Ha/Bohr^2 under the factor two.  With the response the forces sum to zero to ROUNDING, as
    the RHF ones do (measured here: 3e-15 to 8e-15 Ha/Bohr either way, different from run to run because the two-electron kernel
    sums with FP64 atomics), and the figure is the difference of two such residues over 2 * 5e-3 Bohr: 6e-13 to 2e-12 for RHF and
    for B3LYP alike, in no fixed order -- one run gave 7.33e-13 / 7.34e-13, the next 6.2e-13 / 1.7e-12.  A ratio of two rounding
    residues decides nothing; 1e-10 stands for a residue of 1e-12 Ha/Bohr, a hundred times what FP64 leaves and seven orders
    below the 1.6e-3 the sum rule shows without the response."""
    from pyscf import hessian, scf
    mol = make_mol(MOLECULES["h2o"], "sto-3g")

    def figures(mf, response):
        mf.conv_tol = 1e-12
        mf.kernel()
        h = hessian.RKS(mf) if hasattr(mf, "xc") else hessian.RHF(mf)
        assert h.grid_response is False
        h.grid_response = response
        h.kernel()
        raw = h.hess_raw
        n = mol.natm
        return np.abs(raw - raw.T).max(), np.abs(raw.reshape(n, 3, n, 3).sum(axis=2)).max()
    asym_hf, sum_hf = figures(scf.RHF(mol), False)
    asym_on, sum_on = figures(_ks(mol, "B3LYP"), True)
    asym_off, sum_off = figures(_ks(mol, "B3LYP"), False)
    print(f"max |H - H^T|: RHF {asym_hf:.2e}, with response {asym_on:.2e}, without {asym_off:.2e}; "
          f"max |sum_j H_ij|: RHF {sum_hf:.2e}, with response {sum_on:.2e}, without {sum_off:.2e}")
    assert asym_on <= 2.0 * asym_hf and sum_on <= max(2.0 * sum_hf, 1e-10)
    assert asym_off >= 10.0 * asym_on and sum_off >= 10.0 * sum_on


def test_infrared_forwards_the_flag():
    from mi355scf import hessian as hmod
    from pyscf.prop import infrared
    mol = make_mol(MOLECULES["h2o"], "sto-3g")
    mf = _ks(mol, "B3LYP")
    ir = infrared.rks.Infrared(mf)
    assert ir.grid_response is False
    ir.grid_response = True
    seen = []
    orig = hmod.Hessian.kernel

    def spy(self, *a, **k):
        seen.append(self.grid_response)
        return orig(self, *a, **k)
    hmod.Hessian.kernel = spy
    try:
        ir.kernel()
    finally:
        hmod.Hessian.kernel = orig
    assert seen == [True]


def test_optimize_takes_grid_response():
    from pyscf.geomopt.geometric_solver import optimize
    mol = make_mol("O 0 0 0; H 0 -0.80 0.55; H 0 0.72 0.62", "sto-3g")
    mf = _ks(mol, "B3LYP")
    scanners = []
    mol_opt = optimize(mf, grid_response=True, maxsteps=10, callback=lambda env: scanners.append(env["energy_grad"]))
    assert mol_opt._opt_converged, mol_opt._opt_steps
    assert scanners and all(s.g.grid_response is True for s in scanners)
    assert np.abs(scanners[-1].g.de.sum(axis=0)).max() <= 1e-8


# ---------------------------------------------------------------------------------------------
# two ranks
# ---------------------------------------------------------------------------------------------
def _two_rank_scf(mol):
    mf = _ks(mol, "B3LYP", conv_tol=1e-13)
    mf.conv_tol_grad = 1e-9
    return mf


def _worker(rank, world, port, q):
    try:
        sys.path.insert(0, os.path.join(ROOT, "computational-chemistry-ai_amd", "python"))
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
        import torch
        import torch.distributed as dist
        from mi355scf import parallel
        torch.cuda.set_device(0)
        parallel.init("gloo")
        mf = _two_rank_scf(make_mol(MOLECULES["h2o"], "6-31G(d)"))
        mf.shard(rank, world)
        mf.kernel()
        out = {}
        for response in (False, True):
            g = mf.nuc_grad_method()
            g.grid_response = response
            parallel.reset_stats()
            out[response] = (g.kernel().tolist(), dict(parallel.STATS))
        q.put((rank, bool(mf.converged), out))
        dist.destroy_process_group()
    except BaseException:
        import traceback
        q.put((rank, "error", traceback.format_exc()))
        raise


def test_two_rank_gradient_with_response_matches_single_rank():
    """Each rank integrates half of the grid; the [natm, 3] response rides behind the per-AO forces in their all-reduce: the
    gradient equals the single-rank one to 1e-10 and the gradient costs no collective more than without the response."""
    mf = _two_rank_scf(make_mol(MOLECULES["h2o"], "6-31G(d)"))
    mf.kernel()
    g = mf.nuc_grad_method()
    g.grid_response = True
    g1 = g.kernel()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted(q.get(timeout=240) for _ in procs)
    for p in procs:
        p.join(60)
        if p.is_alive():
            p.kill()
    assert not any(r[1] == "error" for r in res), [r[2] for r in res if r[1] == "error"]
    for _rank, converged, out in res:
        assert converged
        err = np.abs(np.array(out[True][0]) - g1).max()
        print(f"two ranks - one rank: {err:.2e}; collectives with response {out[True][1]}, without {out[False][1]}")
        assert err <= 1e-10
        assert out[True][1]["all_reduce"] == out[False][1]["all_reduce"] and out[True][1]["broadcast"] == out[False][1]["broadcast"]
        assert np.abs(np.array(out[True][0]) - np.array(out[False][0])).max() > 1e-6
