"""C-PCM host pieces without a GPU (mi355scf/pcm.py): the solvent template's import surface, the switched cavity, the
conductor-limit anchors of the discretised model, the host derivatives of the gradient, and the wrapper's surface."""
import importlib
import json
import math
import os

import numpy as np
import pytest
import torch

from mi355scf import pcm

HERE = os.path.dirname(os.path.abspath(__file__))


def _resolve(dotted):
    parts = dotted.split(".")
    for cut in range(len(parts), 0, -1):
        try:
            obj = importlib.import_module(".".join(parts[:cut]))
        except ImportError:
            continue
        for p in parts[cut:]:
            obj = getattr(obj, p)
        return obj
    raise ImportError(dotted)


def test_solvent_template_surface_resolves():
    """Every import and dotted chain of calculate_solvent_effect.py (names in tests/golden/template_surface_solvent.json)."""
    with open(os.path.join(HERE, "golden", "template_surface_solvent.json")) as fh:
        s = json.load(fh)
    assert s["script"] == "calculate_solvent_effect"
    for mod, sym in s["imports"]:
        _resolve(mod if sym is None else mod + "." + sym)
    for root, attrs in s["chains"]:
        obj = _resolve(root)
        for a in attrs:
            assert hasattr(obj, a), f"{root}.{'.'.join(attrs)}: '{a}' missing"
            obj = getattr(obj, a)
    from pyscf import solvent
    from rdkit import Chem
    from rdkit.Chem import Descriptors
    assert callable(solvent.PCM)
    assert math.isnan(Descriptors.MolLogP(Chem.MolFromSmiles("CC(=O)O")))


# ---- surface --------------------------------------------------------------------------------------------------------------
def test_isolated_atom_keeps_every_point():
    R = 2.5
    s = pcm.Surface(np.zeros((1, 3)), [R], 302)
    assert s.npts == 302
    assert np.all(s.swf == 1.0)
    assert abs(s.area.sum() - 4 * np.pi * R * R) < 1e-10
    assert np.allclose(np.linalg.norm(s.coords, axis=1), R)
    assert s.blocks[:, 1].sum() == 302 and s.blocks[:, 1].max() <= 64 and np.all(s.blocks[:, 2] == 0)
    assert abs(s.zeta[0] - pcm.XI[302] / (R * np.sqrt(s.weight[0]))) < 1e-14


def test_overlapping_spheres_switch_smoothly():
    """Two spheres: buried points are dropped, swf stays in [0, 1], and the area falls continuously as they approach."""
    R = np.array([2.6, 2.2])
    areas = []
    for d in np.linspace(6.0, 2.0, 41):
        s = pcm.Surface(np.array([[0, 0, 0], [0, 0, d]], dtype=float), R, 302)
        assert np.all((s.swf > 0) & (s.swf <= 1.0))
        areas.append(s.area.sum())
    areas = np.array(areas)
    assert areas[0] == pytest.approx(4 * np.pi * (R ** 2).sum(), rel=1e-12)   # apart: nothing switched
    assert np.all(np.diff(areas) <= 1e-9)                                       # shrinking monotonically
    assert np.max(np.abs(np.diff(areas))) < 0.05 * areas[0]                    # no jumps between 0.1 Bohr steps
    s = pcm.Surface(np.array([[0, 0, 0], [0, 0, 3.0]]), R, 302)
    assert 0 < s.npts < 604 and np.any(s.swf < 0.999)


def test_area_is_continuous_under_small_displacements():
    X = np.array([[0.0, 0.0, 0.0], [0.0, 1.43, 1.11], [0.0, -1.43, 1.11]])
    R = np.array([1.52, 1.10, 1.10]) * 1.2 / 0.52917721092
    a0 = pcm.Surface(X, R, 302).area.sum()
    for ia in range(3):
        for x in range(3):
            da = []
            for h in (1e-4, 5e-5):
                Xp = X.copy()
                Xp[ia, x] += h
                da.append(pcm.Surface(Xp, R, 302).area.sum() - a0)
            # O(h) changes (no point appears or vanishes with a finite area): bounded slope, halving h halves the change
            assert abs(da[0]) < 100.0 * 1e-4, (ia, x, da)
            assert abs(da[0] - 2.0 * da[1]) < 0.05 * abs(da[0]) + 100.0 * 1e-8, (ia, x, da)   # + the O(h^2) part


# ---- conductor-limit anchors ------------------------------------------------------------------------------------------------
def _energy(s, v, f):
    S = pcm.s_matrix(s.coords, s.zeta, s.swf).numpy()
    q = -f * np.linalg.solve(S, v)
    return 0.5 * q @ v, q


def _anchors(ngrid, R=3.0):
    s = pcm.Surface(np.zeros((1, 3)), [R], ngrid)
    vq = pcm.v_nuc(s.coords, s.zeta, np.zeros((1, 3)), [1.0]).numpy()
    mu = np.array([0.3, -0.2, 0.5])
    vd = s.coords @ mu / np.linalg.norm(s.coords, axis=1) ** 3
    return s, vq, vd, mu, R


def test_conductor_limit_charge_and_dipole():
    """eps = inf: a unit charge at the centre of one sphere gives -1/(2R), a point dipole -mu^2/(2R^3).  The discretised
    Gaussian-charge model approaches both as the Lebedev grid is refined (194 -> 302 -> 590); the tolerance at 302 points is
    the 194-to-590 spread, which bounds the discretisation error at the default grid."""
    out = {}
    for n in (194, 302, 590):
        s, vq, vd, mu, R = _anchors(n)
        eq, q = _energy(s, vq, 1.0)
        ed, _ = _energy(s, vd, 1.0)
        out[n] = (eq, ed, q.sum())
    ref_q, ref_d = -1.0 / (2 * R), -(mu @ mu) / (2 * R ** 3)
    tol_q = abs(out[194][0] - out[590][0]) + 1e-3 * abs(ref_q)
    tol_d = abs(out[194][1] - out[590][1]) + 1e-3 * abs(ref_d)
    assert abs(out[302][0] - ref_q) < tol_q + 5e-3 * abs(ref_q), (out, ref_q)
    assert abs(out[302][1] - ref_d) < tol_d + 5e-3 * abs(ref_d), (out, ref_d)
    assert abs(out[302][2] + 1.0) < 5e-3          # Gauss's law in the conductor limit: the surface holds -Q


@pytest.mark.parametrize("method", ["C-PCM", "COSMO"])
@pytest.mark.parametrize("eps", [2.27, 78.39])
def test_finite_eps_scales_by_f(method, eps):
    s, vq, vd, _mu, _R = _anchors(302)
    f = pcm.scaling_factor(eps, method)
    expect = (eps - 1) / eps if method == "C-PCM" else (eps - 1) / (eps + 0.5)
    assert f == pytest.approx(expect, rel=1e-15)
    for v in (vq, vd):
        e_inf, _ = _energy(s, v, 1.0)
        e, _ = _energy(s, v, f)
        assert e == pytest.approx(f * e_inf, rel=1e-13)
    assert pcm.scaling_factor(float("inf"), method) == 1.0 and pcm.scaling_factor(1.0, method) == 0.0


# ---- host derivatives -------------------------------------------------------------------------------------------------------
def _mol_surface(X):
    R = np.array([1.52, 1.10, 1.10]) * 1.2 / 0.52917721092
    return pcm.Surface(X, R, 110)


def test_host_gradient_terms_match_central_differences():
    """d/dR [1/2 q^T S q] (fixed q, points rigid with their owners, swf through the diagonal) and d/dR [q^T v_n]."""
    X = np.array([[0.0, 0.0, 0.0], [0.0, 1.43, 1.11], [0.0, -1.43, 1.11]])
    Z = [8.0, 1.0, 1.0]
    s0 = _mol_surface(X)
    rng = np.random.default_rng(7)
    q = rng.normal(size=s0.npts) * 0.01
    gS = pcm.grad_s(s0, q)
    gV = pcm.grad_vnuc(s0, Z, q)
    h = 1e-5
    for ia in range(3):
        for x in range(3):
            vals = []
            for sgn in (1, -1):
                Xd = X.copy()
                Xd[ia, x] += sgn * h
                s = _mol_surface(Xd)
                assert s.npts == s0.npts
                S = pcm.s_matrix(s.coords, s.zeta, s.swf).numpy()
                vn = pcm.v_nuc(s.coords, s.zeta, Xd, Z).numpy()
                vals.append((0.5 * q @ S @ q, q @ vn))
            dS = (vals[0][0] - vals[1][0]) / (2 * h)
            dV = (vals[0][1] - vals[1][1]) / (2 * h)
            assert abs(gS[ia, x] - dS) < 1e-5 * max(1.0, abs(dS)), (ia, x, gS[ia, x], dS)   # O(h^2) + rounding of 1/swf^2 terms
            assert abs(gV[ia, x] - dV) < 1e-6 * max(1.0, abs(dV)), (ia, x, gV[ia, x], dV)
    assert np.abs(gS.sum(axis=0)).max() < 1e-9


# ---- wrapper surface --------------------------------------------------------------------------------------------------------
def _water():
    from pyscf import gto
    mol = gto.Mole()
    mol.atom = "O 0 0 0; H 0 -0.757 0.587; H 0 0.757 0.587"
    mol.basis = "6-31G*"
    mol.verbose = 0
    mol.build()
    return mol


def test_defaults_and_eps_forwarding():
    from pyscf import dft, scf, solvent
    mf = solvent.PCM(scf.RHF(_water()))
    ws = mf.with_solvent
    assert (ws.method, ws.eps, ws.lebedev_order, ws.vdw_scale, ws.r_probe) == ("C-PCM", 78.3553, 29, 1.2, 0.0)
    assert ws.ngrid == 302 and ws.radii_table is None and ws.atom_radii is None and ws.e is None
    assert isinstance(mf, scf.RHF) and type(mf).__name__ == "PCMRHF"
    mf.eps = 4.89
    assert ws.eps == 4.89 and mf.eps == 4.89
    mf.method = "COSMO"
    assert ws.method == "COSMO" and ws.f == pytest.approx(3.89 / 5.39)
    assert mf.to_gpu() is mf and solvent.PCM(mf) is mf
    mk = dft.RKS(_water())
    mk.xc = "B3LYP"
    pk = mk.PCM()
    assert isinstance(pk, dft.RKS) and pk.xc == "B3LYP" and pk.with_solvent.eps == 78.3553
    r = pcm.atom_radii_bohr(_water())
    assert r == pytest.approx(np.array([1.52, 1.10, 1.10]) * 1.2 / 0.52917721092)
    r = pcm.atom_radii_bohr(_water(), atom_radii={"O": 1.6})
    assert r[0] == pytest.approx(1.6 * 1.2 / 0.52917721092)
    r = pcm.atom_radii_bohr(_water(), radii_table={8: 3.0, 1: 2.0})
    assert list(r) == [3.0, 2.0, 2.0]


def test_refused_cases_raise():
    from pyscf import dft, gto, scf, solvent
    mf = solvent.PCM(scf.RHF(_water()))
    for m in ("IEF-PCM", "SS(V)PE", "SMD"):
        mf.method = m
        with pytest.raises(NotImplementedError):
            mf.with_solvent.build(None, mf.mol)
    with pytest.raises(NotImplementedError):
        solvent.PCM(scf.RHF(_water()), method="SMD")
    mol = gto.Mole()
    mol.atom = "O 0 0 0; H 0 0 0.97"
    mol.basis, mol.spin, mol.verbose = "6-31G*", 1, 0
    mol.build()
    for mfu in (scf.UHF(mol), dft.UKS(mol)):
        with pytest.raises(NotImplementedError):
            solvent.PCM(mfu)
    mf = solvent.PCM(scf.RHF(_water()))
    for name in ("TDA", "TDHF", "TDDFT"):
        with pytest.raises(NotImplementedError):
            getattr(mf, name)()
    with pytest.raises(NotImplementedError):
        mf.shard(0, 2)
    two = scf.RHF(_water())
    two._nranks = 2
    with pytest.raises(NotImplementedError):
        solvent.PCM(two)
    from pyscf import tdscf
    with pytest.raises(NotImplementedError):
        tdscf.TDA(mf)
