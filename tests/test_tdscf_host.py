"""Closed-shell linear response on the host: the UV template's import surface, the Davidson solvers of `mi355scf.tdscf` on
synthetic dense A, B (CPU torch) against the full eigenproblem, and the oscillator-strength formula."""
import json
import os

import numpy as np
import pytest
import torch

from mi355scf import tdscf

HERE = os.path.dirname(os.path.abspath(__file__))


def test_uv_template_import_surface():
    import importlib
    with open(os.path.join(HERE, "golden", "template_surface_uv.json")) as fh:
        surf = json.load(fh)
    for mod, sym in surf["imports"]:
        m = importlib.import_module(mod)
        if sym is not None:
            assert hasattr(m, sym) or importlib.import_module(mod + "." + sym), (mod, sym)
    for root, attrs in surf["chains"]:
        obj = importlib.import_module(root)
        path = root
        for p in attrs:
            path += "." + p
            obj = getattr(obj, p) if hasattr(obj, p) else importlib.import_module(path)
    from pyscf import tdscf as t
    assert t.TDDFT is not None and t.TDA is not None and t.TDHF is not None and t.RPA is not None


def test_pyscf_import_stays_lazy():
    import subprocess
    import sys
    code = "import sys, pyscf; assert 'pyscf.tdscf' not in sys.modules and 'mi355scf.tdscf' not in sys.modules"
    env = dict(os.environ, PYTHONPATH=os.pathsep.join(sys.path))
    subprocess.check_call([sys.executable, "-c", code], env=env)


def test_benzoquinone_fixture():
    from mi355scf import smiles_fixtures
    sym, xyz = smiles_fixtures.lookup("O=C1C=CC(=O)C=C1")
    assert sorted(sym) == sorted(["C"] * 6 + ["O"] * 2 + ["H"] * 4)
    # D2h: the structure is its own image under x -> -x and y -> -y
    for s in ((-1, 1, 1), (1, -1, 1)):
        img = xyz * np.array(s)
        d = np.linalg.norm(img[:, None, :] - xyz[None, :, :], axis=2)
        assert np.all(d.min(axis=1) < 1e-9)


def _problem(nocc, nvir, seed, degenerate=False, pure=False):
    rng = np.random.default_rng(seed)
    n = nocc * nvir
    de = np.sort(rng.uniform(0.3, 2.0, n))
    if degenerate:
        de[2] = de[1]
        de[5] = de[4]
    W = rng.standard_normal((n, n)) * 0.02
    A = np.diag(de) + 0.5 * (W + W.T)
    if degenerate:   # a symmetry that keeps pairs degenerate: swap of elements 1 <-> 2 and 4 <-> 5
        P = np.eye(n)
        P[[1, 2]] = P[[2, 1]]
        P[[4, 5]] = P[[5, 4]]
        A = 0.5 * (A + P @ A @ P.T)
    Bm = rng.standard_normal((n, n)) * 0.01
    B = 0.5 * (Bm + Bm.T)
    if degenerate:
        B = 0.5 * (B + P @ B @ P.T)
    if pure:   # A - B diagonal
        B = A - np.diag(de)
    return de, A, B


def _t(x):
    return torch.as_tensor(x, dtype=torch.float64)


@pytest.mark.parametrize("case", ["plain", "degenerate", "full"])
def test_davidson_tda_matches_eigh(case):
    de, A, _ = _problem(3, 5, 1, degenerate=case == "degenerate")
    n = A.shape[0]
    ns = n if case == "full" else 4
    At = _t(A)
    w, X, conv = tdscf.davidson_tda(lambda V: V @ At.T, _t(de), ns, conv_tol=1e-14, max_cycle=200)
    ref = np.linalg.eigvalsh(A)[:ns]
    assert conv.all()
    assert np.abs(w.numpy() - ref).max() < 1e-10
    # eigenvectors
    r = X.numpy() @ A - w.numpy()[:, None] * X.numpy()
    assert np.abs(r).max() < 1e-6


@pytest.mark.parametrize("case", ["plain", "degenerate", "full", "pure"])
def test_davidson_rpa_matches_eig(case):
    de, A, B = _problem(3, 5, 2, degenerate=case == "degenerate", pure=case == "pure")
    n = A.shape[0]
    ns = n if case == "full" else 4
    apb, amb = _t(A + B), _t(A - B)
    w, X, Y, conv = tdscf.davidson_rpa(lambda V: V @ apb.T, lambda V: V @ amb.T, _t(de), ns, conv_tol=1e-14, max_cycle=200)
    big = np.block([[A, B], [-B, -A]])
    ev = np.linalg.eigvals(big)
    ref = np.sort(ev.real[ev.real > 0])[:ns]
    assert np.abs(ev.imag).max() < 1e-12
    assert conv.all()
    assert np.abs(w.numpy() - ref).max() < 1e-10
    Xn, Yn = X.numpy(), Y.numpy()
    assert np.allclose((Xn * Xn).sum(1) - (Yn * Yn).sum(1), 0.5, atol=1e-10)
    # [[A, B], [-B, -A]] (X, Y) = w (X, Y)
    r1 = Xn @ A + Yn @ B - w.numpy()[:, None] * Xn
    assert np.abs(r1).max() < 1e-6


def test_initial_guess_keeps_degenerate_pairs():
    d = _t([0.5, 0.3, 0.7, 0.7, 0.9])
    V = tdscf.initial_guess(d, 3)
    assert V.shape[0] == 4 and set(V.argmax(1).tolist()) == {0, 1, 2, 3}


def test_oscillator_strength_formula():
    rng = np.random.default_rng(3)
    nocc, nvir = 2, 3
    dip = rng.standard_normal((3, nocc, nvir))
    e = np.array([0.3, 0.5])
    xy = [(rng.standard_normal((nocc, nvir)), rng.standard_normal((nocc, nvir))) for _ in e]
    f = tdscf.oscillator_strengths(e, xy, dip)
    for n, (x, y) in enumerate(xy):
        mu = np.array([2.0 * np.sum((x + y) * dip[c]) for c in range(3)])
        assert abs(f[n] - 2.0 / 3.0 * e[n] * mu @ mu) < 1e-14
    assert np.all(tdscf.oscillator_strengths(e, xy, dip, singlet=False) == 0.0)
