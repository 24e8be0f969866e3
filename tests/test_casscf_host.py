"""CPU-side checks of the CASSCF layer (no GPU): the orbital-gradient and rotation algebra of `mi355scf.casscf` against finite
differences of the energy, state-average weights, the AVAS linear algebra on a planted subspace, AO labels, and the import
surface of the reference's calculate_casscf.py (names only, tests/golden/template_surface_casscf.json).

The energy the finite difference differentiates is written here from dense integrals and shares nothing with the module:
    E(C) = sum_i 2 h_ii + sum_ij [2 (ii|jj) - (ij|ij)] + sum_tu gamma_tu [h_tu + sum_i (2 (tu|ii) - (ti|ui))] + 1/2 sum Gamma_tuvw (tu|vw)
with the RDMs held fixed while the orbitals rotate.  The CI vector is the ground state of `test_fci_host.ref_hamiltonian`."""
import importlib
import json
import os

import numpy as np
import pytest

from conftest import MOLECULES
from test_fci_host import random_integrals, ref_hamiltonian, ref_rdm12

HERE = os.path.dirname(os.path.abspath(__file__))
N, NCORE, NCAS, NELECAS = 6, 1, 3, (1, 1)


def _energy(h, eri, C, gamma, Gamma):
    hm = C.T @ h @ C
    em = np.einsum("pqrs,pi,qj,rk,sl->ijkl", eri, C, C, C, C, optimize=True)
    c, a = slice(0, NCORE), slice(NCORE, NCORE + NCAS)
    e = 2.0 * np.trace(hm[c, c]) + 2.0 * np.einsum("iijj->", em[c, c, c, c]) - np.einsum("ijij->", em[c, c, c, c])
    hc = hm[a, a] + 2.0 * np.einsum("tuii->tu", em[a, a, c, c]) - np.einsum("tiui->tu", em[a, c, a, c])
    return e + np.sum(gamma * hc) + 0.5 * np.sum(Gamma * em[a, a, a, a])


@pytest.fixture(scope="module")
def model():
    h, eri = random_integrals(N, 4242)
    rng = np.random.default_rng(7)
    C, _ = np.linalg.qr(rng.standard_normal((N, N)))
    hm = C.T @ h @ C
    em = np.einsum("pqrs,pi,qj,rk,sl->ijkl", eri, C, C, C, C, optimize=True)
    c, a = slice(0, NCORE), slice(NCORE, NCORE + NCAS)
    hc = hm[a, a] + 2.0 * np.einsum("tuii->tu", em[a, a, c, c]) - np.einsum("tiui->tu", em[a, c, a, c])
    H = ref_hamiltonian(hc, em[a, a, a, a], NCAS, NELECAS)
    w, V = np.linalg.eigh(H)
    gamma, Gamma = ref_rdm12(V[:, 0], V[:, 0], NCAS, NELECAS)
    return h, eri, C, gamma, Gamma


def _module_gradient(h, eri, C, gamma, Gamma):
    from mi355scf import casscf
    hm = C.T @ h @ C
    em = np.einsum("pqrs,pi,qj,rk,sl->ijkl", eri, C, C, C, C, optimize=True)
    c, a = slice(0, NCORE), slice(NCORE, NCORE + NCAS)
    FI = hm + 2.0 * np.einsum("pqii->pq", em[:, :, c, c]) - np.einsum("piqi->pq", em[:, c, :, c])
    FA = np.einsum("pqtu,tu->pq", em[:, :, a, a], gamma) - 0.5 * np.einsum("ptqu,tu->pq", em[:, a, :, a], gamma)
    F = casscf.generalized_fock(FI, FA, gamma, Gamma, em[:, a, a, a], NCORE, NCAS)
    return casscf.orbital_gradient(F, NCORE, NCAS)


def test_gradient_matches_central_finite_differences(model):
    from mi355scf import casscf
    h, eri, C, gamma, Gamma = model
    g = _module_gradient(h, eri, C, gamma, Gamma)
    p, q = casscf.rotation_pairs(N, NCORE, NCAS)
    assert len(p) == NCORE * NCAS + NCORE * (N - NCORE - NCAS) + NCAS * (N - NCORE - NCAS)
    step = 1e-4
    worst = 0.0
    for k in range(len(p)):
        x = np.zeros(len(p))
        x[k] = step
        ep = _energy(h, eri, casscf.rotate(C, x, NCORE, NCAS), gamma, Gamma)
        em_ = _energy(h, eri, casscf.rotate(C, -x, NCORE, NCAS), gamma, Gamma)
        fd = (ep - em_) / (2 * step)
        worst = max(worst, abs(fd - g[p[k], q[k]]))
        assert abs(fd - g[p[k], q[k]]) < 1e-7, (p[k], q[k], fd, g[p[k], q[k]])
    print(f"max |g - finite difference| = {worst:.2e} over {len(p)} rotations, max |g| = {np.abs(g).max():.3f}")
    assert np.abs(g).max() > 1e-2                      # a non-stationary point: the comparison is not 0 == 0
    mask = np.ones((N, N), dtype=bool)
    mask[p, q] = mask[q, p] = False
    assert np.all(g[mask] == 0.0)                      # redundant blocks exactly zero
    assert np.array_equal(g, -g.T)
    assert np.array_equal(casscf.pack(g, NCORE, NCAS), g[p, q])


def test_rotation_is_orthogonal():
    from mi355scf import casscf
    rng = np.random.default_rng(11)
    p, _ = casscf.rotation_pairs(N, NCORE, NCAS)
    for scale in (1e-3, 0.3, 3.0):
        x = scale * rng.standard_normal(len(p))
        U = casscf.expm_antisym(casscf.kappa_matrix(x, N, NCORE, NCAS))
        assert np.abs(U.T @ U - np.eye(N)).max() < 1e-13
    K = casscf.kappa_matrix(1e-3 * rng.standard_normal(len(p)), N, NCORE, NCAS)
    assert np.abs(casscf.expm_antisym(K) - (np.eye(N) + K + K @ K / 2 + K @ K @ K / 6)).max() < 1e-12
    assert np.array_equal(casscf.expm_antisym(np.zeros((N, N))), np.eye(N))


def test_lbfgs_direction_reproduces_newton_on_a_quadratic():
    from mi355scf import casscf
    rng = np.random.default_rng(5)
    A = rng.standard_normal((5, 5))
    A = A @ A.T + 5 * np.eye(5)
    g0 = rng.standard_normal(5)
    assert np.allclose(casscf.lbfgs_direction(g0, np.diag(A), [], []), -g0 / np.diag(A))
    S = [rng.standard_normal(5) for _ in range(5)]
    d = casscf.lbfgs_direction(g0, np.ones(5), S, [A @ s for s in S])
    assert float(d @ g0) < 0


def test_lowest_eigenpair_finds_negative_curvature_and_null_directions():
    """The stability search's Davidson on a diagonally dominant matrix (spectrum 1.5 .. 80, as an orbital Hessian's) with (a) one
    planted eigenvalue -0.06 on a soft, otherwise decoupled rotation -- the symmetric saddle's shape -- and (b) an exactly null
    block (redundant rotations): the lowest eigenvalue is found to 1e-6 in far fewer products than the dimension."""
    from mi355scf import casscf
    rng = np.random.default_rng(3)
    n = 71
    A = rng.standard_normal((n, n))
    A = A @ A.T / n + np.diag(np.linspace(1.5, 80.0, n))
    A[:6] = 0.0
    A[:, :6] = 0.0
    for planted in (0.0, -0.06):
        A[2, 2] = planted
        count = [0]

        def matvec(v):
            count[0] += 1
            return A @ v

        hdiag = np.maximum(np.abs(np.diag(A)), 0.05)
        theta, x, done = casscf.lowest_eigenpair(matvec, hdiag, tol=1e-6)
        assert done and count[0] <= 12
        assert abs(theta - planted) < 1e-6 and abs(np.linalg.norm(x) - 1.0) < 1e-12
        assert np.linalg.norm(A @ x - theta * x) < 1e-6
        theta, x, _ = casscf.lowest_eigenpair(matvec, hdiag, below=-5e-6)
        assert (theta < -5e-6) == (planted < 0)


def test_state_average_weights_and_rdms():
    from mi355scf import casscf
    for bad in ([0.7, 0.7], [1.5, -0.5], [], [0.5, float("nan")], [0.3, 0.3]):
        with pytest.raises(ValueError):
            casscf.check_weights(bad)
    assert np.array_equal(casscf.check_weights([0.25, 0.75]), [0.25, 0.75])
    assert np.array_equal(casscf.check_weights([1.0]), [1.0])
    rng = np.random.default_rng(3)
    rdms = [(rng.standard_normal((3, 3)), rng.standard_normal((3, 3, 3, 3))) for _ in range(3)]
    w = [0.5, 0.3, 0.2]
    g, G = casscf.average_rdms(w, rdms)
    assert np.allclose(g, sum(wi * r[0] for wi, r in zip(w, rdms)), rtol=0, atol=1e-15)
    assert np.allclose(G, sum(wi * r[1] for wi, r in zip(w, rdms)), rtol=0, atol=1e-15)
    with pytest.raises(ValueError):
        casscf.average_rdms([0.5, 0.5], rdms)


def test_pair_packing_is_the_kernels_order():
    from mi355scf import casscf
    v, w = casscf.pair_index(4)
    assert list(v * (v + 1) // 2 + w) == list(range(10)) and np.all(v >= w)
    X = np.arange(10.0)
    U = casscf.unpack_pairs(X, 4)
    assert np.array_equal(U, U.T) and U[3, 1] == 3 * 4 // 2 + 1


def _principal_angle(A, B):
    qa, _ = np.linalg.qr(A)
    qb, _ = np.linalg.qr(B)
    s = np.linalg.svd(qa.T @ qb, compute_uv=False)
    # sin of the largest angle from the projector difference: accurate near 0 where arccos of the cosine is not
    return float(np.linalg.norm(qa @ qa.T - qb @ qb.T, 2)), s


def test_avas_algebra_recovers_a_planted_subspace():
    """Orthonormal AOs (S = 1), 10 orbitals, 4 occupied.  The two reference functions are one vector inside the occupied space
    and one inside the virtual space (orthonormal, S22 = 1), so C^T P C has exactly one unit eigenvalue in each space and zeros
    elsewhere: one occupied and one virtual orbital are kept, and they span the planted vectors."""
    from mi355scf import avas
    rng = np.random.default_rng(99)
    n, nocc = 10, 4
    C, _ = np.linalg.qr(rng.standard_normal((n, n)))
    occ = np.array([2.0] * nocc + [0.0] * (n - nocc))
    a = C[:, :nocc] @ rng.standard_normal(nocc)
    b = C[:, nocc:] @ rng.standard_normal(n - nocc)
    S12 = np.stack([a / np.linalg.norm(a), b / np.linalg.norm(b)], axis=1)
    # a non-orthogonal description of the same two functions: S22 is no unit matrix
    M = np.array([[1.0, 0.4], [0.3, 0.9]])
    S12m, S22m = S12 @ M, M.T @ M
    F = C @ np.diag(np.arange(n, dtype=float)) @ C.T
    for canon in (True, False):
        ncas, nelecas, mo, kept = avas.avas_algebra(C, occ, np.eye(n), S12m, S22m, F, threshold=0.2, canonicalize=canon)
        assert (ncas, nelecas, kept) == (2, 2, (1, 1))
        assert np.abs(mo.T @ mo - np.eye(n)).max() < 1e-12
        act = mo[:, nocc - 1:nocc + 1]
        angle, _ = _principal_angle(act, S12)
        print(f"canonicalize={canon}: sin(largest principal angle) = {angle:.2e}")
        assert angle <= 1e-10
        # occupied and virtual spaces are preserved as a whole
        assert _principal_angle(mo[:, :nocc], C[:, :nocc])[0] < 1e-10
        if canon:
            fb = mo[:, :nocc - 1].T @ F @ mo[:, :nocc - 1]
            assert np.abs(fb - np.diag(np.diag(fb))).max() < 1e-10
    # a threshold above 1 keeps nothing
    assert avas.avas_algebra(C, occ, np.eye(n), S12m, S22m, F, threshold=1.5)[:2] == (0, 0)
    with pytest.raises(NotImplementedError):
        avas.avas_algebra(C, np.array([2.0, 2, 2, 1, 1, 0, 0, 0, 0, 0]), np.eye(n), S12m, S22m, F)


def test_ao_labels_and_search():
    from mi355scf.mole import Mole
    mol = Mole(atom=MOLECULES["h2co"], basis="6-31g(d)", verbose=0).build()
    labels = mol.ao_labels()
    assert len(labels) == mol.nao == 32
    assert labels[0] == "0 C 1s" and "0 C 2px" in labels and "1 O 3dz^2" in labels and "2 H 2s" in labels
    assert len(set(labels)) == len(labels)
    assert len(mol.search_ao_label("C 2p")) == 3
    assert len(mol.search_ao_label("2pz")) == 2                    # one per heavy atom
    assert len(mol.search_ao_label("H 1s")) == 2
    assert len(mol.search_ao_label("3d")) == 10
    assert len(mol.search_ao_label(["C 2p", "O 2p"])) == 6
    assert len(mol.search_ao_label("[CO] 2p")) == 6                # a regular expression
    assert len(mol.search_ao_label("2p")) == 6 and len(mol.search_ao_label("nothing")) == 0
    assert list(mol.search_ao_label("C 2p")) == [labels.index(f"0 C 2p{m}") for m in "xyz"]
    assert mol.ao_labels(fmt=False)[0] == (0, "C", "1s", "")


def test_casscf_template_import_surface():
    with open(os.path.join(HERE, "golden", "template_surface_casscf.json")) as fh:
        surf = json.load(fh)
    assert ["pyscf.mcscf", "avas"] in surf["imports"] and ["pyscf", "tools"] in surf["imports"]
    for mod, sym in surf["imports"]:
        m = importlib.import_module(mod)
        if sym is not None:
            assert hasattr(m, sym) or importlib.import_module(mod + "." + sym), (mod, sym)
    for root, attrs in surf["chains"]:
        obj = importlib.import_module(root)
        path = root
        for p in attrs:
            if not (type(obj).__name__ == "module"):
                break                                               # a class or function: what follows is a call result
            path += "." + p
            obj = getattr(obj, p) if hasattr(obj, p) else importlib.import_module(path)
    from pyscf import mcscf, tools
    from pyscf.mcscf import avas
    import gpu4pyscf.mcscf
    assert callable(avas.avas) and gpu4pyscf.mcscf.avas.avas is avas.avas
    assert isinstance(mcscf.CASSCF, type) and issubclass(mcscf.CASSCF, mcscf.CASCI) and gpu4pyscf.mcscf.CASSCF is mcscf.CASSCF
    assert all(hasattr(mcscf.CASSCF, a) for a in ("state_average", "state_average_", "kernel", "conv_tol", "max_cycle_macro"))
    for fn in (tools.molden.header, tools.molden.orbital_coeff):
        with pytest.raises(NotImplementedError, match="tools.molden is not implemented"):
            fn(None, None) if fn is tools.molden.header else fn(None, None, None)


def test_active_pair_entry_point_is_exported_and_declared():
    from mi355scf import engine
    from conftest import ROOT
    L = engine.lib()
    assert L.mi_eri_active_j is not None
    assert engine.Engine.active_pair_width() == int(L.mi_eri_active_j_width()) >= 16
    hdr = open(os.path.join(ROOT, "include", "mi355scf.h")).read()
    assert "int mi_eri_active_j(mi_ctx *ctx, const double *d_Ca, int ncas, int ldc, double *d_Jp, void *stream);" in hdr
