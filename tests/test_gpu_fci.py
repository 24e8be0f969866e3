"""The native determinant-FCI kernels and solver (`mi355scf.fci`, `mi_fci_*`) against the independent dense reference of
`test_fci_host.py` on random Hamiltonians with the full 8-fold symmetry and O(1) entries (fixed seeds).

Tolerances.  sigma and the diagonal: 1e-11 max(1, |reference|_max) -- each element is an FP64 sum of at most a few 1e5 O(1)
terms (about 1e-13 relative); the factor 100 covers the different summation order of the chunked GEMM.  Eigenvalues: 1e-9 with
the default conv_tol = 1e-10 (the energy error is second order in the residual).  Density matrices: 1e-11 per element.
"""
import functools
import itertools

import numpy as np
import pytest

from test_fci_host import random_integrals, ref_hamiltonian, ref_rdm12, ref_s2

pytestmark = pytest.mark.gpu

CASES = [(1, 1, 1), (2, 1, 1), (4, 2, 2), (5, 3, 2), (6, 3, 3), (6, 6, 0), (6, 5, 1), (7, 4, 3), (8, 4, 4)]


@functools.lru_cache(maxsize=None)
def _problem(norb, na, nb, seed=11):
    h, e = random_integrals(norb, seed + norb)
    return h, e, ref_hamiltonian(h, e, norb, (na, nb))


@functools.lru_cache(maxsize=None)
def _degenerate_problem():
    """(6, 3, 3) with h and eri invariant under every permutation of orbitals 0, 1, 2 (in particular under swapping two of them):
    the two-dimensional representation of that group gives exactly degenerate pairs, one of them the two lowest roots here
    (asserted by the test)."""
    norb = 6
    h, e = random_integrals(norb, 101)
    hs, es = np.zeros_like(h), np.zeros_like(e)
    for perm in itertools.permutations(range(3)):
        P = list(perm) + [3, 4, 5]
        hs += h[np.ix_(P, P)]
        es += e[np.ix_(P, P, P, P)]
    hs, es = hs / 6.0, es / 6.0
    return hs, es, ref_hamiltonian(hs, es, norb, (3, 3))


def _solver(**kw):
    from pyscf import fci
    s = fci.direct_spin1.FCI()
    for k, v in kw.items():
        setattr(s, k, v)
    return s


def _nstr(norb, n):
    from pyscf.fci import cistring
    return cistring.num_strings(norb, n)


def _vectors(norb, na, nb, nvec, seed=5):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((nvec, _nstr(norb, na), _nstr(norb, nb)))


@pytest.mark.parametrize("norb,na,nb", CASES)
def test_sigma_matches_dense_reference(norb, na, nb):
    """Both entry routes: the solver's own operator [1/2 (pq|rs) | h~] (`contract_h`) and PySCF's absorbed form (`contract_2e`)."""
    h, e, H = _problem(norb, na, nb)
    s = _solver()
    c = _vectors(norb, na, nb, 1)[0]
    ref = (H @ c.reshape(-1)).reshape(c.shape)
    tol = 1e-11 * max(1.0, np.abs(ref).max())
    got = s.contract_h(h, e, c, norb, (na, nb))
    got2 = s.contract_2e(s.absorb_h1e(h, e, norb, (na, nb), 0.5), c, norb, (na, nb))
    err, err2 = np.abs(got - ref).max(), np.abs(got2 - ref).max()
    print(f"({norb},{na},{nb}): {H.shape[0]} determinants, |sigma_ref|max {np.abs(ref).max():.3f}, worst error {err:.2e} "
          f"(absorbed form {err2:.2e}), tolerance {tol:.2e}")
    assert got.shape == c.shape and err <= tol and err2 <= tol


def test_sigma_chunked_and_batched_8_4_4():
    """Default workspace (one chunk), a workspace that forces at least three chunks with a ragged last one, and five vectors in
    one call (chunked as well, which also splits the batch): all against the reference."""
    norb, na, nb = 8, 4, 4
    h, e, H = _problem(norb, na, nb)
    c = _vectors(norb, na, nb, 5)
    ref = (H @ c.reshape(5, -1).T).T.reshape(c.shape)
    tol = 1e-11 * max(1.0, np.abs(ref).max())
    one = _solver()
    got1 = one.contract_h(h, e, c[0], norb, (na, nb))
    assert one.timing["chunks"] == 1
    nsa = nsb = 70
    row_mb = 2 * (norb ** 2 + 1) * nsb * 8 / 2 ** 20
    small = _solver(max_workspace_mb=27.5 * row_mb)          # 27 rows per chunk: 27 + 27 + 16
    got3 = small.contract_h(h, e, c[0], norb, (na, nb))
    assert small.timing["chunks"] == 3 and nsa % 27 != 0
    batch = _solver()
    gotb = batch.contract_h(h, e, c, norb, (na, nb))
    assert batch.timing["chunks"] == 1 and batch.timing["sigma_calls"] == 1
    small5 = _solver(max_workspace_mb=3.5 * row_mb)          # three of the five vectors per batch, one row per chunk
    gots = small5.contract_h(h, e, c, norb, (na, nb))
    assert small5.timing["chunks"] == 2 * nsa
    errs = [np.abs(got1 - ref[0]).max(), np.abs(got3 - ref[0]).max(), np.abs(gotb - ref).max(), np.abs(gots - ref).max()]
    print(f"(8,4,4): one chunk {errs[0]:.2e}, three chunks {errs[1]:.2e}, batch of 5 {errs[2]:.2e}, batch of 5 chunked {errs[3]:.2e}; "
          f"one chunk vs three chunks differ by {np.abs(got1 - got3).max():.2e}; tolerance {tol:.2e}")
    assert max(errs) <= tol


@pytest.mark.parametrize("norb,na,nb", CASES)
def test_hdiag_matches_reference_diagonal(norb, na, nb):
    h, e, H = _problem(norb, na, nb)
    hd = _solver().make_hdiag(h, e, norb, (na, nb))
    tol = 1e-11 * max(1.0, np.abs(np.diag(H)).max())
    err = np.abs(hd - np.diag(H)).max()
    print(f"({norb},{na},{nb}): worst diagonal error {err:.2e}, tolerance {tol:.2e}")
    assert hd.shape == (H.shape[0],) and err <= tol


def _check_roots(s, h, e, H, norb, nelec, nroots):
    w_ref = np.linalg.eigvalsh(H)[:nroots]
    en, ci = s.kernel(h, e, norb, nelec, nroots=nroots, ecore=0.25)
    if nroots == 1:
        assert np.isscalar(en) and isinstance(ci, np.ndarray) and ci.ndim == 2
        en, ci = np.array([en]), [ci]
    assert len(en) == nroots and len(ci) == nroots and np.all(s.converged)
    err = np.abs(np.sort(en) - 0.25 - w_ref).max()
    X = np.array([c.reshape(-1) for c in ci])
    ortho = np.abs(X @ X.T - np.eye(nroots)).max()
    ray = np.abs(np.einsum("ki,ij,kj->k", X, H, X) + 0.25 - en).max()
    print(f"norb {norb} nelec {nelec} nroots {nroots}: worst |E - E_ref| {err:.2e}, orthonormality {ortho:.2e}, "
          f"Rayleigh quotient vs reported energy {ray:.2e}")
    assert err <= 1e-9 and ortho <= 1e-8 and ray <= 1e-9
    return en


@pytest.mark.parametrize("norb,na,nb", [(6, 3, 3), (8, 4, 4)])
@pytest.mark.parametrize("nroots", [1, 5])
def test_lowest_roots_match_dense_diagonalisation(norb, na, nb, nroots):
    h, e, H = _problem(norb, na, nb)
    _check_roots(_solver(), h, e, H, norb, (na, nb), nroots)


def test_exactly_degenerate_pair_is_found():
    h, e, H = _degenerate_problem()
    w = np.linalg.eigvalsh(H)[:6]
    gaps = np.diff(w[:5])
    print(f"lowest reference roots {w}, gaps {gaps}")
    assert gaps.min() < 1e-11                               # an exactly degenerate pair inside the five lowest
    _check_roots(_solver(), h, e, H, 6, (3, 3), 5)


@pytest.mark.parametrize("norb,na,nb", [(4, 2, 2), (5, 3, 2), (5, 3, 0)])
def test_density_matrices_match_reference(norb, na, nb):
    h, e, H = _problem(norb, na, nb)
    s = _solver(max_workspace_mb=2.5 * 2 * (norb ** 2 + 1) * _nstr(norb, nb) * 8 / 2 ** 20)    # two alpha rows per chunk
    w, U = np.linalg.eigh(H)
    c0 = U[:, 0].reshape(_nstr(norb, na), _nstr(norb, nb))
    c1 = _vectors(norb, na, nb, 1)[0]
    c1 /= np.linalg.norm(c1)
    r1, r2 = ref_rdm12(c0, c0, norb, (na, nb))
    t1, t2 = ref_rdm12(c1, c0, norb, (na, nb))
    dm1 = s.make_rdm1(c0, norb, (na, nb))
    dm1b, dm2 = s.make_rdm12(c0, norb, (na, nb))
    tdm1 = s.trans_rdm1(c1, c0, norb, (na, nb))
    tdm1b, tdm2 = s.trans_rdm12(c1, c0, norb, (na, nb))
    errs = [np.abs(dm1 - r1).max(), np.abs(dm1b - r1).max(), np.abs(dm2 - r2).max(), np.abs(tdm1 - t1).max(),
            np.abs(tdm1b - t1).max(), np.abs(tdm2 - t2).max()]
    n = na + nb
    tr1, tr2 = np.trace(dm1), np.einsum("ppqq->", dm2)
    en = np.sum(h * dm1) + 0.5 * np.sum(e * dm2)
    print(f"({norb},{na},{nb}): dm1 {errs[0]:.2e}/{errs[1]:.2e}, dm2 {errs[2]:.2e}, trans dm1 {errs[3]:.2e}/{errs[4]:.2e}, trans dm2 "
          f"{errs[5]:.2e}; traces {tr1:.12f}, {tr2:.12f}; energy from RDMs - E {en - w[0]:.2e}")
    assert max(errs) <= 1e-11
    assert abs(tr1 - n) <= 1e-11 and abs(tr2 - n * (n - 1)) <= 1e-10 and abs(en - w[0]) <= 1e-10 * max(1.0, abs(w[0]))


@pytest.mark.parametrize("norb,na,nb", [(4, 2, 2), (5, 3, 2), (6, 4, 2)])
def test_spin_square_matches_reference_operator(norb, na, nb):
    s = _solver()
    S2 = ref_s2(norb, (na, nb))
    w, U = np.linalg.eigh(S2)
    shape = (_nstr(norb, na), _nstr(norb, nb))
    smin = 0.5 * (na - nb)
    low = U[:, np.abs(w - smin * (smin + 1)) < 1e-9][:, 0]                 # lowest spin (singlet for na = nb)
    high = U[:, np.abs(w - (smin + 1) * (smin + 2)) < 1e-9][:, 0]          # next multiplicity (triplet for na = nb)
    mixed = _vectors(norb, na, nb, 1, seed=9)[0].reshape(-1)
    worst = 0.0
    for name, v in (("low", low), ("high", high), ("mixed", mixed), ("unnormalised", 3.0 * (low + 0.5 * high))):
        ss, mult = s.spin_square(v.reshape(shape), norb, (na, nb))
        ref = v @ S2 @ v / (v @ v)
        worst = max(worst, abs(ss - ref))
        assert abs(mult - (2 * (np.sqrt(ref + 0.25) - 0.5) + 1)) < 1e-9
    print(f"({norb},{na},{nb}): worst |<S^2> - reference| {worst:.2e}")
    assert worst <= 1e-11


def test_large_ci_and_integer_nelec():
    norb = 4
    h, e, H = _problem(norb, 2, 2)
    s = _solver()
    en, ci = s.kernel(h, e, norb, 4)                     # an int: split by Ms = 0
    assert abs(en - np.linalg.eigvalsh(H)[0]) <= 1e-9
    big = s.large_ci(ci, norb, (2, 2), tol=0.2)
    assert len(big) == int((np.abs(ci) > 0.2).sum()) and all(a.count("1") == 2 and b.count("1") == 2 for _, a, b in big)
    occ = s.large_ci(ci, norb, (2, 2), tol=0.2, return_strs=False)
    assert all(len(a) == 2 and len(b) == 2 for _, a, b in occ)


def test_space_beyond_the_memory_cap_is_refused():
    norb, na, nb = 6, 3, 3
    h, e, _ = _problem(norb, na, nb)
    s = _solver(max_memory=0.2)                          # MB: 400 determinants x (1 + 2 x 40 + 4) vectors need 0.26 MB
    with pytest.raises(NotImplementedError, match="400 determinants"):
        s.kernel(h, e, norb, (na, nb))
    with pytest.raises(NotImplementedError, match="max_workspace_mb"):
        _solver(max_workspace_mb=0.001).contract_h(h, e, _vectors(norb, na, nb, 1)[0], norb, (na, nb))
    with pytest.raises(NotImplementedError, match="16"):
        s.kernel(np.zeros((17, 17)), np.zeros((17,) * 4), 17, (1, 1))
