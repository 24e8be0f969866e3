"""The native determinant-FCI kernels and solver (`mi355scf.fci`, `mi_fci_*`) against the independent dense reference of
`test_fci_host.py` on random Hamiltonians with the full 8-fold symmetry and O(1) entries (fixed seeds).

Tolerances.  sigma and the diagonal: 1e-11 max(1, |reference|_max) -- each element is an FP64 sum of at most a few 1e5 O(1)
terms (about 1e-13 relative); the factor 100 covers the different summation order of the chunked GEMM.  Eigenvalues: 1e-9 with
the default conv_tol = 1e-10 (the energy error is second order in the residual).  Density matrices: 1e-11 per element.

CASES (dense reference) stops at (8,4,4), 70 beta strings: one block shape of the gather kernels.  LARGE runs every other
launch shape -- more than one beta strip per thread, 1024-thread blocks, the LDS limit raised above 64 KB, norb up to 16,
na = 0 -- against the matrix-free reference of `test_fci_host.py` (`ref_sigma` and friends), same tolerances.
"""
import functools
import itertools

import numpy as np
import pytest

from test_fci_host import (random_integrals, ref_hamiltonian, ref_hdiag, ref_rdm12, ref_rdm12_large, ref_s2, ref_sigma, ref_spin_E,
                           ref_spin_square_large)

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


# =================================================================================================
# every launch shape of the gather kernels, against the matrix-free reference
# =================================================================================================
# fci_threads(nsb) = 1024 for nsb >= 1024, else nsb rounded up to 64; thread t of the sigma gather owns the beta strings
# t + k * 1024, k < FCI_NPT = 13; the staged beta row needs 8 nsb bytes of LDS, above 64 KB (nsb > 8192) through
# hipFuncSetAttribute.  CASES stops at nsb = 70: one block shape, k = 0 only, norb <= 8.
LARGE = [(9, 4, 4),       # 126 x 126: first norb beyond a byte of the mask; T = 128
         (12, 2, 6),      # 66 x 924: the largest block below 1024 threads (T = 960)
         (14, 1, 4),      # 14 x 1001: T = 1024 with idle lanes, k = 0 only
         (13, 1, 6),      # 13 x 1716: k in {0, 1}, ragged second strip (692)
         (14, 0, 7),      # 1 x 3432: na = 0 (no alpha links, the dummy table), k up to 3
         (16, 0, 8),      # 1 x 12870: k up to 12 (ragged 582); 102 960 B of LDS: the raised limit
         (16, 1, 7),      # 16 x 11440: the raised limit with alpha links
         (16, 7, 1)]      # 11440 x 16: T = 64, 70 alpha links, many alpha rows


@functools.lru_cache(maxsize=None)
def _large_problem(norb, na, nb):
    """(h, eri, c, ref_sigma(c), ref_hdiag) of a LARGE case; c is the first of `_vectors`."""
    h, e = random_integrals(norb, 11 + norb)
    c = _vectors(norb, na, nb, 1)[0]
    return h, e, c, ref_sigma(h, e, norb, (na, nb), c), ref_hdiag(h, e, norb, (na, nb))


def _row_mb(norb, nsb):
    """MB of one alpha row of the two work arrays D and F for one vector."""
    return 2 * (norb ** 2 + 1) * nsb * 8 / 2 ** 20


@pytest.mark.parametrize("norb,na,nb", LARGE)
def test_sigma_and_diagonal_at_every_launch_shape(norb, na, nb):
    """`contract_h`, `contract_2e(absorb_h1e(...))` and `make_hdiag` against `ref_sigma` / `ref_hdiag`, the file's tolerance
    rule (an element is a sum of at most 257 + 272 FP64 terms).
    MI355X, worst sigma error (absorbed form) at |sigma_ref|max, diagonal error: (9,4,4) 7.1e-14 (8.5e-14) at 153, 1.1e-14;
    (12,2,6) 9.9e-14 (1.6e-13) at 158, 1.4e-14; (14,1,4) 7.1e-14 (8.5e-14) at 117, 7.1e-15; (13,1,6) 8.5e-14 (9.9e-14) at 148,
    1.1e-14; (14,0,7) 7.1e-14 (8.5e-14) at 117, 1.4e-14; (16,0,8) 7.1e-14 (1.1e-13) at 161, 1.4e-14; (16,1,7) 2.0e-13 (1.7e-13)
    at 255, 1.8e-14; (16,7,1) 2.0e-13 (1.9e-13) at 219, 1.8e-14: at most 1e-4 of the tolerance."""
    h, e, c, ref, hd_ref = _large_problem(norb, na, nb)
    s = _solver()
    tol = 1e-11 * max(1.0, np.abs(ref).max())
    got = s.contract_h(h, e, c, norb, (na, nb))
    got2 = s.contract_2e(s.absorb_h1e(h, e, norb, (na, nb), 0.5), c, norb, (na, nb))
    hd = s.make_hdiag(h, e, norb, (na, nb))
    told = 1e-11 * max(1.0, np.abs(hd_ref).max())
    err, err2, errd = np.abs(got - ref).max(), np.abs(got2 - ref).max(), np.abs(hd - hd_ref.reshape(-1)).max()
    print(f"({norb},{na},{nb}): {ref.shape[0]} x {ref.shape[1]} determinants, |sigma_ref|max {np.abs(ref).max():.3f}, worst error {err:.2e} "
          f"(absorbed form {err2:.2e}), tolerance {tol:.2e}; diagonal {errd:.2e}, tolerance {told:.2e}")
    assert s.timing["chunks"] == 2 and got.shape == c.shape and hd.shape == (c.size,)
    assert err <= tol and err2 <= tol and errd <= told


@pytest.mark.parametrize("norb,na,nb", LARGE)
def test_spin_square_at_every_launch_shape(norb, na, nb):
    """`mi_fci_gather_d` modes 1 and 2 at size: a normalised random vector and an unnormalised one.
    MI355X: worst |<S^2> - reference| 8.9e-16 at (9,4,4) and (12,2,6), 0 at the other six."""
    s = _solver()
    v = _vectors(norb, na, nb, 2, seed=9)
    worst = 0.0
    for c in (v[0] / np.linalg.norm(v[0]), 3.0 * v[1]):
        ss, mult = s.spin_square(c, norb, (na, nb))
        ref = ref_spin_square_large(c, norb, (na, nb))
        worst = max(worst, abs(ss - ref))
        assert abs(mult - (2 * (np.sqrt(ref + 0.25) - 0.5) + 1)) < 1e-9
    print(f"({norb},{na},{nb}): worst |<S^2> - reference| {worst:.2e}")
    assert worst <= 1e-11


def test_sigma_chunked_and_batched_at_size():
    """(16,1,7): 5 + 5 + 5 + 1 alpha rows per chunk (one row of D and F is 44.9 MB) and one chunk; (13,1,6): two vectors in
    one call; (16,7,1): 5000 + 5000 + 1440 alpha rows.  Every call sets its own `max_workspace_mb`.
    MI355X, error / max(1, |ref|max): 7.8e-16 (four chunks), 7.8e-16 (one chunk), 6.2e-16 (batch of two), 7.8e-16 (three chunks)."""
    norb, na, nb = 16, 1, 7
    h, e, c, ref, _ = _large_problem(norb, na, nb)
    row = _row_mb(norb, 11440)
    four = _solver(max_workspace_mb=5.5 * row)
    got4 = four.contract_h(h, e, c, norb, (na, nb))
    one = _solver(max_workspace_mb=16.5 * row)
    got1 = one.contract_h(h, e, c, norb, (na, nb))
    assert four.timing["chunks"] == 4 and one.timing["chunks"] == 1
    errs = [np.abs(got4 - ref).max() / max(1.0, np.abs(ref).max()), np.abs(got1 - ref).max() / max(1.0, np.abs(ref).max())]

    norb, na, nb = 13, 1, 6
    h, e, c, ref, _ = _large_problem(norb, na, nb)
    c2 = _vectors(norb, na, nb, 2)
    assert np.array_equal(c2[0], c)
    ref2 = np.stack([ref, ref_sigma(h, e, norb, (na, nb), c2[1])])
    batch = _solver(max_workspace_mb=2 * 13.5 * _row_mb(norb, 1716))
    gotb = batch.contract_h(h, e, c2, norb, (na, nb))
    assert batch.timing["chunks"] == 1 and batch.timing["sigma_calls"] == 1 and gotb.shape == c2.shape
    errs.append(np.abs(gotb - ref2).max() / max(1.0, np.abs(ref2).max()))

    norb, na, nb = 16, 7, 1
    h, e, c, ref, _ = _large_problem(norb, na, nb)
    three = _solver(max_workspace_mb=5000.5 * _row_mb(norb, 16))
    got3 = three.contract_h(h, e, c, norb, (na, nb))
    assert three.timing["chunks"] == 3 and 11440 % 5000 != 0
    errs.append(np.abs(got3 - ref).max() / max(1.0, np.abs(ref).max()))
    print(f"error / max(1, |ref|max): (16,1,7) four chunks {errs[0]:.2e}, one chunk {errs[1]:.2e}; (13,1,6) batch of two {errs[2]:.2e}; "
          f"(16,7,1) three chunks {errs[3]:.2e}; tolerance 1e-11")
    assert max(errs) <= 1e-11


@pytest.mark.parametrize("norb,na,nb,rows", [(13, 1, 6, 5), (16, 1, 7, 6)])
def test_density_matrices_at_size(norb, na, nb, rows):
    """`make_rdm12` / `trans_rdm12` of normalised random vectors in three row chunks (5 + 5 + 3, 6 + 6 + 4) against
    `ref_rdm12_large`, 1e-11 per element; traces and the energy from the density matrices against <c|ref_sigma(c)>.
    MI355X, (13,1,6) / (16,1,7): dm1 1.0e-15 / 3.1e-15, dm2 1.4e-15 / 3.9e-15, transition dm1 2.9e-17 / 3.0e-17, transition dm2
    4.0e-17 / 4.9e-17, energy from the RDMs - <c|H|c> 7.8e-15 / -8.9e-15."""
    h, e, c, sig, _ = _large_problem(norb, na, nb)
    nrm = np.linalg.norm(c)
    c0 = c / nrm
    c1 = _vectors(norb, na, nb, 1, seed=6)[0]
    c1 /= np.linalg.norm(c1)
    s = _solver(max_workspace_mb=(rows + 0.5) * _row_mb(norb, _nstr(norb, nb)))
    assert s._chunks(s._tab(norb, (na, nb)), 1)[1] == rows and _nstr(norb, na) % rows != 0
    r1, r2 = ref_rdm12_large(c0, c0, norb, (na, nb))
    t1, t2 = ref_rdm12_large(c1, c0, norb, (na, nb))
    dm1, dm2 = s.make_rdm12(c0, norb, (na, nb))
    tdm1, tdm2 = s.trans_rdm12(c1, c0, norb, (na, nb))
    errs = [np.abs(dm1 - r1).max(), np.abs(dm2 - r2).max(), np.abs(tdm1 - t1).max(), np.abs(tdm2 - t2).max()]
    n = na + nb
    tr1, tr2 = np.trace(dm1), np.einsum("ppqq->", dm2)
    en, en_ref = np.sum(h * dm1) + 0.5 * np.sum(e * dm2), np.sum(c * sig) / nrm ** 2
    print(f"({norb},{na},{nb}): dm1 {errs[0]:.2e}, dm2 {errs[1]:.2e}, trans dm1 {errs[2]:.2e}, trans dm2 {errs[3]:.2e}; traces {tr1:.12f}, "
          f"{tr2:.12f}; energy from RDMs - <c|H|c> {en - en_ref:.2e}")
    assert max(errs) <= 1e-11
    assert abs(tr1 - n) <= 1e-11 and abs(tr2 - n * (n - 1)) <= 1e-10 and abs(en - en_ref) <= 1e-10 * max(1.0, abs(en_ref))


def test_gather_d_planes_through_the_c_abi():
    """`mi_fci_gather_d` at (13,1,6) (two beta strips), rows [4, 11) of 13, two vectors, modes 1, 2 and 3: every plane against
    Ea_rs C, C Eb_rs^T and their sum, and plane norb^2 against C.  Entries are +-c or a sum of two such: exact, one ulp of the
    sum allowed.  The output starts as NaN (an element not written shows) and is followed by a guard band.
    MI355X: all 4 084 080 elements bit-identical in each of the three modes (336 336, 1 177 176 and 1 400 784 of them non-zero)."""
    import ctypes
    import torch
    from mi355scf import engine
    from test_gpu_dense_kernels import assert_guard, guarded
    norb, na, nb = 13, 1, 6
    n2, nsa, nsb, a0, nrow, nvec = norb * norb, 13, 1716, 4, 7, 2
    s = _solver()
    tb = s._tab(norb, (na, nb))
    assert (tb["nsa"], tb["nsb"], tb["nla"]) == (nsa, nsb, 13)
    c = _vectors(norb, na, nb, nvec, seed=8)
    Ea, Eb = ref_spin_E(norb, na, 0), ref_spin_E(norb, nb, 1)
    A = np.stack([[Ea[r][q] @ c[v] for v in range(nvec)] for r in range(norb) for q in range(norb)])[:, :, a0:a0 + nrow]
    B = np.stack([[(Eb[r][q] @ c[v].T).T for v in range(nvec)] for r in range(norb) for q in range(norb)])[:, :, a0:a0 + nrow]
    own = c[None, :, a0:a0 + nrow]
    dc = torch.as_tensor(c, device=tb["dev"]).contiguous()
    size = (n2 + 1) * nvec * nrow * nsb
    for mode, ref in ((1, A), (2, B), (3, A + B)):
        ref = np.concatenate([ref, own]).reshape(-1)
        buf = guarded(size)
        buf[:size] = float("nan")
        engine._check(engine.lib().mi_fci_gather_d(dc.data_ptr(), nvec, nsa, nsb, norb, a0, nrow, tb["alink"].data_ptr(), tb["nla"],
                                                   tb["btab"].data_ptr(), mode, buf.data_ptr(),
                                                   ctypes.c_void_p(torch.cuda.current_stream(tb["dev"]).cuda_stream)))
        torch.cuda.synchronize()
        got = buf[:size].cpu().numpy()
        assert_guard(buf, size, f"gather_d mode {mode}")
        assert not np.isnan(got).any(), f"mode {mode}: {int(np.isnan(got).sum())} elements not written"
        bad = np.abs(got - ref) > np.spacing(np.abs(ref))
        print(f"mode {mode}: {int(np.count_nonzero(ref))} non-zero reference entries of {size}, {int((got != ref).sum())} not bit-identical, "
              f"{int(bad.sum())} beyond one ulp")
        assert not bad.any()


def test_solver_at_13_1_6():
    """One `kernel()` where the sigma gather runs two strips.  The Davidson stops when the 2-norm of its residual (H c - E c) is
    below sqrt(conv_tol) = 1e-5 and the energy moved by less than conv_tol = 1e-10; the returned vector is that Ritz vector
    (renormalised), so against one `ref_sigma` |H_ref c - E c|_max <= |H_ref c - E c|_2 <= sqrt(conv_tol) + sqrt(ndet) x the
    sigma tolerance (the solver's residual is built from the device's sigma), and the Rayleigh quotient is the reported energy
    to rounding (1e-9 asked).  That the root is the lowest is pinned at the small sizes.
    MI355X: E = -94.8941120305 + 0.25, |r|_2 8.2e-06 (bound 1.02e-05), |r|_max 3.7e-07, Rayleigh quotient - E -1.1e-13."""
    norb, na, nb = 13, 1, 6
    h, e, _, ref0, _ = _large_problem(norb, na, nb)
    s = _solver()
    en, ci = s.kernel(h, e, norb, (na, nb), nroots=1, ecore=0.25)
    assert s.converged and np.isscalar(en) and ci.shape == (13, 1716) and abs(np.linalg.norm(ci) - 1.0) <= 1e-12
    sig = ref_sigma(h, e, norb, (na, nb), ci)
    r = sig - (en - 0.25) * ci
    bound = s.conv_tol ** 0.5 + np.sqrt(ci.size) * 1e-11 * max(1.0, np.abs(ref0).max())
    ray = np.sum(ci * sig) + 0.25 - en
    print(f"(13,1,6): E = {en:.10f}, |H_ref c - E c|_2 {np.linalg.norm(r):.2e} (bound {bound:.2e}), max {np.abs(r).max():.2e}, "
          f"Rayleigh quotient - E {ray:.2e}")
    assert np.abs(r).max() <= np.linalg.norm(r) <= bound and abs(ray) <= 1e-9


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
