"""Closed-shell TDA / TDHF / TDDFT on the device against dense A, B built from the oracle's ERI tensor in the same orbitals."""
import numpy as np
import pytest

from conftest import MOLECULES

pytestmark = pytest.mark.gpu
_MF = {}


def _rhf(name):
    if name not in _MF:
        from pyscf import gto, scf
        from oracle import oracle as orc
        mol = gto.M(atom=MOLECULES[name], basis="6-31g(d)", verbose=0)
        mf = scf.RHF(mol)
        mf.conv_tol = 1e-11
        mf.kernel()
        _MF[name] = (mf, orc.Oracle(mol).eri_full())
    return _MF[name]


def _dense_ab(mf, eri, singlet, cx=1.0):
    C, e = np.asarray(mf.mo_coeff), np.asarray(mf.mo_energy)
    no = int((np.asarray(mf.mo_occ) > 0).sum())
    Co, Cv = C[:, :no], C[:, no:]
    nv = Cv.shape[1]
    ovov = np.einsum("pqrs,pi,qa,rj,sb->iajb", eri, Co, Cv, Co, Cv, optimize=True)
    oovv = np.einsum("pqrs,pi,qj,ra,sb->ijab", eri, Co, Co, Cv, Cv, optimize=True)
    de = (e[no:][None, :] - e[:no, None]).reshape(-1)
    n = no * nv
    A = np.diag(de) - cx * oovv.transpose(0, 2, 1, 3).reshape(n, n)
    B = -cx * ovov.transpose(0, 3, 2, 1).reshape(n, n)
    if singlet:
        A += 2.0 * ovov.reshape(n, n)
        B += 2.0 * ovov.reshape(n, n)
    dip = mf.engine.int1e(with_dipole=True)[3].cpu().numpy()
    return A, B, np.einsum("xpq,pi,qa->xia", dip, Co, Cv)


@pytest.mark.parametrize("name", ["h2o", "h2co"])
@pytest.mark.parametrize("singlet", [True, False])
def test_cis_and_tdhf_match_dense(name, singlet):
    from pyscf import tdscf
    from mi355scf.tdscf import oscillator_strengths
    mf, eri = _rhf(name)
    A, B, dip_ov = _dense_ab(mf, eri, singlet)
    ns = 6
    td = tdscf.TDA(mf)
    td.singlet, td.nstates, td.conv_tol = singlet, ns, 1e-12
    e, xy = td.kernel()
    assert td.converged.all()
    assert np.abs(e - np.linalg.eigvalsh(A)[:ns]).max() < 1e-8
    for x, y in xy:
        assert abs((x * x).sum() - 0.5) < 1e-10 and np.all(y == 0)

    td = tdscf.TDHF(mf)
    td.singlet, td.nstates, td.conv_tol = singlet, ns, 1e-12
    e, xy = td.kernel()
    w2, Z = np.linalg.eig((A - B) @ (A + B))
    ref = np.sort(np.sqrt(w2.real))[:ns]
    assert td.converged.all()
    assert np.abs(e - ref).max() < 1e-8
    for x, y in xy:
        assert abs((x * x).sum() - (y * y).sum() - 0.5) < 1e-10
    f = td.oscillator_strength()
    if not singlet:
        assert np.all(f == 0)
        return
    # dense reference of f from the eigenvectors of the full problem
    big = np.block([[A, B], [-B, -A]])
    ev, vec = np.linalg.eig(big)
    order = np.argsort(np.where(ev.real > 0, ev.real, np.inf))[:ns]
    n = A.shape[0]
    xy_ref = []
    for k in order:
        v = vec[:, k].real
        x, y = v[:n], v[n:]
        s = np.sqrt(0.5 / (x @ x - y @ y))
        xy_ref.append(((x * s).reshape(dip_ov.shape[1:]), (y * s).reshape(dip_ov.shape[1:])))
    fr = oscillator_strengths(ev.real[order], xy_ref, dip_ov)
    # degenerate roots may mix: compare sums over (near-)degenerate groups
    assert abs(f.sum() - fr.sum()) < 1e-6
    assert np.abs(np.sort(f) - np.sort(fr)).max() < 1e-6 or np.allclose(ev.real[order][1:], ev.real[order][:-1], atol=1e-6)


def test_triplet_below_singlet():
    from pyscf import tdscf
    mf, _ = _rhf("h2co")
    es = tdscf.TDHF(mf).kernel(nstates=3)[0]
    t = tdscf.TDHF(mf)
    t.singlet = False
    et = t.kernel(nstates=3)[0]
    assert et[0] < es[0]


@pytest.mark.parametrize("xc", ["B3LYP", "PBE", "SVWN"])
def test_tddft_solver_matches_its_dense_operator(xc):
    """TD-DFT roots (TDA and RPA) equal the eigenvalues of the dense operator assembled column by column from the same
    products (J/K through the batched kernel, XC response through the SCF's quadrature)."""
    import torch
    from pyscf import gto, dft, tdscf
    mol = gto.M(atom=MOLECULES["h2o"], basis="6-31g(d)", verbose=0)
    mf = dft.RKS(mol)
    mf.xc = xc
    mf.conv_tol = 1e-11
    mf.kernel()
    ns = 4
    td = tdscf.TDA(mf)
    td.nstates, td.conv_tol = ns, 1e-11
    e, _ = td.kernel()
    n = td._nocc * td._nvir
    I = torch.eye(n, dtype=torch.float64, device=td._de.device)
    A = td._tda_matvec(I).cpu().numpy()
    assert np.abs(A - A.T).max() < 1e-7
    assert np.abs(e - np.linalg.eigvalsh(0.5 * (A + A.T))[:ns]).max() < 1e-6
    rp = tdscf.TDDFT(mf)
    rp.nstates, rp.conv_tol = ns, 1e-11
    e2, xy = rp.kernel()
    P, M = (t.cpu().numpy() for t in rp._rpa_products(I))
    w2 = np.linalg.eigvals((0.5 * (M + M.T)) @ (0.5 * (P + P.T)))
    assert np.abs(e2 - np.sort(np.sqrt(w2.real))[:ns]).max() < 1e-6
    for x, y in xy:
        assert abs((x * x).sum() - (y * y).sum() - 0.5) < 1e-9
    assert np.all(e2 <= e + 1e-9)   # RPA roots lie below the TDA ones


def test_uks_and_meta_gga_refused():
    from pyscf import gto, dft, scf, tdscf
    mol = gto.M(atom="O 0 0 0; H 0 0 0.97", basis="6-31g(d)", spin=1, verbose=0)
    with pytest.raises(NotImplementedError):
        tdscf.TDDFT(scf.UHF(mol))
    mol2 = gto.M(atom=MOLECULES["h2o"], basis="6-31g(d)", verbose=0)
    mf = dft.RKS(mol2)
    mf.xc = "TPSS"
    with pytest.raises(NotImplementedError):
        tdscf.TDDFT(mf)


def test_tdhf_from_oracle_orbitals():
    """End to end from the oracle's own RHF orbitals: TDHF roots agree with those from the engine's SCF to 1e-6 Ha."""
    from pyscf import gto, scf, tdscf
    from oracle import oracle as orc
    mf, _ = _rhf("h2o")
    ref = tdscf.TDHF(mf)
    ref.nstates, ref.conv_tol = 5, 1e-11
    e_ref = ref.kernel()[0]
    mol = gto.M(atom=MOLECULES["h2o"], basis="6-31g(d)", verbose=0)
    r = orc.rhf(mol, conv_tol=1e-11)
    mf2 = scf.RHF(mol)
    mf2.mo_coeff, mf2.mo_energy, mf2.mo_occ = r["mo_coeff"], r["mo_energy"], r["mo_occ"]
    td = tdscf.TDHF(mf2)
    td.nstates, td.conv_tol = 5, 1e-11
    e = td.kernel()[0]
    assert np.abs(e - e_ref).max() < 1e-6
