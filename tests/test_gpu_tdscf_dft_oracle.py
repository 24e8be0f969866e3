"""TD-DFT against an independent reference: dense A, B from the oracle's McMurchie-Davidson ERI tensor plus an XC kernel
from central differences of the oracle's XC potential (its own functional code with complex-step first derivatives,
`oracle.dft.eval_xc`) on the engine's pruned product grid, in the engine's orbitals."""
import numpy as np
import pytest

from conftest import MOLECULES

pytestmark = pytest.mark.gpu
_MF = {}


def _oracle_vxc(ao, w, terms, dm, rho_cut=1e-10):
    """The oracle's closed-shell XC matrix (oracle.dft.nr_rks, with the AO values evaluated once)."""
    from oracle import dft as odft
    c0 = ao[0] @ dm
    rho = np.einsum("gi,gi->g", ao[0], c0)
    grad = np.array([2 * np.einsum("gi,gi->g", ao[1 + k], c0) for k in range(3)])
    sigma = (grad * grad).sum(axis=0)
    ok = rho > rho_cut
    _, vr, vs = odft.eval_xc(terms, np.where(ok, rho, 1.0), np.where(ok, sigma, 0.0))
    vr, vs = np.where(ok, vr, 0), np.where(ok, vs, 0)
    aow = ao[0] * (0.5 * w * vr)[:, None]
    for k in range(3):
        aow += ao[1 + k] * (2 * w * vs * grad[k])[:, None]
    v = ao[0].T @ aow
    return v + v.T


def _setup(xc):
    if xc not in _MF:
        from pyscf import gto, dft
        from oracle import oracle as orc, dft as odft
        mol = gto.M(atom=MOLECULES["h2o"], basis="6-31g(d)", verbose=0)
        mf = dft.RKS(mol)
        mf.xc = xc
        mf.conv_tol = 1e-11
        mf.kernel()
        coords = mf.grids.coords.cpu().numpy()
        w = mf.grids.weights.cpu().numpy()
        ao = odft.eval_ao(mol, coords, 1)
        hyb, terms = odft.parse_xc(xc)
        _MF[xc] = (mol, mf, orc.Oracle(mol).eri_full(), ao, w, terms, hyb)
    return _MF[xc]


def _oracle_dvxc(ao, w, terms, D0, M, h=1e-4):
    s = h / np.abs(M).max()
    return (_oracle_vxc(ao, w, terms, D0 + s * M) - _oracle_vxc(ao, w, terms, D0 - s * M)) / (2 * s)


@pytest.mark.parametrize("xc", ["B3LYP", "PBE", "BLYP", "SVWN", "PBE0"])
def test_dvxc_matches_oracle_differences(xc):
    import torch
    from pyscf import tdscf
    mol, mf, _, ao, w, terms, _ = _setup(xc)
    td = tdscf.TDA(mf)
    td._setup()
    D0 = np.asarray(mf.make_rdm1())
    rng = np.random.default_rng(7)
    a = rng.standard_normal((2, mol.nao, mol.nao)) * 0.1
    Ms = 0.5 * (a + a.transpose(0, 2, 1))
    got = td._dvxc(torch.as_tensor(Ms, device=td._de.device)).cpu().numpy()
    for m in range(2):
        ref = _oracle_dvxc(ao, w, terms, D0, Ms[m])
        assert np.abs(got[m] - ref).max() <= 1e-6 * np.abs(ref).max(), (xc, np.abs(got[m] - ref).max())


def _dense_ab(mol, mf, eri, ao, w, terms, hyb):
    C, e = np.asarray(mf.mo_coeff), np.asarray(mf.mo_energy)
    no = int((np.asarray(mf.mo_occ) > 0).sum())
    Co, Cv = C[:, :no], C[:, no:]
    nv = Cv.shape[1]
    n = no * nv
    ovov = np.einsum("pqrs,pi,qa,rj,sb->iajb", eri, Co, Cv, Co, Cv, optimize=True).reshape(n, n)
    oovv = np.einsum("pqrs,pi,qj,ra,sb->ijab", eri, Co, Co, Cv, Cv, optimize=True).transpose(0, 2, 1, 3).reshape(n, n)
    ovvo = np.einsum("pqrs,pi,qa,rj,sb->iajb", eri, Co, Cv, Co, Cv, optimize=True).transpose(0, 3, 2, 1).reshape(n, n)
    # XC kernel: the response of the total-density XC potential to the total density change 2 D_s of a unit amplitude
    D0 = np.asarray(mf.make_rdm1())
    fxc = np.zeros((n, n))
    for j in range(no):
        for b in range(nv):
            Dt = np.outer(Co[:, j], Cv[:, b]) + np.outer(Cv[:, b], Co[:, j])   # 2 D_s
            fxc[:, j * nv + b] = (Co.T @ _oracle_dvxc(ao, w, terms, D0, Dt) @ Cv).reshape(-1)
    de = (e[no:][None, :] - e[:no, None]).reshape(-1)
    A = np.diag(de) + 2 * ovov - hyb * oovv + fxc
    B = 2 * ovov - hyb * ovvo + fxc
    return A, B


@pytest.mark.parametrize("xc", ["B3LYP", "PBE", "SVWN"])
def test_tddft_roots_match_dense_oracle(xc):
    from pyscf import tdscf
    mol, mf, eri, ao, w, terms, hyb = _setup(xc)
    A, B = _dense_ab(mol, mf, eri, ao, w, terms, hyb)
    assert np.abs(A - A.T).max() < 1e-6
    A, B = 0.5 * (A + A.T), 0.5 * (B + B.T)
    ns = 5
    td = tdscf.TDA(mf)
    td.nstates, td.conv_tol = ns, 1e-11
    e, _ = td.kernel()
    assert td.converged.all()
    assert np.abs(e - np.linalg.eigvalsh(A)[:ns]).max() < 1e-6, (e, np.linalg.eigvalsh(A)[:ns])
    rp = tdscf.TDDFT(mf)
    rp.nstates, rp.conv_tol = ns, 1e-11
    e2, xy = rp.kernel()
    w2 = np.linalg.eigvals((A - B) @ (A + B))
    ref = np.sort(np.sqrt(w2.real))[:ns]
    assert rp.converged.all()
    assert np.abs(e2 - ref).max() < 1e-6, (e2, ref)
    for x, y in xy:
        assert abs((x * x).sum() - (y * y).sum() - 0.5) < 1e-9


def test_batched_and_looped_jk_give_the_same_roots(monkeypatch):
    """PBE needs only J of symmetric densities, which both builds provide: the roots agree to 1e-9."""
    from pyscf import tdscf
    from mi355scf import tdscf as mtd
    _, mf, *_ = _setup("PBE")
    out = []
    for lim in (0, 10 ** 9):
        monkeypatch.setattr(mtd, "JK_MULTI_MIN", lim)
        td = tdscf.TDDFT(mf)
        td.nstates, td.conv_tol = 5, 1e-11
        out.append(td.kernel()[0])
    assert np.abs(out[0] - out[1]).max() < 1e-9
