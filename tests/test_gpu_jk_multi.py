"""mi_build_jk_multi: J/K of batches of symmetric and antisymmetric densities in one pass over the resident tiles, against
dense einsum on the oracle's McMurchie-Davidson tensor, against the looped single-density build, and through
`SCF.get_jk(hermi=0)`."""
import numpy as np
import pytest
import torch

from conftest import MOLECULES

pytestmark = pytest.mark.gpu
_CASES = {}


def _case(name, basis):
    key = (name, basis)
    if key not in _CASES:
        from mi355scf.engine import Engine
        from mi355scf.mole import Mole
        from oracle import oracle as orc
        mol = Mole(atom=MOLECULES[name], basis=basis, verbose=0).build()
        eng = Engine(mol)
        eng.prepare_eri(1e-13)
        _CASES[key] = (mol, eng, orc.Oracle(mol).eri_full())
    return _CASES[key]


def _densities(n, nao, kinds, seed):
    rng = np.random.default_rng(seed)
    D, sym = [], []
    for m in range(n):
        a = rng.standard_normal((nao, nao))
        s = kinds[m % len(kinds)]
        D.append(0.5 * (a + a.T) if s > 0 else 0.5 * (a - a.T))
        sym.append(s)
    return np.array(D), sym


@pytest.mark.parametrize("name,basis", [("h2o", "cc-pvdz"), ("h2co", "6-31g(d)"), ("h2o", "6-31g(d)")])
@pytest.mark.parametrize("n,kinds", [(1, [1]), (1, [-1]), (3, [1, -1]), (16, [1, -1, -1]), (19, [-1, 1])])
def test_jk_multi_matches_dense(name, basis, n, kinds):
    mol, eng, eri = _case(name, basis)
    D, sym = _densities(n, mol.nao, kinds, seed=n * 7 + len(kinds))
    J, K = eng.get_jk_multi(torch.as_tensor(D, device=eng.device), sym)
    J, K = J.cpu().numpy(), K.cpu().numpy()
    Jr = np.einsum("ijkl,mkl->mij", eri, D)
    Kr = np.einsum("ijkl,mjl->mik", eri, D)
    scale = max(1.0, np.abs(Kr).max())
    assert np.abs(K - Kr).max() < 1e-10 * scale, np.abs(K - Kr).max()
    for m in range(n):
        if sym[m] > 0:
            assert np.abs(J[m] - Jr[m]).max() < 1e-10 * scale
        else:
            assert np.abs(J[m]).max() == 0.0 and np.abs(Jr[m]).max() < 1e-10 * scale


@pytest.mark.parametrize("basis", ["cc-pvdz", "cc-pvtz"])
def test_jk_multi_equals_looped_build_benzene(basis):
    from mi355scf.engine import Engine
    from mi355scf.mole import Mole
    from mi355scf import smiles_fixtures
    sym_, xyz = smiles_fixtures.lookup("c1ccccc1")
    mol = Mole(atom=[(s, tuple(x)) for s, x in zip(sym_, xyz)], basis=basis, verbose=0).build()
    eng = Engine(mol)
    eng.prepare_eri(1e-13)
    D, sym = _densities(8, mol.nao, [1], seed=5)
    Dt = torch.as_tensor(D, device=eng.device)
    J, K = eng.get_jk_multi(Dt, sym)
    for m in range(8):
        j, k = eng.get_jk(Dt[m])
        assert (J[m] - j).abs().max().item() <= 1e-12 * j.abs().max().item()
        assert (K[m] - k).abs().max().item() <= 1e-12 * k.abs().max().item()
    del eng


def test_get_jk_hermi0_nonsymmetric():
    from pyscf import gto, scf
    from oracle import oracle as orc
    mol = gto.M(atom=MOLECULES["h2o"], basis="6-31g(d)", verbose=0)
    mf = scf.RHF(mol)
    rng = np.random.default_rng(11)
    dm = rng.standard_normal((mol.nao, mol.nao))
    J, K = mf.get_jk(mol, dm, hermi=0)
    eri = orc.Oracle(mol).eri_full()
    assert np.abs(J - np.einsum("ijkl,kl->ij", eri, dm)).max() < 1e-10
    assert np.abs(K - np.einsum("ijkl,jl->ik", eri, dm)).max() < 1e-10
    dms = np.array([dm, dm.T, 0.5 * (dm + dm.T)])
    J3, K3 = mf.get_jk(mol, dms, hermi=0)
    assert np.abs(K3 - np.einsum("ijkl,mjl->mik", eri, dms)).max() < 1e-10
    assert np.abs(J3 - np.einsum("ijkl,mkl->mij", eri, dms)).max() < 1e-10


def test_jk_multi_j_only():
    mol, eng, eri = _case("h2o", "6-31g(d)")
    D, sym = _densities(5, mol.nao, [1, -1], seed=3)
    J, K = eng.get_jk_multi(torch.as_tensor(D, device=eng.device), sym, with_k=False)
    assert K is None
    Jr = np.einsum("ijkl,mkl->mij", eri, D)
    Jr[np.array(sym) < 0] = 0.0
    assert np.abs(J.cpu().numpy() - Jr).max() < 1e-10 * max(1.0, np.abs(Jr).max())


def test_get_jk_hermi0_density_fitted():
    """Density fitting: hermi=0 goes through the dense fitted route, which is exact for any density of the fitted model."""
    from pyscf import gto, scf
    from oracle import oracle as orc
    mol = gto.M(atom=MOLECULES["h2o"], basis="6-31g(d)", verbose=0)
    mf = scf.RHF(mol).density_fit()
    mf.kernel()
    rng = np.random.default_rng(13)
    dm = rng.standard_normal((mol.nao, mol.nao)) * 0.1
    ds = 0.5 * (dm + dm.T)
    J, K = mf.get_jk(mol, dm, hermi=0)
    Jt, Kt = mf.get_jk(mol, dm.T, hermi=0)
    Js, Ks = mf.get_jk(mol, ds, hermi=1)
    assert np.abs(Kt - K.T).max() < 1e-10 and np.abs(J - Js).max() < 1e-10
    assert np.abs(0.5 * (K + Kt) - Ks).max() < 1e-10
    eri = orc.Oracle(mol).eri_full()
    assert np.abs(K - np.einsum("ijkl,jl->ik", eri, dm)).max() < 1e-2     # fitting error only
