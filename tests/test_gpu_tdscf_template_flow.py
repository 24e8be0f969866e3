"""The UV template's flow (perform_ground_state -> perform_tddft -> analyze_excitations) through the drop-in names:
`gpu4pyscf.dft.RKS(mol).to_gpu()`, `tdscf.TDDFT(mf)`, `td.nstates`, `td.kernel()`, `td.analyze()`,
`td.oscillator_strength()`, `td.xy[n]`; B3LYP/6-31G*, 10 states."""
import io

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _flow(smiles):
    import gpu4pyscf
    from pyscf import gto, tdscf
    from mi355scf import smiles_fixtures
    sym, xyz = smiles_fixtures.lookup(smiles)
    mol = gto.Mole()
    mol.atom = [(s, tuple(x)) for s, x in zip(sym, xyz)]
    mol.basis = "6-31G*"
    mol.unit = "Angstrom"
    mol.verbose = 0
    mol.build()
    mf = gpu4pyscf.dft.RKS(mol).to_gpu()
    mf.xc = "B3LYP"
    mf.kernel()
    assert mf.converged
    td = tdscf.TDDFT(mf)
    td.nstates = 10
    e, xy = td.kernel()
    td.stdout = io.StringIO()
    td.verbose = 4
    td.analyze()
    log = td.stdout.getvalue()
    assert log.count("Excited State") == 10 and " eV " in log and " nm " in log and "f=" in log and " -> " in log
    f = td.oscillator_strength()
    x, y = td.xy[0]
    nocc = td._scf.mol.nelectron // 2
    assert x.shape == (nocc, mol.nao - nocc) and y.shape == x.shape
    return mol, td, np.asarray(e), np.asarray(f)


def test_benzoquinone_uv_flow():
    mol, td, e, f = _flow("O=C1C=CC(=O)C=C1")
    assert mol.nao == 120 and mol.nelectron == 56 and mol.natm == 12
    assert len(e) == 10 and td.converged.all()
    assert np.all(e > 0) and np.all(np.diff(e) >= 0) and np.all(f >= 0)


def test_benzene_uv_flow_symmetry():
    mol, td, e, f = _flow("c1ccccc1")
    assert len(e) == 10 and td.converged.all()
    assert np.all(e > 0) and np.all(np.diff(e) >= 0) and np.all(f >= 0)
    assert f[0] < 1e-4                      # S1 (B2u) is dark
    bright = int(np.argmax(f))              # E1u: a degenerate pair carries the intensity
    k = bright + 1 if bright + 1 < len(e) and abs(e[bright + 1] - e[bright]) < abs(e[bright] - e[bright - 1]) else bright - 1
    assert abs(e[k] - e[bright]) < 2e-5
    assert abs(f[k] - f[bright]) <= 1e-3 * f[bright]
