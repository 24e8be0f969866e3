"""The active-pair Coulomb kernel (`mi_eri_active_j` / `Engine.active_pair_j`):
    Jp[vw, p, q] = sum_rs (pq|rs) Ca[r, v] Ca[s, w],  v >= w packed as v (v + 1) / 2 + w
against dense contractions of the CPU oracle's tensor, tolerance 1e-10 max(1, |ref|max) (the margin of test_gpu_jk_multi.py), and
exact (p, q) symmetry.  `Ca` is seeded random with non-orthogonal columns.  Pair counts: ncas = 1, 2, 5, 16 and the pass
boundaries -- the kernel finishes W = `Engine.active_pair_width()` = 32 pairs per pass in two 16-wide column blocks; pair counts
are triangular numbers, so 32 and 33 themselves do not occur: ncas = 5 / 6 (15 / 21 pairs) straddle the one-block / two-block
switch, ncas = 7 (28) is the last single pass and ncas = 8 (36 = W + 4) the first to need a second one; ncas = 16 (136) takes five."""
import functools

import numpy as np
import pytest

from conftest import MOLECULES

pytestmark = pytest.mark.gpu

NCAS = (1, 2, 5, 6, 7, 8, 16)
STORE_OPTS = [("default", {}), ("nt2", {"jk_nt": 2}), ("ao_order0", {"ao_order": 0}), ("tri0", {"tri_tiles": 0})]


@functools.lru_cache(maxsize=None)
def _mol(name, basis):
    from mi355scf.mole import Mole
    return Mole(atom=MOLECULES[name], basis=basis, verbose=0).build()


@functools.lru_cache(maxsize=None)
def _eri(name, basis):
    from oracle import oracle as orc
    e = orc.Oracle(_mol(name, basis)).eri_full()
    e.setflags(write=False)
    return e


def _reference(eri, Ca):
    full = np.einsum("pqrs,rv,sw->vwpq", eri, Ca, Ca, optimize=True)
    v, w = np.tril_indices(Ca.shape[1])
    return full[v, w]


def _check(eng, eri, nao, ncas_list, seed, tag):
    rng = np.random.default_rng(seed)
    for ncas in ncas_list:
        Ca = rng.standard_normal((nao, ncas))
        ref = _reference(eri, Ca)
        Jp = eng.active_pair_j(Ca).cpu().numpy()
        assert Jp.shape == (ncas * (ncas + 1) // 2, nao, nao)
        scale = max(1.0, np.abs(ref).max())
        err = np.abs(Jp - ref).max()
        print(f"{tag} ncas={ncas} ({Jp.shape[0]} pairs): max|Jp - ref| = {err:.3e} (scale {scale:.2f})")
        assert err < 1e-10 * scale, (ncas, err)
        assert np.array_equal(Jp, Jp.transpose(0, 2, 1))


@pytest.mark.parametrize("name,basis,nao", [("h2o", "sto-3g", 7), ("h2co", "6-31g(d)", 32)])
def test_active_pair_j_matches_oracle(name, basis, nao):
    """N = 7: a single ragged tile; N = 32: several tiles (the padded leading dimension leaves a ragged last block)."""
    from mi355scf.engine import Engine
    mol = _mol(name, basis)
    assert mol.nao == nao
    assert Engine.active_pair_width() == 32
    eng = Engine(mol)
    eng.prepare_eri(1e-13)
    _check(eng, _eri(name, basis), nao, NCAS, 500 + nao, f"{name}/{basis}")
    eng.close()


@pytest.mark.parametrize("oid,opts", STORE_OPTS[1:], ids=[o[0] for o in STORE_OPTS[1:]])
def test_active_pair_j_under_store_options(oid, opts):
    """The resident store layouts test_gpu_jk_variants.py switches between for the batched J/K (nontemporal stream, caller's AO
    order, full block-diagonal tiles), same option names; h2co/6-31g(d) and the ragged N = 18 of h2o/6-31g(d)."""
    from mi355scf.engine import Engine
    for name, basis in (("h2co", "6-31g(d)"), ("h2o", "6-31g(d)")):
        mol = _mol(name, basis)
        eng = Engine(mol)
        for k, v in opts.items():
            eng.set_option(k, v)
        eng.prepare_eri(1e-13)
        _check(eng, _eri(name, basis), mol.nao, (2, 6, 8), 900 + mol.nao, f"{name}/{basis} {oid}")
        eng.close()


def test_active_pair_j_equals_j_only_batched_build_benzene():
    """benzene/sto-3g: the same operators from materialised pair densities through `get_jk_multi(..., with_k=False)`."""
    import torch
    from mi355scf import smiles_fixtures
    from mi355scf.engine import Engine
    from mi355scf.mole import Mole
    sym_, xyz = smiles_fixtures.lookup("c1ccccc1")
    mol = Mole(atom=[(s, tuple(x)) for s, x in zip(sym_, xyz)], basis="sto-3g", verbose=0).build()
    eng = Engine(mol)
    eng.prepare_eri(1e-13)
    rng = np.random.default_rng(66)
    for ncas in (6, 8):
        Ca = rng.standard_normal((mol.nao, ncas))
        v, w = np.tril_indices(ncas)
        D = 0.5 * (np.einsum("rm,sm->mrs", Ca[:, v], Ca[:, w]) + np.einsum("sm,rm->mrs", Ca[:, v], Ca[:, w]))
        J, _ = eng.get_jk_multi(torch.as_tensor(D, device=eng.device), [1] * len(v), with_k=False)
        Jp = eng.active_pair_j(Ca)
        rel = float((Jp - J).abs().max() / J.abs().max())
        print(f"benzene/sto-3g ncas={ncas}: max|Jp - J| / max|J| = {rel:.3e}")
        assert rel <= 1e-12
    eng.close()


def test_active_pair_j_refusals():
    """A sharded store and an unprepared context are errors of the library, not faults; bad shapes are refused in Python."""
    import ctypes
    import torch
    from mi355scf import engine
    from mi355scf.engine import Engine, EngineError
    mol = _mol("h2o", "sto-3g")
    eng = Engine(mol)
    eng.prepare_eri(1e-13, rank=0, nranks=2)                 # a sharded store
    with pytest.raises(EngineError):
        eng.active_pair_j(np.ones((mol.nao, 2)))
    eng.close()
    eng = Engine(mol)                                        # never prepared: the C entry itself refuses
    Ca = torch.ones((mol.nao, 2), dtype=torch.float64, device=eng.device)
    out = torch.zeros((3, mol.nao, mol.nao), dtype=torch.float64, device=eng.device)
    rc = engine.lib().mi_eri_active_j(eng._h, Ca.data_ptr(), 2, 2, out.data_ptr(), None)
    assert rc != 0 and float(out.abs().max()) == 0.0
    for bad in (0, 17):
        assert engine.lib().mi_eri_active_j(eng._h, Ca.data_ptr(), bad, 17, out.data_ptr(), None) != 0
    with pytest.raises(ValueError):
        eng.active_pair_j(np.ones((mol.nao, 17)))
    with pytest.raises(ValueError):
        eng.active_pair_j(np.ones((mol.nao + 1, 2)))
    eng.close()
