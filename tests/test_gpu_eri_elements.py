"""Element-wise pins of rows a3/a4: the resident tiles against the oracle's McMurchie-Davidson integrals,
integral by integral -- not only through J/K contractions -- and the Schwarz factors against the oracle's.
  * H2O/cc-pVTZ: the whole tensor (`mi_eri_unpack` vs `orc_eri_full`, 58^4 elements, s..f shells);
  * ibuprofen/def2-TZVP (BASELINE config 5, 105 GB resident) and C60/6-31G* shard 0 of 8 (config 4, 63 GB): seeded random
    shell quartets read back with `mi_eri_read_quartet`, stratified over the angular classes incl. (ff|ff) / (dd|dd).
Tolerance 1e-10 absolute (FP64; integrals are O(1e-3 .. 1)).
The plain Coulomb store is also evaluated under every option that selects another evaluation route, launch shape or layout
(`test_coulomb_store_under_evaluation_options*`): whole tensor and Schwarz table again, same bounds."""
import numpy as np
import pytest

from conftest import MOLECULES

pytestmark = pytest.mark.gpu


def _fixture_mol(smiles, basis):
    from mi355scf import smiles_fixtures
    from mi355scf.mole import Mole
    sym, xyz = smiles_fixtures.TABLE[smiles]()
    return Mole(atom="; ".join(f"{s} {x:.6f} {y:.6f} {z:.6f}" for s, (x, y, z) in zip(sym, xyz)), basis=basis, verbose=0).build()


def test_full_tensor_and_schwarz_h2o_ccpvtz():
    from mi355scf.engine import Engine
    from mi355scf.mole import Mole
    from oracle import oracle as orc
    mol = Mole(atom=MOLECULES["h2o"], basis="cc-pvtz", verbose=0).build()
    eng = Engine(mol)
    eng.prepare_eri(1e-13)
    o = orc.Oracle(mol)
    ref = o.eri_full()
    got = eng.eri_dense().cpu().numpy()
    assert np.abs(got - ref).max() < 1e-10, np.abs(got - ref).max()
    q, qo = eng.schwarz(), o.schwarz()
    kept = q > 0
    assert kept.sum() > 0.9 * q.size
    assert np.abs(q - qo)[kept].max() < 1e-11
    assert (qo[~kept] * qo.max() < 1e-13).all()          # dropped pairs really are negligible
    # a shell block read back through the debug ABI equals the same block of the dense tensor
    loc = mol.ao_loc_nr()
    for sh in ((mol.nbas - 1, 3, 7, 0), (5, 5, 5, 5), (2, 9, 11, 11)):
        blk = eng.eri_read_quartet(*sh)
        sl = tuple(slice(loc[s_], loc[s_ + 1]) for s_ in sh)
        assert np.abs(blk - ref[sl]).max() < 1e-10


_DENSE = {}


def _dense_ref(name, basis):
    """(mol, oracle tensor, oracle Schwarz table), once per module."""
    if (name, basis) not in _DENSE:
        from mi355scf.mole import Mole
        from oracle import oracle as orc
        mol = Mole(atom=MOLECULES[name], basis=basis, verbose=0).build()
        o = orc.Oracle(mol)
        _DENSE[(name, basis)] = (mol, o.eri_full(), o.schwarz())
    return _DENSE[(name, basis)]


def _check_store(name, basis, opts):
    from mi355scf.engine import Engine
    mol, ref, qo = _dense_ref(name, basis)
    eng = Engine(mol)
    for k, v in opts.items():
        eng.set_option(k, v)
    st = eng.prepare_eri(1e-13)                 # every option of this file takes effect here at the latest
    got = eng.eri_dense().cpu().numpy()
    err = np.abs(got - ref).max()
    q = eng.schwarz()
    kept = q > 0
    qerr = np.abs(q - qo)[kept].max()
    print(f"{name}/{basis} {opts}: max|eri - oracle| = {err:.3e}, max|q - oracle| = {qerr:.3e}, {st['n_quartets']} quartets")
    assert got.shape == ref.shape and np.isfinite(got).all()
    assert err < 1e-10, err
    assert kept.sum() > 0.9 * q.size
    assert qerr < 1e-11
    assert (qo[~kept] * qo.max() < 1e-13).all()
    eng.close()
    return st


# `work_mb` below 8 is taken as 8 (MiB; the hand-over buffer never has fewer than 2^20 doubles).  On these two molecules every
# class pair hands over fewer doubles than that, so the smallest setting runs ONE chunk per class pair and the store does not
# report chunk counts; the several-chunk fill is pinned on benzene/cc-pVTZ at this setting (tests/test_gpu_jk_variants.py), where
# the (pp|pp) class alone needs more than four fills.
EVAL_OPTIONS = [
    {"eri_tpq": 0},
    {"eri_tpq": 1, "tpq_maxprim": 1e9},
    {"eri_fused": 1},
    {"eri_fused": 1, "eri_tpq": 0},
    {"prim_lds": 1},
    {"task_table": 0},
    {"rys_fine": 0},
    {"xcd_map": 0},
    {"rys_qpw_maxcomp": 0},
    {"rys_qpw_maxcomp": 10 ** 9, "rys_qpw_maxprim": 1e9},      # four quartets per wave wherever that kernel form exists
    {"xf_qpw_max": 0},
    {"xf_qpw_max": 10 ** 9},
    {"xf_mlds": 64},
    {"xf_mfma_min": 0},
    {"xf_mfma_min": 10 ** 9},
    {"work_mb": 1},
    {"ao_order": 0},
    {"ket_cluster": 0},
    {"tri_tiles": 0},
    {"ao_order": 0, "ket_cluster": 0, "tri_tiles": 0},
]


@pytest.mark.parametrize("opts", EVAL_OPTIONS, ids=lambda o: ",".join(f"{k}={v:g}" for k, v in o.items()))
def test_coulomb_store_under_evaluation_options_h2o_ccpvtz(opts):
    """H2O/cc-pVTZ (N = 58, s..f shells, contracted s and p): all 58^4 elements and the Schwarz table per option set."""
    st = _check_store("h2o", "cc-pvtz", opts)
    assert st["n_tiles"] > 0


@pytest.mark.parametrize("opts", [{"eri_fused": 1}, {"eri_fused": 1, "eri_tpq": 0}, {"work_mb": 1}, {"eri_tpq": 0, "work_mb": 1}],
                         ids=lambda o: ",".join(f"{k}={v:g}" for k, v in o.items()))
def test_coulomb_store_under_evaluation_options_h2co_631gd(opts):
    """H2CO/6-31G(d) (N = 32: no ragged block, d shells, no f)."""
    _check_store("h2co", "6-31g(d)", opts)


def _sample_quartets(mol, n, seed, classes):
    """Seeded shell quartets: `classes` (tuples of four l) first, then uniformly random ones."""
    rng = np.random.default_rng(seed)
    ls = mol._bas[:, 1]
    by_l = {l: np.where(ls == l)[0] for l in set(ls.tolist())}
    out = []
    for cls in classes:
        for _ in range(n // (4 * len(classes))):
            out.append(tuple(int(rng.choice(by_l[l])) for l in cls))
    while len(out) < n:
        out.append(tuple(int(x) for x in rng.integers(0, mol.nbas, 4)))
    return out


def _compare_sampled(eng, o, quartets, allow_missing):
    nchk = nmiss = nscreened = 0
    worst = 0.0
    for sh in quartets:
        got = eng.eri_read_quartet(*sh)
        if np.isnan(got).any():                 # some of its tiles live on another rank: compare what is here
            assert allow_missing
            nmiss += 1
        ref = o.eri_shell(*sh)
        ok = ~np.isnan(got)
        if not ok.any():
            continue
        zero = ok & (got == 0.0)
        if zero.any():                          # Schwarz-screened tiles: the integrals are below the threshold
            nscreened += 1
            assert np.abs(ref[zero]).max() < 1e-11
        worst = max(worst, np.abs(got - ref)[ok].max())
        nchk += 1
    assert worst < 1e-10, worst
    return nchk, nmiss, nscreened


def test_sampled_quartets_ibuprofen_def2tzvp():
    """BASELINE config 5's tensor (N = 573, 237 shells, 105 GB of resident tiles)."""
    from mi355scf.engine import Engine, release_cache
    from oracle import oracle as orc
    mol = _fixture_mol("CC(C)Cc1ccc(cc1)C(C)C(=O)O", "def2-TZVP")
    assert (mol.nao, mol.nbas) == (573, 237)
    eng = Engine(mol)
    st = eng.prepare_eri(1e-13)
    assert st["stored_bytes"] > 90e9
    classes = [(3, 3, 3, 3), (2, 2, 2, 2), (3, 2, 1, 0), (3, 3, 2, 2), (1, 1, 1, 1), (2, 1, 2, 0), (0, 0, 0, 0), (3, 0, 3, 0)]
    nchk, _nmiss, _nscr = _compare_sampled(eng, orc.Oracle(mol), _sample_quartets(mol, 2000, 11, classes), allow_missing=False)
    assert nchk == 2000
    eng.close()
    release_cache()


def test_sampled_quartets_c60_631gs_shard():
    """BASELINE config 4: rank 0 of 8 of the C60/6-31G* store (N = 840, 360 shells, ~63 GB per rank)."""
    from mi355scf.engine import Engine, release_cache
    from oracle import oracle as orc
    mol = _fixture_mol("C60", "6-31G*")
    assert (mol.nao, mol.nbas) == (840, 360)
    eng = Engine(mol)
    st = eng.prepare_eri(1e-13, rank=0, nranks=8)
    assert 55e9 < st["stored_bytes"] < 72e9
    classes = [(2, 2, 2, 2), (2, 1, 1, 0), (1, 1, 1, 1), (2, 2, 1, 1), (0, 0, 0, 0), (2, 0, 2, 0)]
    nchk, nmiss, _nscr = _compare_sampled(eng, orc.Oracle(mol), _sample_quartets(mol, 2000, 12, classes), allow_missing=True)
    assert nchk > 300 and nmiss > 1000           # about 1/8 of the quartets is resident on this rank
    eng.close()
    release_cache()
