"""Every selectable J/K digestion path against the FP64 CPU oracle, element by element.

`mi_set_option` selects between `jk_tiles_kernel`, `jk_tiles_kjlt_kernel`, `jk_tiles_pipe_kernel` and `jk_tiles_pair_kernel`, the
DPP or ds_bpermute reduce-scatter, the nontemporal stream with its cached prefix, two planners of segments and waves, and three
layouts of the store (`tri_tiles`, `ao_order`, `ket_cluster`).  Each case here sets options, asks `Engine.jk_describe`
(`mi_jk_describe`: the record the launch itself consults) that the intended path is the one that runs, and compares J+K, J-only
and K-only over the whole matrices with
  * `oracle.Oracle(mol).jk(D, tol=0.0)`: 1e-10 absolute (the bound of test_gpu_parity.py), and
  * the default-option build of the same density: 1e-11 (the bound test_gpu_parity.py puts between builds of one density).
Molecules are chosen for block edges (AO blocks of 8): N = 7 is one ragged block, N = 32 has none, N = 34 a last block of 2,
N = 58 is ragged with s..f shells.  Consumers of the same store (`mi_build_jk_multi`, `mi_eri_qtrans`) run under the options they
read, against dense contractions of `Oracle.eri_full()` with the tolerances of test_gpu_jk_multi.py / test_gpu_mp2_stream.py.

The cached-prefix / nontemporal split only exists on stores beyond 256 MiB: benzene/cc-pVTZ (4.9 GB), whole J and K from the
oracle's in-core route (the route and threading of bench.py's CPU leg), bound 1e-9 max(1, |ref|.max()) as test_gpu_configs.py."""
import os
import time

import numpy as np
import pytest

from conftest import MOLECULES

pytestmark = pytest.mark.gpu

CASES = [("h2o", "sto-3g", 7), ("h2co", "6-31g(d)", 32), ("ch4", "cc-pvdz", 34), ("h2o", "cc-pvtz", 58)]
_REF = {}
BUILDS = ((True, True), (True, False), (False, True))          # J+K, J only, K only


def _sym_density(n, seed):
    rng = np.random.default_rng(seed)
    a = rng.normal(size=(n, n))
    return (a + a.T) * 0.5


def _engine(mol, opts):
    from mi355scf.engine import Engine
    eng = Engine(mol)
    for k, v in opts.items():
        eng.set_option(k, v)
    st = eng.prepare_eri(1e-13)
    return eng, st


def _ref(name, basis):
    """(mol, [D0, D1], oracle [(J0, K0), (J1, K1)], default-option [(J0, K0), (J1, K1)], stats of the default store), once."""
    key = (name, basis)
    if key not in _REF:
        from mi355scf.mole import Mole
        from oracle import oracle as orc
        mol = Mole(atom=MOLECULES[name], basis=basis, verbose=0).build()
        D = [_sym_density(mol.nao, 7), _sym_density(mol.nao, 8)]
        o = orc.Oracle(mol)
        ora = [o.jk(d, tol=0.0) for d in D]
        eng, st = _engine(mol, {})
        d = eng.jk_describe()
        assert d["family"] == "plain" and (d["nt"], d["dpp"], d["tri"], d["n_jk_cached"]) == (0, 1, 1, 0), d
        assert d["waves"] == d["segments"] > 0
        dflt = [tuple(x.cpu().numpy() for x in eng.get_jk(dm)) for dm in D]
        eng.close()
        _REF[key] = (mol, D, ora, dflt, st)
    return _REF[key]


def _cmp(tag, got, ora, dflt):
    """Whole matrices, no element left out: oracle at 1e-10, default-option build at 1e-11."""
    got = got.cpu().numpy()
    assert got.shape == ora.shape and np.isfinite(got).all(), tag
    eo, ed = np.abs(got - ora).max(), np.abs(got - dflt).max()
    print(f"{tag}: max|got - oracle| = {eo:.3e}, max|got - default| = {ed:.3e}")
    assert eo < 1e-10, (tag, eo)
    assert ed < 1e-11, (tag, ed)


def _check_single(tag, eng, D, ora, dflt, want):
    """J+K, J-only and K-only of one density; `want(with_j, with_k)` -> fields `jk_describe` must report for that build."""
    for wj, wk in BUILDS:
        d = eng.jk_describe(wj, wk, 1)
        for k, v in want(wj, wk).items():
            assert d[k] == v, (tag, wj, wk, k, d)
        J, K = eng.get_jk(D, with_j=wj, with_k=wk)
        if wj:
            _cmp(f"{tag} J (with_k={int(wk)}) [{d['family']}]", J, ora[0], dflt[0])
        if wk:
            _cmp(f"{tag} K (with_j={int(wj)}) [{d['family']}]", K, ora[1], dflt[1])


def _check_pair(tag, eng, D, ora, dflt, want):
    """n_dm = 2 with two DIFFERENT densities (a swap of the accumulator sets fails), each result against the oracle;
    `want(with_j, with_k)` as in `_check_single`."""
    import torch
    D2 = torch.as_tensor(np.stack(D), device=eng.device)
    for wj, wk in BUILDS:
        d = eng.jk_describe(wj, wk, 2)
        for k, v in want(wj, wk).items():
            assert d[k] == v, (tag, wj, wk, k, d)
        J, K = eng.get_jk(D2, with_j=wj, with_k=wk)
        for m in range(2):
            if wj:
                _cmp(f"{tag} J[{m}] (with_k={int(wk)}) [{d['family']}]", J[m], ora[m][0], dflt[m][0])
            if wk:
                _cmp(f"{tag} K[{m}] (with_j={int(wj)}) [{d['family']}]", K[m], ora[m][1], dflt[m][1])


# ---- kernel family, reduce-scatter and cache policy on the default layout -----------------------------------------------------
KERNEL_VARIANTS = [
    ("dpp0", {"jk_dpp": 0}, "plain", dict(nt=0, dpp=0)),
    ("kjlt", {"jk_kjlt": 1}, "kjlt", dict(nt=0, dpp=1)),
    ("nt2", {"jk_nt": 2}, "plain", dict(nt=1, dpp=1)),
    ("nt0", {"jk_nt": 0}, "plain", dict(nt=0, dpp=1)),
    ("kjlt_nt2", {"jk_kjlt": 1, "jk_nt": 2}, "kjlt", dict(nt=1, dpp=1)),
    ("kjlt_dpp0", {"jk_kjlt": 1, "jk_dpp": 0}, "kjlt", dict(nt=0, dpp=0)),
]


@pytest.mark.parametrize("name,basis,nao", CASES)
@pytest.mark.parametrize("vid,opts,family,fields", KERNEL_VARIANTS, ids=[v[0] for v in KERNEL_VARIANTS])
def test_kernel_variants(name, basis, nao, vid, opts, family, fields):
    mol, D, ora, dflt, _ = _ref(name, basis)
    assert mol.nao == nao
    eng, _ = _engine(mol, opts)

    def want(wj, wk):                         # the KJLT kernel only exists for the J+K build
        return dict(fields, family=family if (family != "kjlt" or (wj and wk)) else "plain", tri=1, n_jk_cached=0)
    _check_single(f"{name}/{basis} {vid}", eng, D[0], ora[0], dflt[0], want)
    eng.close()


# ---- full rows: the half-tile pipeline kernel and the plain kernel on full-row tiles -----------------------------------------------
@pytest.mark.parametrize("name,basis,nao", CASES)
@pytest.mark.parametrize("nt", [1, 2])
@pytest.mark.parametrize("pipe", [-1, 0, 1])
def test_full_rows_pipeline_and_plain(name, basis, nao, pipe, nt):
    """`tri_tiles = 0`.  The stores here are cache-resident (< 256 MiB), so `jk_pipe = -1` selects the pipeline like 1 does; a
    build without K has no pipeline form and must fall back to the plain kernel.  The pipeline kernel has the ds_bpermute
    reduce-scatter only, and its K-only form only the nontemporal stream: the accessor says so."""
    mol, D, ora, dflt, _ = _ref(name, basis)
    eng, st = _engine(mol, {"tri_tiles": 0, "jk_pipe": pipe, "jk_nt": nt})
    assert st["stored_bytes"] < 256 << 20

    def want(wj, wk):
        if pipe != 0 and wk:
            return dict(family="pipe", tri=0, dpp=0, nt=1 if (nt == 2 or not wj) else 0)
        return dict(family="plain", tri=0, dpp=1, nt=1 if nt == 2 else 0)
    _check_single(f"{name}/{basis} tri0 pipe={pipe} nt={nt}", eng, D[0], ora[0], dflt[0], want)
    eng.close()


# ---- the two planners of segments and waves -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,basis,nao", CASES)
@pytest.mark.parametrize("waves", [1, 3, 64, 10 ** 6])
def test_fixed_wave_planner(name, basis, nao, waves):
    """`jk_waves = N > 0`: N waves with equal-cost contiguous shares.  1 and 3 give several segments per wave, 64 leaves waves
    with empty shares on the small stores, 10**6 exceeds the number of tiles and is clamped to it."""
    mol, D, ora, dflt, st0 = _ref(name, basis)
    eng, st = _engine(mol, {"jk_waves": waves})
    assert st["n_tiles"] == st0["n_tiles"] and st["n_runs"] == st0["n_runs"]
    nw = min(waves, st["n_tiles"])

    def want(wj, wk):
        return dict(family="plain", waves=nw, n_jk_cached=0)
    d = eng.jk_describe()
    assert st["n_runs"] <= d["segments"] <= st["n_runs"] + nw - 1, (d, st)    # runs, cut once more per wave boundary at most
    if waves == 1:
        assert d["segments"] == st["n_runs"]
    _check_single(f"{name}/{basis} jk_waves={waves}", eng, D[0], ora[0], dflt[0], want)
    eng.close()


@pytest.mark.parametrize("name,basis,nao", CASES)
def test_fixed_wave_planner_with_pair_kernel(name, basis, nao):
    mol, D, ora, dflt, st0 = _ref(name, basis)
    eng, st = _engine(mol, {"jk_waves": 3, "jk_pair": 1})
    _check_pair(f"{name}/{basis} jk_waves=3 pair", eng, D, ora, dflt,
                lambda wj, wk: dict(family="pair", waves=min(3, st["n_tiles"]), nt=0))
    eng.close()


@pytest.mark.parametrize("name,basis,nao", CASES)
@pytest.mark.parametrize("runmax", [1, 2, "above"])
def test_runmax_cuts_runs_into_segments(name, basis, nao, runmax):
    """`runmax` = tiles per work item of the longest-first planner: 1 makes every tile a segment, a value above the longest
    run (a run has at most one tile per AO block) leaves the runs whole, 2 lies strictly in between when some run is longer."""
    mol, D, ora, dflt, st0 = _ref(name, basis)
    nblk = (mol.nao + 7) // 8
    eng, st = _engine(mol, {"runmax": nblk + 1 if runmax == "above" else runmax})
    d = eng.jk_describe()
    nt_, nr = st["n_tiles"], st["n_runs"]
    if runmax == 1:
        assert d["segments"] == nt_, (d, st)
    elif runmax == "above":
        assert d["segments"] == nr, (d, st)
    else:
        assert max(nr, (nt_ + 1) // 2) <= d["segments"] <= nt_, (d, st)
        if nt_ >= 2 * nr:                                 # then some run has two tiles or more: runmax = 2 merges a pair
            assert d["segments"] < nt_, (d, st)
    if nblk > 1:
        assert nr < nt_                                   # the three settings really differ on every store but the one-block one

    def want(wj, wk):
        return dict(family="plain", waves=d["segments"], segments=d["segments"])
    _check_single(f"{name}/{basis} runmax={runmax}", eng, D[0], ora[0], dflt[0], want)
    eng.close()


# ---- layouts of the store -------------------------------------------------------------------------------------------------------------
LAYOUTS = [("ao_order0", {"ao_order": 0}, 1), ("ket_cluster0", {"ket_cluster": 0}, 1),
           ("ao0_ket0_tri0", {"ao_order": 0, "ket_cluster": 0, "tri_tiles": 0, "jk_pipe": 0}, 0),
           ("ao0_ket0_tri0_pipe", {"ao_order": 0, "ket_cluster": 0, "tri_tiles": 0}, 0)]


@pytest.mark.parametrize("name,basis,nao", CASES)
@pytest.mark.parametrize("lid,opts,tri", LAYOUTS, ids=[v[0] for v in LAYOUTS])
def test_store_layouts(name, basis, nao, lid, opts, tri):
    mol, D, ora, dflt, _ = _ref(name, basis)
    eng, _ = _engine(mol, opts)
    pipe = tri == 0 and "jk_pipe" not in opts

    def want(wj, wk):
        return dict(family="pipe" if (pipe and wk) else "plain", tri=tri)
    _check_single(f"{name}/{basis} {lid}", eng, D[0], ora[0], dflt[0], want)
    eng.close()


# ---- two densities in one pass ------------------------------------------------------------------------------------------------------------
PAIR_VARIANTS = [("pair", {}, dict(nt=0, dpp=1, tri=1)), ("pair_nt2", {"jk_nt": 2}, dict(nt=1, dpp=1, tri=1)),
                 ("pair_dpp0", {"jk_dpp": 0}, dict(nt=0, dpp=0, tri=1)), ("pair_tri0", {"tri_tiles": 0, "jk_pipe": 0}, dict(nt=0, dpp=1, tri=0)),
                 ("pair_tri0_nt2_dpp0", {"tri_tiles": 0, "jk_pipe": 0, "jk_nt": 2, "jk_dpp": 0}, dict(nt=1, dpp=0, tri=0))]


@pytest.mark.parametrize("name,basis,nao", CASES)
@pytest.mark.parametrize("vid,opts,fields", PAIR_VARIANTS, ids=[v[0] for v in PAIR_VARIANTS])
def test_pair_kernel_variants(name, basis, nao, vid, opts, fields):
    mol, D, ora, dflt, _ = _ref(name, basis)
    eng, _ = _engine(mol, dict(opts, jk_pair=1))
    _check_pair(f"{name}/{basis} {vid}", eng, D, ora, dflt, lambda wj, wk: dict(fields, family="pair"))
    assert eng.jk_describe(n_dm=1)["family"] != "pair" and eng.jk_describe(n_dm=3)["family"] != "pair"
    eng.set_option("jk_pair", 0)                          # immediate: the same store, one pass per density
    assert eng.jk_describe(n_dm=2)["family"] != "pair"
    _check_pair(f"{name}/{basis} {vid} looped", eng, D, ora, dflt, lambda wj, wk: dict(fields, family="plain"))
    eng.close()


# ---- re-preparation on one context, and a new context on the parked store ------------------------------------------------------------------
@pytest.mark.parametrize("name,basis,nao", CASES)
def test_reprepare_with_other_layout_and_planner(name, basis, nao):
    """One Engine: defaults first, then `tri_tiles`, `ao_order`, `jk_waves`, `runmax` flipped and `prepare_eri` again (a stale tile
    directory, AO permutation or segment buffer of the first store would show), then back to the defaults."""
    mol, D, ora, dflt, st0 = _ref(name, basis)
    eng, _ = _engine(mol, {})
    _check_single(f"{name}/{basis} first prepare", eng, D[0], ora[0], dflt[0], lambda wj, wk: dict(family="plain", tri=1))
    d0 = eng.jk_describe()
    for k, v in (("tri_tiles", 0), ("ao_order", 0), ("jk_waves", 5), ("runmax", 1)):
        eng.set_option(k, v)
    assert eng.jk_describe() == d0                        # all four wait for the next prepare
    st = eng.prepare_eri(1e-13)
    nw = min(5, st["n_tiles"])
    _check_single(f"{name}/{basis} second prepare", eng, D[0], ora[0], dflt[0],
                  lambda wj, wk: dict(family="pipe" if wk else "plain", tri=0, waves=nw))
    _check_pair(f"{name}/{basis} second prepare, n_dm=2 looped", eng, D, ora, dflt, lambda wj, wk: dict(tri=0, waves=nw))
    for k, v in (("tri_tiles", 1), ("ao_order", 1), ("jk_waves", 0), ("runmax", 0)):
        eng.set_option(k, v)
    eng.prepare_eri(1e-13)
    assert eng.jk_describe() == d0
    _check_single(f"{name}/{basis} third prepare", eng, D[0], ora[0], dflt[0], lambda wj, wk: dict(family="plain", tri=1))
    eng.close()


def test_new_context_reuses_parked_store_with_other_layout():
    """A closed context parks its tile store and the next context on the device takes it over when it is large enough.  The
    first context has full rows in the caller's AO order, the second the default layout (triangular rows, angular-momentum-major
    order, fewer doubles) on the same block of memory, the third another molecule: nothing of an earlier store's content,
    directory or permutation may survive."""
    from mi355scf.engine import release_cache, tile_store_allocations
    mol, D, ora, dflt, _ = _ref("h2o", "cc-pvtz")
    mol_s, D_s, ora_s, dflt_s, _ = _ref("ch4", "cc-pvdz")
    release_cache()
    eng, st = _engine(mol, {"tri_tiles": 0, "ao_order": 0, "jk_pipe": 0})
    _check_single("parked store: first context, full rows", eng, D[0], ora[0], dflt[0], lambda wj, wk: dict(family="plain", tri=0))
    eng.close()
    n1 = tile_store_allocations(0)
    eng, st2 = _engine(mol, {"ket_cluster": 0})
    assert st2["stored_bytes"] < st["stored_bytes"]       # triangular rows: fewer doubles than the parked block holds
    assert tile_store_allocations(0) == n1                # ... which was taken over, not allocated afresh
    _check_single("parked store: second context, default rows", eng, D[0], ora[0], dflt[0], lambda wj, wk: dict(family="plain", tri=1))
    _check_pair("parked store: second context, pair", eng, D, ora, dflt, lambda wj, wk: dict(tri=1))
    eng.close()
    eng, _ = _engine(mol_s, {})
    _check_single("parked store: smaller molecule", eng, D_s[0], ora_s[0], dflt_s[0], lambda wj, wk: dict(family="plain", tri=1))
    eng.close()
    release_cache()


# ---- the other consumers of the store ----------------------------------------------------------------------------------------------------------
_ERI = {}


def _eri_full(name, basis):
    if (name, basis) not in _ERI:
        from oracle import oracle as orc
        _ERI[(name, basis)] = orc.Oracle(_ref(name, basis)[0]).eri_full()
    return _ERI[(name, basis)]


CONSUMER_OPTS = [("nt2", {"jk_nt": 2}, dict(nt=1, tri=1)), ("ao_order0", {"ao_order": 0}, dict(nt=0, tri=1)),
                 ("tri0", {"tri_tiles": 0}, dict(nt=0, tri=0))]


@pytest.mark.parametrize("name,basis", [("h2co", "6-31g(d)"), ("h2o", "cc-pvtz")])
@pytest.mark.parametrize("oid,opts,fields", CONSUMER_OPTS, ids=[v[0] for v in CONSUMER_OPTS])
def test_jk_multi_and_qtrans_under_store_options(name, basis, oid, opts, fields):
    """`mi_build_jk_multi` and `mi_eri_qtrans` read the same directory, segments, AO permutation and `jk_nt` switch as the
    single-density kernels: dense contractions of the oracle's tensor, tolerances of test_gpu_jk_multi.py (1e-10 max(1, |K|))
    and test_gpu_mp2_stream.py (1e-10 absolute, exact (q, r) symmetry)."""
    import torch
    from mi355scf.engine import Engine
    mol = _ref(name, basis)[0]
    eri = _eri_full(name, basis)
    nao = mol.nao
    eng, _ = _engine(mol, opts)
    d = eng.jk_describe()
    for k, v in fields.items():
        assert d[k] == v, (k, d)
    rng = np.random.default_rng(31 + nao)
    n = 11                                                # more than one launch of the default batch of 8
    A = rng.standard_normal((n, nao, nao))
    sym = [1 if m % 3 else -1 for m in range(n)]
    Dm = np.array([0.5 * (a + s * a.T) for a, s in zip(A, sym)])
    J, K = eng.get_jk_multi(torch.as_tensor(Dm, device=eng.device), sym)
    J, K = J.cpu().numpy(), K.cpu().numpy()
    Jr = np.einsum("ijkl,mkl->mij", eri, Dm, optimize=True)
    Kr = np.einsum("ijkl,mjl->mik", eri, Dm, optimize=True)
    scale = max(1.0, np.abs(Kr).max())
    print(f"{name}/{basis} {oid}: multi max|K - ref| = {np.abs(K - Kr).max():.3e} (scale {scale:.2f})")
    assert np.abs(K - Kr).max() < 1e-10 * scale
    for m in range(n):
        if sym[m] > 0:
            assert np.abs(J[m] - Jr[m]).max() < 1e-10 * scale
        else:
            assert np.abs(J[m]).max() == 0.0 and np.abs(Jr[m]).max() < 1e-10 * scale
    for nb in (1, Engine.qtrans_batch() + 1):
        C = rng.standard_normal((nao, nb))
        ref = np.einsum("spqr,so->opqr", eri, C, optimize=True)
        Y = eng.eri_qtrans(C).cpu().numpy()
        err = np.abs(Y - ref).max()
        print(f"{name}/{basis} {oid}: qtrans nb={nb} max|Y - ref| = {err:.3e}")
        assert Y.shape == ref.shape and err < 1e-10, err
        assert np.abs(Y - Y.transpose(0, 1, 3, 2)).max() <= 1e-13
    eng.close()


# ---- a store beyond the Infinity Cache: cached prefix and nontemporal remainder -----------------------------------------------------------
def _cpu_share():
    """CPUs this process may really use (affinity mask and cgroup quota), as the benchmark's CPU leg sizes its thread pool."""
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    try:
        quota, period = open("/sys/fs/cgroup/cpu.max").read().split()[:2]
        if quota != "max":
            n = min(n, max(1, int(round(int(quota) / int(period)))))
    except Exception:
        pass
    return max(1, min(n, 16))


def test_cached_prefix_and_nontemporal_split_benzene_ccpvtz():
    """benzene/cc-pVTZ: N = 264, 4.9 GB of tiles.  Whole J and K of two seeded densities from the oracle's packed in-core array
    (no screening: tol = 0) once; then `jk_cache_mb` = 0 / default / larger than the store, re-prepared each time, and under each
    the default kernel (J+K, J only, K only), `jk_kjlt`, `jk_dpp = 0`, `jk_nt = 0` and the pair kernel with two densities.  The
    fixed-wave planner has no cached prefix; a hand-over buffer of the smallest accepted size (`work_mb` below 8 is taken as 8 MiB =
    2^20 doubles) is filled in several chunks here: the (pp|pp) class alone hands over 81 doubles for each of its ~10^5 quartets
    (the store does not report the chunk count; the kept p-p shell pairs are counted from `schwarz()` instead)."""
    import torch
    from mi355scf import fixtures
    from mi355scf.engine import Engine, release_cache
    from mi355scf.mole import Mole
    from oracle import oracle as orc
    release_cache()
    mol = Mole(atom=fixtures.BENZENE, basis="cc-pvtz", verbose=0).build()
    assert mol.nao == 264
    D = [_sym_density(264, 7), _sym_density(264, 8)]
    orc.Oracle.set_num_threads(_cpu_share())
    t0 = time.time()
    o = orc.Oracle(mol).incore(tol=0.0)
    t_pack = time.time() - t0
    t0 = time.time()
    ora = [o.jk_incore(d) for d in D]
    t_jk = time.time() - t0
    del o
    print(f"oracle benzene/cc-pVTZ on {orc.Oracle.num_threads()} threads: in-core pack {t_pack:.1f} s, two J/K digestions {t_jk:.2f} s")
    bound = [tuple(1e-9 * max(1.0, np.abs(x).max()) for x in jk) for jk in ora]

    def cmp(tag, got, m, which):
        got = got.cpu().numpy()
        err = np.abs(got - ora[m][which]).max()
        print(f"{tag}: max|got - oracle| = {err:.3e} (bound {bound[m][which]:.3e})")
        assert np.isfinite(got).all() and err < bound[m][which], (tag, err)

    def run_all(eng, tag, nt_on):
        for opts, family in (({}, "plain"), ({"jk_kjlt": 1}, "kjlt"), ({"jk_dpp": 0}, "plain"), ({"jk_nt": 0}, "plain")):
            for k, v in opts.items():
                eng.set_option(k, v)
            d = eng.jk_describe()
            assert d["family"] == family and d["nt"] == (0 if "jk_nt" in opts else nt_on) and d["dpp"] == (0 if "jk_dpp" in opts else 1), d
            for wj, wk in (BUILDS if not opts else BUILDS[:1]):
                J, K = eng.get_jk(D[0], with_j=wj, with_k=wk)
                if wj:
                    cmp(f"{tag} {opts} J (with_k={int(wk)})", J, 0, 0)
                if wk:
                    cmp(f"{tag} {opts} K (with_j={int(wj)})", K, 0, 1)
            for k, v in (("jk_kjlt", 0), ("jk_dpp", 1), ("jk_nt", 1)):
                eng.set_option(k, v)
        eng.set_option("jk_pair", 1)
        D2 = torch.as_tensor(np.stack(D), device=eng.device)
        for wj, wk in BUILDS:
            d = eng.jk_describe(wj, wk, 2)
            assert d["family"] == "pair" and d["nt"] == nt_on, d
            J, K = eng.get_jk(D2, with_j=wj, with_k=wk)
            for m in range(2):
                if wj:
                    cmp(f"{tag} pair J[{m}] (with_k={int(wk)})", J[m], m, 0)
                if wk:
                    cmp(f"{tag} pair K[{m}] (with_j={int(wj)})", K[m], m, 1)
        eng.set_option("jk_pair", -1)
        assert eng.jk_describe(n_dm=2)["family"] == "plain"      # 4.9 GB is below the 16 GB switch

    eng = Engine(mol)
    for cache_mb in (0, None, 10 ** 6):
        if cache_mb is not None:
            eng.set_option("jk_cache_mb", cache_mb)
        st = eng.prepare_eri(1e-13)
        assert st["stored_bytes"] > 256 << 20
        d = eng.jk_describe()
        assert d["nt"] == 1 and d["waves"] == d["segments"] > 0, d
        if cache_mb == 0:
            assert d["n_jk_cached"] == 0, d
        elif cache_mb is None:
            assert 0 < d["n_jk_cached"] < d["segments"], d
        else:
            assert st["stored_bytes"] < cache_mb << 20 and d["n_jk_cached"] == d["segments"], d
        run_all(eng, f"jk_cache_mb={cache_mb}", 1)
        eng.close()
        eng = Engine(mol)                                  # (default jk_cache_mb again; the parked store is taken over)
    # the fixed-wave planner: no cached prefix whatever jk_cache_mb says; smallest hand-over buffer: several chunks per class pair
    eng.set_option("jk_waves", 4096)
    eng.set_option("work_mb", 1)
    eng.set_option("eri_tpq", 0)                           # every class through the Rys launch -> buffer -> transform launch pair
    st = eng.prepare_eri(1e-13)
    ls = mol._bas[:, 1]
    n_pp = int((np.triu(eng.schwarz() > 0) & (ls[:, None] == 1) & (ls[None, :] == 1)).sum())
    assert n_pp * (n_pp + 1) // 2 * 81 > 4 * (8 << 17), n_pp   # (pp|pp) alone: more than four fills of the 8 MiB buffer
    d = eng.jk_describe()
    assert d["waves"] == 4096 and d["n_jk_cached"] == 0 and d["nt"] == 1, d
    for wj, wk in BUILDS:
        J, K = eng.get_jk(D[0], with_j=wj, with_k=wk)
        if wj:
            cmp(f"jk_waves=4096 work_mb=8 J (with_k={int(wk)})", J, 0, 0)
        if wk:
            cmp(f"jk_waves=4096 work_mb=8 K (with_j={int(wj)})", K, 0, 1)
    eng.close()
    release_cache()
