"""Streaming MP2 (`mi355scf.mp2`, algorithm "stream") and its native kernel, the occupied-index quarter transformation of the
resident ERI tiles (`mi_eri_qtrans` / `Engine.eri_qtrans`).

Tolerances are the project's own: 1e-10 absolute for ERI-level parity (as test_gpu_eri_elements.py / test_gpu_rsh.py), 1e-8 Ha
for MP2 energies (as test_gpu_interaction.py; 1e-7 where that file allows it for UMP2 on a closed shell).  References: the CPU
oracle's dense integrals wherever they exist (N <= 80); the dense path (`mi_eri_unpack` + torch contractions, the tested code
of the earlier revision) at benzene/cc-pVDZ; nothing independent at benzene/cc-pVTZ (N = 264), where only internal
consistency can be checked -- said again in that test."""
import numpy as np
import pytest

from conftest import MOLECULES

pytestmark = pytest.mark.gpu

OH = "O 0 0 0; H 0 0 0.9697"


def _mol(atom, basis, spin=0):
    from mi355scf.mole import Mole
    return Mole(atom=atom, basis=basis, spin=spin, verbose=0).build()


def _rhf(mol, tol=1e-11):
    from pyscf import scf
    mf = scf.RHF(mol)
    mf.conv_tol = tol
    mf.kernel()
    assert mf.converged
    return mf


def _mp2(mf, algorithm="stream", **kw):
    from pyscf import mp
    pt = mp.MP2(mf, **{k: v for k, v in kw.items() if k == "frozen"})
    pt.algorithm = algorithm
    if "occ_batch" in kw:
        pt.occ_batch = kw["occ_batch"]
    pt.kernel()
    return pt


# ---- 1. kernel vs the oracle, element by element ------------------------------------------------------------------------------
@pytest.mark.parametrize("tri", [1, 0])
@pytest.mark.parametrize("name,basis,nao", [("h2o", "6-31G(d)", 18), ("h2co", "6-31G(d)", 32), ("h2o", "cc-pVTZ", 58)])
def test_qtrans_matches_oracle_elementwise(name, basis, nao, tri):
    """Y[o,p,q,r] = sum_s C[s,o] (sp|qr) against einsum over the oracle's dense tensor, seeded random dense C, for nb = 1, 3
    and batch + 1 (a second pass).  N = 18 has ragged edge tiles, N = 32 none, N = 58 has f shells; both tile layouts."""
    from mi355scf.engine import Engine
    from oracle import oracle as orc
    mol = _mol(MOLECULES[name], basis)
    assert mol.nao == nao
    eng = Engine(mol)
    eng.set_option("tri_tiles", tri)
    eng.prepare_eri(1e-13)
    eri = orc.Oracle(mol).eri_full()
    rng = np.random.default_rng(20240 + nao + tri)
    cap = Engine.qtrans_batch()
    for nb in (1, 3, cap + 1):
        C = rng.standard_normal((nao, nb))
        ref = np.einsum("spqr,so->opqr", eri, C, optimize=True)
        Y = eng.eri_qtrans(C).cpu().numpy()
        assert Y.shape == (nb, nao, nao, nao)
        err = np.abs(Y - ref).max()
        print(f"{name}/{basis} tri={tri} nb={nb}: max |Y - ref| = {err:.3e} (max |ref| = {np.abs(ref).max():.3f})")
        assert err < 1e-10, err
        assert np.abs(Y - Y.transpose(0, 1, 3, 2)).max() <= 1e-13


def test_qtrans_screened_tiles_give_zero_not_garbage():
    """A store prepared with a loose Schwarz tolerance drops tiles: where the dense copy of that store (`mi_eri_unpack`) is
    zero for every s, Y must be exactly zero, and everywhere it equals the contraction of that (screened) dense copy."""
    import torch
    from mi355scf.engine import Engine
    # two waters 8 A apart: whole tiles between the monomers fall below 1e-5
    atom = MOLECULES["h2o"] + "; O 0 0 8.0; H 0 -0.757 8.587; H 0 0.757 8.587"
    mol = _mol(atom, "6-31G(d)")
    eng = Engine(mol)
    eng.prepare_eri(1e-5)
    dense = eng.eri_dense()
    assert float((dense == 0).double().mean()) > 0.2          # tiles really were dropped
    rng = np.random.default_rng(7)
    C = torch.as_tensor(rng.standard_normal((mol.nao, 3)), device=eng.device)
    Y = eng.eri_qtrans(C)
    ref = torch.einsum("spqr,so->opqr", dense, C)
    assert float((Y - ref).abs().max()) < 1e-10
    dead = (dense != 0).sum(dim=0) == 0                       # (p,q,r) that no stored integral reaches
    assert int(dead.sum()) > 0
    assert float(Y[:, dead].abs().max()) == 0.0
    assert bool(torch.isfinite(Y).all())


# ---- 2. energies vs the oracle ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("basis", ["6-31G", "cc-pVTZ"])
def test_stream_energy_matches_oracle(basis):
    from oracle import oracle as orc
    mol = _mol(MOLECULES["h2o"], basis)
    pt = _mp2(_rhf(mol))
    ref = orc.mp2(mol)
    print(f"H2O/{basis}: E_corr stream = {pt.e_corr:.12f}, oracle = {ref:.12f}, diff = {pt.e_corr - ref:.2e}")
    assert abs(pt.e_corr - ref) < 1e-8
    assert abs(pt.e_corr_os + pt.e_corr_ss - pt.e_corr) < 1e-12


def test_stream_known_answer_components_and_t2():
    """H2O/cc-pVDZ: -0.204019967288338 Ha of PySCF's own example/test [MEM]; os + ss = total; t2 equals the dense path's."""
    mf = _rhf(_mol(MOLECULES["h2o"], "cc-pVDZ"))
    pt = _mp2(mf)
    print(f"H2O/cc-pVDZ: E_corr = {pt.e_corr:.15f} (os {pt.e_corr_os:.12f}, ss {pt.e_corr_ss:.12f})")
    assert abs(pt.e_corr + 0.204019967288338) < 2e-8
    assert abs(pt.e_corr_os + pt.e_corr_ss - pt.e_corr) < 1e-12
    assert pt.e_corr_os < 0 and pt.e_corr_ss < 0 and abs(pt.e_corr_os) > abs(pt.e_corr_ss)
    assert abs(pt.e_tot - (mf.e_tot + pt.e_corr)) < 1e-14
    pd = _mp2(mf, "dense")
    assert pt.t2 is not None and pt.t2.shape == pd.t2.shape
    assert float((pt.t2 - pd.t2).abs().max()) < 1e-9
    assert abs(pt.e_corr - pd.e_corr) < 1e-8
    assert abs(pt.e_corr_os - pd.e_corr_os) < 1e-8 and abs(pt.e_corr_ss - pd.e_corr_ss) < 1e-8


# ---- 3. stream vs dense beyond the oracle's reach -----------------------------------------------------------------------------
def test_stream_matches_dense_benzene_ccpvdz():
    """N = 114: the dense path is the earlier revision's tested code, not the code under test."""
    from pyscf import scf
    from mi355scf.fixtures import BENZENE
    mol = _mol(BENZENE, "cc-pVDZ")
    mf = _rhf(mol)
    es, ed = _mp2(mf).e_corr, _mp2(mf, "dense").e_corr
    print(f"benzene/cc-pVDZ RMP2: stream {es:.12f}, dense {ed:.12f}, diff {es - ed:.2e}")
    assert abs(es - ed) < 1e-8
    mu = scf.UHF(mol)
    mu.conv_tol = 1e-11
    mu.kernel()
    us, ud = _mp2(mu).e_corr, _mp2(mu, "dense").e_corr
    print(f"benzene/cc-pVDZ UMP2: stream {us:.12f}, dense {ud:.12f}, diff {us - ud:.2e}; vs RMP2 {us - es:.2e}")
    assert abs(us - ud) < 1e-8
    assert abs(us - es) < 1e-7


# ---- 4. open shell ------------------------------------------------------------------------------------------------------------
def test_ump2_open_shell_oh():
    """OH/6-31G(d) doublet: stream vs dense, and vs a NumPy UMP2 from the oracle's integrals and the converged orbitals."""
    from pyscf import scf
    from oracle import oracle as orc
    mol = _mol(OH, "6-31G(d)", spin=1)
    mf = scf.UHF(mol)
    mf.conv_tol = 1e-11
    mf.kernel()
    assert mf.converged
    ps, pd = _mp2(mf), _mp2(mf, "dense")
    eri = orc.Oracle(mol).eri_full()
    c, e, occ = np.asarray(mf.mo_coeff), np.asarray(mf.mo_energy), np.asarray(mf.mo_occ)
    sp = [(c[s][:, occ[s] > 0], c[s][:, occ[s] == 0], e[s][occ[s] > 0], e[s][occ[s] == 0]) for s in range(2)]

    def ovov(a, b):
        return np.einsum("pqrs,pi,qa,rj,sb->iajb", eri, sp[a][0], sp[a][1], sp[b][0], sp[b][1], optimize=True)

    def den(a, b):
        return sp[a][2][:, None, None, None] - sp[a][3][None, :, None, None] + sp[b][2][None, None, :, None] - sp[b][3][None, None, None, :]

    ref_ss = 0.0
    for s in range(2):
        g = ovov(s, s)
        anti = g - g.transpose(0, 3, 2, 1)
        ref_ss += 0.25 * np.sum(anti * anti / den(s, s))
    g = ovov(0, 1)
    ref_os = np.sum(g * g / den(0, 1))
    ref = ref_ss + ref_os
    print(f"OH/6-31G(d) UMP2: stream {ps.e_corr:.12f}, dense {pd.e_corr:.12f}, numpy {ref:.12f}")
    assert abs(ps.e_corr - pd.e_corr) < 1e-8
    assert abs(ps.e_corr - ref) < 1e-8
    assert abs(ps.e_corr_ss - ref_ss) < 1e-8 and abs(ps.e_corr_os - ref_os) < 1e-8
    assert ps.t2 is None


# ---- 5. frozen core -----------------------------------------------------------------------------------------------------------
def test_frozen_core():
    from oracle import oracle as orc
    mol = _mol(MOLECULES["h2o"], "cc-pVDZ")
    mf = _rhf(mol)
    full = _mp2(mf).e_corr
    f1 = _mp2(mf, frozen=1)
    eri = orc.Oracle(mol).eri_full()
    c, e, occ = np.asarray(mf.mo_coeff), np.asarray(mf.mo_energy), np.asarray(mf.mo_occ)
    o = occ > 0
    o[0] = False
    co, cv, eo, ev = c[:, o], c[:, occ == 0], e[o], e[occ == 0]
    g = np.einsum("pqrs,pi,qa,rj,sb->iajb", eri, co, cv, co, cv, optimize=True)
    d = eo[:, None, None, None] - ev[None, :, None, None] + eo[None, None, :, None] - ev[None, None, None, :]
    ref = float(np.sum(g / d * (2 * g - g.transpose(0, 3, 2, 1))))
    print(f"H2O/cc-pVDZ frozen=1: stream {f1.e_corr:.12f}, numpy {ref:.12f}; all-electron {full:.12f}")
    assert abs(f1.e_corr - ref) < 1e-8
    assert f1.t2.shape == (4, 19, 4, 19)
    assert abs(_mp2(mf, frozen=[0]).e_corr - f1.e_corr) < 1e-12
    assert abs(_mp2(mf, frozen=0).e_corr - full) < 1e-12
    assert abs(f1.e_corr) < abs(full)
    # a frozen virtual as well: the highest orbital
    nmo = c.shape[1]
    fv = _mp2(mf, frozen=[0, nmo - 1])
    cv2, ev2 = cv[:, :-1], ev[:-1]
    g = np.einsum("pqrs,pi,qa,rj,sb->iajb", eri, co, cv2, co, cv2, optimize=True)
    d = eo[:, None, None, None] - ev2[None, :, None, None] + eo[None, None, :, None] - ev2[None, None, None, :]
    assert abs(fv.e_corr - float(np.sum(g / d * (2 * g - g.transpose(0, 3, 2, 1))))) < 1e-8


# ---- 6. batching is invisible -------------------------------------------------------------------------------------------------
def test_occupied_batching_is_invisible():
    mf = _rhf(_mol(MOLECULES["h2co"], "6-31G(d)"))
    es = [_mp2(mf, occ_batch=b).e_corr for b in (1, 2, 8)]
    auto = _mp2(mf).e_corr
    print("H2CO/6-31G(d) E_corr by occupied batch 1, 2, all, auto:", es, auto)
    assert max(abs(x - es[0]) for x in es + [auto]) < 1e-11


def test_t2_is_dropped_above_the_cap(monkeypatch):
    from mi355scf import mp2
    mf = _rhf(_mol(MOLECULES["h2o"], "6-31G"))
    kept = _mp2(mf)
    monkeypatch.setattr(mp2, "T2_MAX_BYTES", 8 * 5 * 5 * 8 * 8 - 1)      # one byte less than this molecule's amplitudes
    dropped = _mp2(mf)
    assert kept.t2 is not None and dropped.t2 is None
    assert abs(kept.e_corr - dropped.e_corr) < 1e-12


# ---- 7. the gap itself: N = 264 > 220 -----------------------------------------------------------------------------------------
def test_benzene_ccpvtz_runs():
    """Benzene/cc-pVTZ (N = 264) was refused (NotImplementedError) by the dense path.  There is NO independent reference at
    this size (the oracle stops at N = 80, the dense path at 220): only internal consistency is checked here."""
    from mi355scf.fixtures import BENZENE
    mol = _mol(BENZENE, "cc-pVTZ")
    assert mol.nao == 264
    mf = _rhf(mol, tol=1e-10)
    pa = _mp2(mf, occ_batch=8)
    pb = _mp2(mf, occ_batch=5)
    print(f"benzene/cc-pVTZ: E_corr = {pa.e_corr:.12f} (batch 8), {pb.e_corr:.12f} (batch 5); timing {pa.timing}")
    assert np.isfinite(pa.e_corr) and pa.e_corr < 0
    assert pa.e_tot == mf.e_tot + pa.e_corr
    assert abs(pa.e_corr - pb.e_corr) < 1e-10
    assert abs(pa.e_corr_os + pa.e_corr_ss - pa.e_corr) < 1e-12
    assert pa.t2 is not None and tuple(pa.t2.shape) == (21, 243, 21, 243)     # 208 MB: below the 1.17 GB cap
    fc = _mp2(mf, frozen=6)
    assert abs(fc.e_corr) < abs(pa.e_corr) and fc.e_corr < 0
    with pytest.raises(NotImplementedError):
        _mp2(mf, "dense")


# ---- 8. template flow ---------------------------------------------------------------------------------------------------------
def test_calculate_energy_mp2_flow():
    """`templates/calculate_energy.py:117-141`, GPU rung of `--method MP2`: call sequence only."""
    import cupy, gpu4pyscf  # noqa: F401
    from gpu4pyscf.scf import hf as gpu_hf
    from pyscf import gto
    mol = gto.Mole()
    mol.atom = MOLECULES["h2co"]
    mol.basis = "6-31G(d)"
    mol.charge = 0
    mol.spin = 0
    mol.verbose = 0
    mol.build()
    mf_hf = gpu_hf.RHF(mol)
    mf_hf.init_guess = "atom"
    mf_hf = mf_hf.to_gpu()
    mf_hf.kernel()
    from gpu4pyscf import mp
    mp2 = mp.MP2(mf_hf)
    mp2.kernel()
    energy = mp2.e_tot
    assert isinstance(energy, float) and energy < mf_hf.e_tot
    import pyscf.mp
    for m in (mp, pyscf.mp):
        assert m.MP2 is m.RMP2 is m.UMP2 is m.mp2.MP2


# ---- 9. refusals keep their types ---------------------------------------------------------------------------------------------
def test_refusals():
    from pyscf import scf
    from mi355scf.engine import Engine, EngineError
    mol = _mol(MOLECULES["h2o"], "6-31G")
    mf = _rhf(mol)
    mf._nranks = 2                                           # a two-rank object
    try:
        for alg in ("stream", "dense"):
            with pytest.raises(NotImplementedError):
                _mp2(mf, alg)
    finally:
        mf._nranks = 1
    eng = Engine(mol)
    eng.prepare_eri(1e-13, rank=0, nranks=2)                 # a sharded store
    with pytest.raises(EngineError):
        eng.eri_qtrans(np.ones((mol.nao, 1)))
    md = scf.RHF(mol)                                        # direct mode: the store is not resident
    md._test_memory_view = (True, 1.0e9, 0.45e9)
    md.direct_reserve_gb = 0.0
    md.kernel()
    assert md._stream_groups > 1
    with pytest.raises(NotImplementedError):
        _mp2(md)
    with pytest.raises(ValueError):
        _mp2(mf, "fast")
