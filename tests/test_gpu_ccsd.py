"""`cc.CCSD` / `ccsd_t` on the engine against the spin-orbital reference of `test_cc_host.py`, evaluated in the engine's own
converged orbitals with the CPU oracle's integrals (as `test_gpu_casci._reference` does).  Energies are compared to 1e-8 -- the
engine-versus-oracle margin `test_gpu_rsh.py` and `test_gpu_casci.py` use.  SCF conv_tol 1e-11, CCSD conv_tol 1e-10 and
conv_tol_normt 1e-8.  Molecules come from `conftest.MOLECULES`; H2 (not in that table) is 0.74 Angstrom along z."""
import functools
import math

import numpy as np
import pytest

from conftest import MOLECULES
from test_cc_host import H2, ref_ccsd, ref_ccsd_t

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _rhf(name, basis):
    from pyscf import gto, scf
    mol = gto.M(atom=MOLECULES.get(name, H2), basis=basis, verbose=0)
    mf = scf.RHF(mol)
    mf.conv_tol = 1e-11
    mf.kernel()
    assert mf.converged
    return mol, mf


@functools.lru_cache(maxsize=None)
def _ccsd(name, basis, frozen=None):
    from pyscf import cc
    mol, mf = _rhf(name, basis)
    mycc = cc.CCSD(mf, frozen=frozen)
    mycc.conv_tol, mycc.conv_tol_normt = 1e-10, 1e-8
    mycc.kernel()
    assert mycc.converged
    return mycc


@functools.lru_cache(maxsize=None)
def _reference(name, basis, frozen=0):
    """(reference CCSD dict, reference E(T)) from oracle integrals in the engine's converged orbitals."""
    from oracle import oracle as orc
    mol, mf = _rhf(name, basis)
    o = orc.Oracle(mol)
    S, T, V, _ = o.int1e()
    ref = ref_ccsd(T + V, o.eri_full(), np.asarray(mf.mo_coeff), mol.energy_nuc(), mol.nelectron // 2, frozen=frozen)
    return ref, ref_ccsd_t(ref)


def test_h2_ccsd_is_full_ci_and_t_vanishes():
    from pyscf import fci
    mol, mf = _rhf("h2", "6-31g(d,p)")
    mycc = _ccsd("h2", "6-31g(d,p)")
    e_fci = fci.FCI(mf).kernel()[0]
    et = mycc.ccsd_t()
    print(f"H2/6-31G(d,p): E(CCSD) - E(FCI) = {mycc.e_tot - e_fci:.2e}, E_corr = {mycc.e_corr:.8f}, E(T) = {et:.2e}, {mycc.cycles} cycles")
    assert abs(mycc.e_tot - e_fci) <= 1e-8 and abs(et) <= 1e-12
    assert mycc.e_corr < 0 and mycc.converged and isinstance(et, float) and mycc.e_t == et
    assert abs(mycc.e_tot - (mf.e_tot + mycc.e_corr)) < 1e-14 and mycc.e_hf == mf.e_tot


def test_h2o_sto3g_against_the_spin_orbital_reference():
    """o = 5, v = 2: v below any tile."""
    from pyscf import mp
    mol, mf = _rhf("h2o", "sto-3g")
    mycc = _ccsd("h2o", "sto-3g")
    ref, ref_t = _reference("h2o", "sto-3g")
    et = mycc.ccsd_t()
    emp2 = mp.MP2(mf).kernel()[0]
    t1, t2 = mycc.t1, mycc.t2
    print(f"H2O/STO-3G: E_corr - ref = {mycc.e_corr - ref['e_corr']:.2e}, E(T) - ref = {et - ref_t:.2e} (E(T) = {et:.3e}), "
          f"emp2 - MP2 = {mycc.emp2 - emp2:.2e}, |t2 - t2^T| = {np.abs(t2 - t2.transpose(1, 0, 3, 2)).max():.2e}")
    assert abs(mycc.e_corr - ref["e_corr"]) <= 1e-8 and abs(et - ref_t) <= 1e-8
    assert abs(mycc.emp2 - emp2) <= 1e-10
    assert isinstance(t1, np.ndarray) and isinstance(t2, np.ndarray) and t1.shape == (5, 2) and t2.shape == (5, 5, 2, 2)
    assert np.abs(t2 - t2.transpose(1, 0, 3, 2)).max() <= 1e-12
    # the amplitudes are the reference's: same-spin block of the spin-orbital t2 is t2 - t2^T(ab), alpha t1 is t1
    assert np.abs(ref["t1"][0::2, 0::2] - t1).max() < 1e-6
    assert np.abs(ref["t2"][0::2, 1::2, 0::2, 1::2] - t2).max() < 1e-6
    assert abs(mycc.energy(t1, t2) - mycc.e_corr) < 1e-12
    emp2_i, t1_i, t2_i = mycc.init_amps()
    assert abs(emp2_i - emp2) <= 1e-10 and np.abs(t1_i).max() == 0 and t2_i.shape == t2.shape


def test_h2o_631gd_frozen_core_batches_and_reproducibility():
    """o = 5, v = 13: not a multiple of 8 or 16."""
    mycc = _ccsd("h2o", "6-31g(d)")
    ref, ref_t = _reference("h2o", "6-31g(d)")
    et = mycc.ccsd_t()
    print(f"H2O/6-31G(d): E_corr - ref = {mycc.e_corr - ref['e_corr']:.2e}, E(T) - ref = {et - ref_t:.2e} (E(T) = {et:.6f}), "
          f"{mycc.cycles} cycles, {mycc.timing['t_triples']} triples in batches of {mycc.timing['t_batch']}")
    assert mycc.t1.shape == (5, 13) and mycc.timing["t_triples"] == 35
    assert abs(mycc.e_corr - ref["e_corr"]) <= 1e-8 and abs(et - ref_t) <= 1e-8

    fz = _ccsd("h2o", "6-31g(d)", 1)
    ref_f, ref_ft = _reference("h2o", "6-31g(d)", 1)
    et_f = fz.ccsd_t()
    print(f"frozen = 1: E_corr - ref = {fz.e_corr - ref_f['e_corr']:.2e}, E(T) - ref = {et_f - ref_ft:.2e}")
    assert fz.t1.shape == (4, 13) and abs(fz.e_corr - ref_f["e_corr"]) <= 1e-8 and abs(et_f - ref_ft) <= 1e-8

    mycc.t_batch = 3                                     # 35 triples: eleven batches of 3 and one of 2
    e3, e3_again = mycc.ccsd_t(), mycc.ccsd_t()
    assert mycc.timing["t_batch"] == 3
    mycc.t_batch = None
    e_all, e_all_again = mycc.ccsd_t(), mycc.ccsd_t()
    e_torch = mycc.ccsd_t(algorithm="torch")
    print(f"t_batch = 3 vs None: {e3 - e_all:.2e}, native vs torch: {e_all - e_torch:.2e}, repeats: {e3 - e3_again:.1e}, {e_all - e_all_again:.1e}")
    assert abs(e3 - e_all) <= 1e-11 and abs(e_all - e_torch) <= 1e-11 and abs(e3 - e_torch) <= 1e-11
    assert e3 == e3_again and e_all == e_all_again       # bit-identical
    assert mycc.e_t == e_torch and abs(mycc.e_tot - (mycc.e_hf + mycc.e_corr)) < 1e-14       # ccsd_t leaves e_tot alone


def _numpy_t_energy(raw, ijk, wt, t1, ovov, eo, ev):
    """The expression of `mi_cc_t_energy` (include/mi355scf.h) written out in numpy, every transposition literally: cube p of a
    triple is indexed by (a,b,c), (a,c,b), (b,a,c), (b,c,a), (c,a,b), (c,b,a) for p = 0..5."""
    out = np.zeros(len(ijk))
    for t, (i, j, k) in enumerate(ijk):
        R = raw[:, t]
        W = np.einsum("abc->abc", R[0]) + np.einsum("acb->abc", R[1]) + np.einsum("bac->abc", R[2]) + np.einsum("bca->abc", R[3]) \
            + np.einsum("cab->abc", R[4]) + np.einsum("cba->abc", R[5])
        V = W + np.einsum("a,bc->abc", t1[i], ovov[j, :, k, :]) + np.einsum("b,ac->abc", t1[j], ovov[i, :, k, :]) \
            + np.einsum("c,ab->abc", t1[k], ovov[i, :, j, :])
        Z = 4 * W + W.transpose(1, 2, 0) + W.transpose(2, 0, 1) - 2 * (W.transpose(0, 2, 1) + W.transpose(2, 1, 0) + W.transpose(1, 0, 2))
        D = eo[i] + eo[j] + eo[k] - ev[:, None, None] - ev[None, :, None] - ev[None, None, :]
        out[t] = wt[t] * np.sum(Z * V / (3.0 * D))
    return out


def _amp_inputs(o, v):
    """Random numerators, old amplitudes and (ia|jb); e_occ in [-2, -1], e_vir in [0.5, 1.5]: every denominator is below -1.5."""
    rng = np.random.default_rng(1000 * o + v)
    n = o * v + (o * v) ** 2
    return rng.standard_normal(n), rng.standard_normal(n), rng.standard_normal((o, v, o, v)), -1.0 - rng.random(o), 0.5 + rng.random(v)


def _check_amp_sums(name, got_dt2, got_e, dt_terms, e_terms):
    """The two sums against `math.fsum` of the reference terms with the a-priori bound of ANY summation order,
    (N + 8) 2^-53 sum |terms| (N - 1 additions of relative error 2^-53 each; the 8 covers the few roundings inside a term,
    contracted or not)."""
    from test_gpu_dense_kernels import U, record
    for what, got, terms in (("|err|^2", got_dt2, dt_terms), ("energy", got_e, e_terms)):
        bound = (terms.size + 8) * U * math.fsum(np.abs(terms))
        record(f"cc_amp_update {name} {what} ({terms.size} terms)", abs(got - math.fsum(terms)) / bound)


@pytest.mark.parametrize("o,v", [(1, 1), (2, 3), (5, 13), (8, 64), (10, 80)])
def test_amp_update_kernel_against_numpy(o, v):
    """`mi_cc_amp_update` against `numpy_amp_update`.  The kernel is a grid-stride loop of at most 1024 blocks x 256 threads:
    (8,64) has 262 656 elements, 512 past one trip; (10,80) has 640 800, 2.44 trips with a ragged last one.  New amplitudes within
    2 ulp (one correctly rounded division on both sides), err = new - old exactly for the kernel's own new amplitudes, the
    two sums within the any-order bound, and everything bit-identical on a repeat.
    MI355X: new amplitudes bit-identical (0 ulp) in all five cases.  Sum error / bound, |err|^2 and energy: (1,1) 0, 0; (2,3) 0, 0;
    (5,13) 4.2e-4, 0; (8,64) 4.4e-5, 3.3e-8; (10,80) 9.8e-6, 1.4e-8."""
    import torch
    from mi355scf import ccsd
    from test_cc_host import numpy_amp_update
    num, told, ovov, eo, ev = _amp_inputs(o, v)
    new, err, dt_terms, e_terms = numpy_amp_update(num, told, ovov, eo, ev)
    T = lambda a: torch.as_tensor(a, dtype=torch.float64, device="cuda").contiguous()
    args = [T(a) for a in (num, told, ovov, eo, ev)]
    tnew, terr, dt2, e = ccsd.amp_update_native(*args)
    tnew2, terr2, dt2_again, e_again = ccsd.amp_update_native(*args)
    tnew, terr = tnew.cpu().numpy(), terr.cpu().numpy()
    ulps = np.abs(tnew - new) / np.spacing(np.abs(new))
    print(f"o = {o}, v = {v}: {new.size} amplitudes, worst new-amplitude error {ulps.max():.1f} ulp, "
          f"{int((terr != tnew - told).sum())} err elements differ from new - old")
    assert tnew.shape == new.shape and ulps.max() <= 2.0
    assert np.array_equal(terr, tnew - told)
    _check_amp_sums(f"({o},{v})", dt2, e, dt_terms, e_terms)
    assert np.array_equal(tnew2.cpu().numpy(), tnew) and np.array_equal(terr2.cpu().numpy(), terr)
    assert dt2 == dt2_again and e == e_again                # fixed-order sums


def test_amp_update_c_entry_writes_only_its_outputs():
    """(8,64) through `mi_cc_amp_update` itself: `tnew`, `err`, `part` and `out` start as NaN, each followed by a guard band.
    Every element of the four is written (2 x 1024 block partials, 2 results), nothing beyond them.
    MI355X: all guards intact, no NaN left, sum error / bound 4.4e-5 (|err|^2) and 3.3e-8 (energy)."""
    import ctypes
    import torch
    from mi355scf import engine
    from test_cc_host import numpy_amp_update
    from test_gpu_dense_kernels import assert_guard, guarded
    o, v = 8, 64
    num, told, ovov, eo, ev = _amp_inputs(o, v)
    new, err, dt_terms, e_terms = numpy_amp_update(num, told, ovov, eo, ev)
    n = new.size
    L = engine.lib()
    nblk = min(-(-n // 256), int(L.mi_cc_amp_blocks()))
    assert nblk == 1024 and n == 262656
    T = lambda a: torch.as_tensor(a, dtype=torch.float64, device="cuda").contiguous()
    d_num, d_told, d_ovov, d_eo, d_ev = (T(a) for a in (num, told, ovov, eo, ev))
    sizes = dict(tnew=n, err=n, part=2 * nblk, out=2)
    bufs = {k: guarded(m) for k, m in sizes.items()}
    for k, m in sizes.items():
        bufs[k][:m] = float("nan")
    engine._check(L.mi_cc_amp_update(d_num.data_ptr(), d_told.data_ptr(), bufs["tnew"].data_ptr(), bufs["err"].data_ptr(), d_ovov.data_ptr(),
                                     d_eo.data_ptr(), d_ev.data_ptr(), o, v, bufs["part"].data_ptr(), bufs["out"].data_ptr(),
                                     ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    host = {k: bufs[k][:m].cpu().numpy() for k, m in sizes.items()}
    for k, m in sizes.items():
        assert_guard(bufs[k], m, f"cc_amp_update {k}")
        assert not np.isnan(host[k]).any(), f"{k}: {int(np.isnan(host[k]).sum())} elements not written"
    assert (np.abs(host["tnew"] - new) <= 2.0 * np.spacing(np.abs(new))).all() and np.array_equal(host["err"], host["tnew"] - told)
    part = host["part"].reshape(nblk, 2)
    assert host["out"][0] == np.add.accumulate(part[:, 0])[-1] and host["out"][1] == np.add.accumulate(part[:, 1])[-1]   # block order
    _check_amp_sums("(8,64) C entry", host["out"][0], host["out"][1], dt_terms, e_terms)


@pytest.mark.parametrize("v", [2, 8, 13, 16, 17, 25])
def test_t_energy_kernel_against_numpy(v):
    """Random raw cubes: a wrong permutation shows here, whatever the GEMM operands were.  1e-12 relative is FP64
    summation-order noise over at most 25^3 terms with a margin of a few hundred ulp.  v = 8 and 16 are whole tiles (no
    masked lane), v = 25 has four blocks (the block decode walks to A = 3); the third triple is also run alone (ntrip = 1).
    MI355X: worst per-triple relative error 6.0e-16 (v = 2), 3.7e-16 at v = 25; the lone triple is bit-identical to its batched value."""
    import torch
    from mi355scf import ccsd
    rng = np.random.default_rng(100 + v)
    o = 4
    ijk = np.array([(3, 2, 0), (2, 1, 0), (3, 3, 1), (1, 1, 0), (3, 2, 2), (2, 0, 0), (1, 1, 1), (3, 3, 3)], dtype=np.int32)
    wt = np.array([6.0, 6.0, 3.0, 3.0, 3.0, 3.0, 1.0, 1.0])
    raw = rng.standard_normal((6, len(ijk), v, v, v))
    t1, ovov = rng.standard_normal((o, v)), rng.standard_normal((o, v, o, v))
    eo, ev = -1.0 - rng.random(o), 0.5 + rng.random(v)
    ref = _numpy_t_energy(raw, ijk, wt, t1, ovov, eo, ev)
    dev = torch.device("cuda", 0)
    T = lambda a, dt=torch.float64: torch.as_tensor(a, dtype=dt, device=dev).contiguous()
    got = ccsd.t_energy_native(T(raw), T(ijk, torch.int32), T(wt), T(t1), T(ovov), T(eo), T(ev)).cpu().numpy()
    again = ccsd.t_energy_native(T(raw), T(ijk, torch.int32), T(wt), T(t1), T(ovov), T(eo), T(ev)).cpu().numpy()
    alt = ccsd._t_energy_torch(T(raw), T(ijk, torch.int64), T(wt), T(t1), T(ovov), T(eo), T(ev)).cpu().numpy()
    rel = np.abs(got - ref) / np.abs(ref)
    print(f"v = {v}: per-triple relative error {rel}, torch path {np.abs(alt - ref) / np.abs(ref)}")
    assert np.all(np.abs(ref) > 1e-3)                    # random cubes: no triple's sum is accidentally tiny
    assert rel.max() <= 1e-12 and (np.abs(alt - ref) / np.abs(ref)).max() <= 1e-12
    assert np.array_equal(got, again)
    lone = ccsd.t_energy_native(T(raw[:, 2:3]), T(ijk[2:3], torch.int32), T(wt[2:3]), T(t1), T(ovov), T(eo), T(ev)).cpu().numpy()
    print(f"ntrip = 1: relative error {abs(lone[0] - ref[2]) / abs(ref[2]):.2e}, batched - lone {got[2] - lone[0]:.1e}")
    assert lone.shape == (1,) and abs(lone[0] - ref[2]) <= 1e-12 * abs(ref[2]) and lone[0] == got[2]


def test_restart_from_converged_amplitudes():
    from pyscf import cc
    mol, mf = _rhf("h2o", "6-31g(d)")
    first = _ccsd("h2o", "6-31g(d)")
    again = cc.CCSD(mf)
    again.conv_tol, again.conv_tol_normt = 1e-10, 1e-8
    e_corr, t1, t2 = again.kernel(first.t1, first.t2)
    print(f"restart: {again.cycles} cycles, E_corr - first = {e_corr - first.e_corr:.2e}")
    assert again.converged and again.cycles <= 2 and abs(e_corr - first.e_corr) <= 1e-10
    assert np.abs(t2 - first.t2).max() < 1e-7


def test_readme_snippet():
    mol, mf = _rhf("h2o", "sto-3g")
    mine = _ccsd("h2o", "sto-3g")

    def snippet(mf):
        from pyscf import cc
        mycc = cc.CCSD(mf); mycc.kernel(); et = mycc.ccsd_t(); return mycc.e_tot + et

    e = snippet(mf)
    expect = mf.e_tot + mine.e_corr + mine.ccsd_t()
    print(f"README snippet: {e:.10f}, E(RHF) + E_corr + E(T) = {expect:.10f}")
    # The snippet stops at the defaults (|dE| < 1e-7, |dt| < 1e-5); the energy is linear in t2 and quadratic in t1, so what is left
    # is bounded by |dt| times the norm of the integrals it is contracted with (0.1 here): 1e-6.
    assert abs(e - expect) <= 1e-6


def test_direct_mode_and_oversized_cases_are_refused(monkeypatch):
    import torch
    from pyscf import cc, gto, scf
    from mi355scf.ccsd import CCSD
    mol, mf = _rhf("h2o", "sto-3g")
    md = scf.RHF(gto.M(atom=MOLECULES["h2o"], basis="sto-3g", verbose=0))          # direct mode: the store is not resident
    md._test_memory_view = (True, 1.0e9, 0.45e9)
    md.direct_reserve_gb = 0.0
    md.kernel()
    assert md._stream_groups > 1
    with pytest.raises(NotImplementedError, match="direct mode"):
        cc.CCSD(md).kernel()
    with pytest.raises(NotImplementedError, match="density-fitted"):
        cc.CCSD(mf).density_fit()
    # does not fit: pretend 1 MB of HBM is free; H2O/STO-3G (o = 5, v = 2) needs 3 * 7^4 doubles = 57.6 kB plus one qtrans
    # orbital, a few hundred kB more than 80 % of that
    real = torch.cuda.mem_get_info
    need = CCSD._need_bytes(5, 2, CCSD.diis_space)
    assert need == 8 * 3 * 7 ** 4
    monkeypatch.setattr(torch.cuda, "mem_get_info", lambda *a, **k: (need, real(*a, **k)[1]))
    small = cc.CCSD(mf)
    with pytest.raises(NotImplementedError, match=r"needs [0-9.]+ GB") as info:
        small.kernel()
    print(f"refused: {info.value}")
    assert "80 %" in str(info.value) and small.e_corr is None
    monkeypatch.setattr(torch.cuda, "mem_get_info", real)
    assert abs(cc.CCSD(mf).kernel()[0] - _ccsd("h2o", "sto-3g").e_corr) < 1e-6    # and with the real figure it runs
