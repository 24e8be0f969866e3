"""`mi355scf.ao2mo` on the engine: the shared integral transformation against `torch.einsum` over the dense copy of the same
store (1e-10 absolute, the bound `test_gpu_mp2_stream.py` uses for `eri_qtrans` against that store), the guard of the resident
store and the frozen-core Fock matrix.  Molecules come from `conftest.MOLECULES`."""
import functools

import numpy as np
import pytest

from conftest import MOLECULES

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _rhf(basis):
    from pyscf import gto, scf
    mol = gto.M(atom=MOLECULES["h2o"], basis=basis, verbose=0)
    mf = scf.RHF(mol)
    mf.conv_tol = 1e-11
    mf.kernel()
    assert mf.converged
    return mol, mf


@pytest.mark.parametrize("basis,nao,ntargets", [("6-31g", 13, 2), ("6-31g(d)", 18, 1)])
def test_transform_matches_einsum_over_the_dense_store(basis, nao, ntargets):
    """Four seeded random coefficient blocks of pairwise different widths (a swapped index fails by shape or by value), C1 one
    column wider than a pass over the store; two targets sharing C1 and C2 are MP2's alpha-beta case.  N = 18 has (spherical) d
    shells, so the kernel's AO permutation is exercised."""
    import torch
    from mi355scf import ao2mo
    from mi355scf.engine import Engine
    mol, mf = _rhf(basis)
    eng = ao2mo.resident_engine(mf, "test")
    assert eng.nao == nao
    rng = np.random.default_rng(1300 + nao)
    block = lambda w: torch.as_tensor(rng.standard_normal((nao, w)), dtype=torch.float64, device=eng.device)
    C1, C2 = block(Engine.qtrans_batch() + 1), block(3)
    targets = [(block(5), block(2)), (block(4), block(6))][:ntargets]
    timing = dict(qtrans_seconds=0.0, gemm_seconds=0.0, passes=0)
    out = ao2mo.transform(eng, C1, C2, targets, timing)
    assert timing["passes"] == 2 and timing["qtrans_seconds"] > 0 and timing["gemm_seconds"] > 0
    dense = eng.eri_dense()
    assert len(out) == ntargets
    for got, (C3, C4) in zip(out, targets):
        ref = torch.einsum("spqr,so,pa,qj,rb->oajb", dense, C1, C2, C3, C4)
        assert got.shape == ref.shape == (C1.shape[1], 3, C3.shape[1], C4.shape[1])
        err = float((got - ref).abs().max())
        print(f"H2O/{basis}: max |transform - einsum| = {err:.3e} (max |ref| = {float(ref.abs().max()):.3f})")
        assert err < 1e-10
    untimed = ao2mo.transform(eng, C1, C2, targets)             # the kernel sums with atomics: equal to rounding, not bitwise
    assert all(float((a - b).abs().max()) < 1e-10 for a, b in zip(untimed, out))


def test_transform_holds_two_tensors_at_its_peak():
    """With one target as wide as the basis every intermediate is one [n1, N, N, N] tensor T: Y + X1, X1 + X2 and X2 + result are
    the three stages, so torch never holds more than 2 T (what `qtrans_work_bytes` and the callers' 80 % plans count; the
    kernel's accumulator is not torch's).  Keeping X1 through the third GEMM would show as 3 T."""
    import torch
    from mi355scf import ao2mo
    mol, mf = _rhf("6-31g")
    eng = ao2mo.resident_engine(mf, "test")
    N, n1 = eng.nao, 9
    rng = np.random.default_rng(77)
    C1, C = (torch.as_tensor(rng.standard_normal((N, w)), dtype=torch.float64, device=eng.device) for w in (n1, N))
    ao2mo.transform(eng, C1, C, [(C, C)])                       # warm: library work spaces exist
    torch.cuda.synchronize(eng.device)
    torch.cuda.reset_peak_memory_stats(eng.device)
    base = torch.cuda.memory_allocated(eng.device)
    out, = ao2mo.transform(eng, C1, C, [(C, C)])
    torch.cuda.synchronize(eng.device)
    peak = torch.cuda.max_memory_allocated(eng.device) - base
    T = 8 * n1 * N ** 3
    print(f"transform peak: {peak} B = {peak / T:.3f} T (T = {T} B)")
    assert out.shape == (n1, N, N, N) and 2 * T <= peak <= 2 * T + 8192      # 8 KiB: the allocator's 512 B rounding, the copy of C1


def test_resident_engine_prepares_a_missing_store_and_refuses_sharded_and_direct_mode_references():
    from pyscf import gto, scf
    from mi355scf import ao2mo
    mol, mf = _rhf("6-31g")
    eng = ao2mo.resident_engine(mf, "test")
    assert eng is mf.engine and eng.eri_ready
    mf._nranks = 2                                           # a two-rank object
    try:
        with pytest.raises(NotImplementedError, match="sharded"):
            ao2mo.resident_engine(mf, "test")
    finally:
        mf._nranks = 1
    fitted = scf.RHF(gto.M(atom=MOLECULES["h2o"], basis="sto-3g", verbose=0)).density_fit()     # its set-up builds no store
    fitted.kernel()
    assert fitted.converged and not fitted.engine.eri_ready
    assert ao2mo.resident_engine(fitted, "test") is fitted.engine and fitted.engine.eri_ready
    md = scf.RHF(gto.M(atom=MOLECULES["h2o"], basis="sto-3g", verbose=0))          # direct mode: the store is not resident
    md._test_memory_view = (True, 1.0e9, 0.45e9)
    md.direct_reserve_gb = 0.0
    md.kernel()
    assert md._stream_groups > 1
    with pytest.raises(NotImplementedError, match="direct mode"):
        ao2mo.resident_engine(md, "test")


def test_core_fock():
    import torch
    from mi355scf import ao2mo
    mol, mf = _rhf("6-31g")
    eng = ao2mo.resident_engine(mf, "test")
    C = torch.as_tensor(np.asarray(mf.mo_coeff), dtype=torch.float64, device=eng.device)
    h = mf._h1
    Dc = 2.0 * C[:, :3] @ C[:, :3].T
    J, K = mf._jk(Dc)
    ref = mol.energy_nuc() + float(torch.sum(Dc * (h + 0.5 * (J - 0.5 * K))))
    FI, e_core = ao2mo.core_fock(mf, C, 3)
    print(f"H2O/6-31G, ncore = 3: E_core = {e_core:.12f}, reference {ref:.12f}, diff {e_core - ref:.2e}")
    assert abs(e_core - ref) <= 1e-12
    assert float((FI - (h + J - 0.5 * K)).abs().max()) <= 1e-12
    F0, e0 = ao2mo.core_fock(mf, C, 0)
    assert F0 is h and e0 == float(mol.energy_nuc())
