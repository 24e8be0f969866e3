"""`mi_grad_eri_xpairs` (signed exchange-pair terms sum_m t_m (R^m_ac R^m_bd + R^m_ad R^m_bc) in the two-particle density of every
derivative quartet) against EXACT FP64 derivative integrals of the CPU oracle.

Inputs and tolerance as in test_gpu_grad_oracle.py (its helpers, seeds and cached references are imported, not copied): random
O(1) matrices from fixed seeds, prepare_eri(1e-14), grad_dtol = 1e-30, |g - g_ref| <= 1e-10 max(1, |g_ref|max) + 2 (dropped part
reported by the oracle).

  * symmetric R: the oracle knows the exchange of a symmetric matrix through its spin-density slot,
        g_K[R] = orc.grad_eri(D, R, 1) - orc.grad_eri(D, None, 1)   (the gradient of -1/4 ex(R, R)),  term = -4 t g_K[R];
  * antisymmetric R: the dense derivative tensor d/dA_mu (mu nu|kappa lambda) of water/6-31G(d), assembled once from
    `Oracle.eri_ip1_shell`, contracted in NumPy with the two-particle density of the E2 formula of include/mi355scf.h.
Each test prints its figures (pytest -rP shows them)."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import MOLECULES
from test_gpu_grad_oracle import DEFAULTS, DTOL, QTOL, ROUTES, SYSTEMS, _check_routes, _dev, _mol, _oracle_eri, _routes, _sym

pytestmark = pytest.mark.gpu


def _asym(n, seed):
    a = np.random.default_rng(seed).standard_normal((n, n))
    return a - a.T


def _run(eng, mol, D, hyb, M=None, pairs=None, xpairs=None, rank=0, nranks=1):
    g = torch.zeros(mol.natm, 3, dtype=torch.float64, device=eng.device)
    kw = {}
    if pairs is not None:
        kw["pairs"] = (_dev(np.array(pairs[0]), eng) if len(pairs[1]) else None, np.asarray(pairs[1], dtype=np.float64))
    if xpairs is not None:
        R, t, sym = xpairs
        kw["xpairs"] = (_dev(np.array(R), eng) if len(t) else None, np.asarray(t, dtype=np.float64), list(sym))
    eng.grad_eri(_dev(D, eng), hyb, g, spin_density=_dev(M, eng) if M is not None else None, rank=rank, nranks=nranks, **kw)
    return g.cpu().numpy()


# ---- 1. symmetric R through the oracle ------------------------------------------------------------------------------------------
T8 = (0.7, -1.3, 0.4, -0.25, 2.0, -0.6, 0.05, -2.0)
S2 = (0.7, -1.3)
_XREF = {}


def _sym_reference(system, mol, D, M):
    """Per system, once: the 8 symmetric R^m with g_K[R^m] and its dropped part, and two pair matrices with g_J[Q^k].
    R^0..2 are independent random matrices (one oracle pass each); R^3..7 are multiples of M and D, whose g_K the shared
    reference of test_gpu_grad_oracle already holds (g_K[a R] = a^2 g_K[R])."""
    if system not in _XREF:
        from oracle import oracle as orc
        n = mol.nao
        o = orc.Oracle(mol)
        gJ, gKD, gKM, drop = _oracle_eri(system, mol, D, M)       # g_K[D], g_K[D] + g_K[M]
        g1, d1 = o.grad_eri(D, None, hyb=1.0, qtol=QTOL)
        R, gK, dK = [], [], []
        for m in range(3):
            Rm = _sym(n, 101 + m)
            g, d = o.grad_eri(D, Rm, hyb=1.0, qtol=QTOL)
            R.append(Rm), gK.append(g - g1), dK.append(np.abs(d).max() + np.abs(d1).max())
        for a, base, gb in ((0.5, M, gKM - gKD), (-1.5, D, gKD), (0.8, M, gKM - gKD), (1.2, D, gKD), (-0.3, M, gKM - gKD)):
            R.append(a * base), gK.append(a * a * gb), dK.append(2 * a * a * drop)
        Q, gQ, dQ = [], [], []
        for k in range(2):
            Qk = _sym(n, 111 + k)
            g, d = o.grad_eri(Qk, None, hyb=0.0, qtol=QTOL)
            Q.append(Qk), gQ.append(g), dQ.append(np.abs(d).max())
        _XREF[system] = (R, gK, dK, Q, gQ, dQ)
    return _XREF[system]


def _reference(system, mol, D, M, hyb, spin, kx, with_pairs):
    gJ, gKD, gKM, drop = _oracle_eri(system, mol, D, M)
    R, gK, dK, Q, gQ, dQ = _sym_reference(system, mol, D, M)
    g = gJ + hyb * (gKM if spin else gKD)
    for m in range(kx):
        g = g - 4.0 * T8[m] * gK[m]
        drop = drop + 4.0 * abs(T8[m]) * dK[m]
    if with_pairs:
        for k in range(2):
            g = g + S2[k] * gQ[k]
            drop = drop + abs(S2[k]) * dQ[k]
    return g, 1e-10 * max(1.0, np.abs(g).max()) + 2 * drop


@pytest.mark.parametrize("system", list(SYSTEMS))
def test_symmetric_exchange_pairs_match_exact_oracle(system):
    """K_x = 1, 3, 8 with weights of both signs; with and without `pairs` and a spin density; hyb 0 / 0.2 / 1; a three-way rank
    split that sums to the whole."""
    from mi355scf.engine import Engine
    mol = _mol(*SYSTEMS[system])
    n = mol.nao
    D, M = _sym(n, 31), _sym(n, 32)
    eng = Engine(mol)
    eng.prepare_eri(QTOL)
    eng.set_option("grad_dtol", DTOL)
    R, _gK, _dK, Q, _gQ, _dQ = _sym_reference(system, mol, D, M)
    worst = 0.0
    for kx, hyb, spin, with_pairs in ((1, 1.0, False, False), (3, 0.2, True, True), (8, 0.0, False, True), (8, 1.0, True, False)):
        ref, tol = _reference(system, mol, D, M, hyb, spin, kx, with_pairs)
        args = dict(M=M if spin else None, pairs=(Q, S2) if with_pairs else None, xpairs=(R[:kx], T8[:kx], [1] * kx))
        g = _run(eng, mol, D, hyb, **args)
        err = np.abs(g - ref).max()
        worst = max(worst, err / max(1.0, np.abs(ref).max()))
        print(f"{system} K_x={kx} hyb={hyb} spin={spin} pairs={with_pairs}: |g - g_ref| = {err:.2e} (tol {tol:.1e}, |g_ref|max "
              f"{np.abs(ref).max():.1f})")
        assert err < tol, (system, kx, hyb, spin, with_pairs, err, tol)
        if kx == 3:
            parts = [_run(eng, mol, D, hyb, rank=r, nranks=3, **args) for r in range(3)]
            assert all(np.abs(p).max() > 0 for p in parts)
            err3 = np.abs(sum(parts) - ref).max()
            print(f"{system}: three-way rank split |sum - g_ref| = {err3:.2e}")
            assert err3 < tol, (system, "rank split", err3, tol)
    print(f"{system}: worst |g - g_ref| / max(1, |g_ref|) = {worst:.2e}")


# ---- 2. antisymmetric and mixed R against the dense derivative tensor -------------------------------------------------------------
_DENSE = {}


def _dense():
    """(mol, oracle, T1 [3, n, n, n, n] = d/dA_mu (mu nu|kappa lambda) with A_mu the centre of mu's shell, atom of each AO,
    first AO of each shell) of water/6-31G(d) (10 shells, 10^4 shell quadruples), built once per session."""
    if not _DENSE:
        from oracle import oracle as orc
        mol = _mol(MOLECULES["h2o"], "6-31g(d)")
        o = orc.Oracle(mol)
        assert o.nbas == 10
        off = np.concatenate([[0], np.cumsum(2 * o.bas[:, 1] + 1)])
        n = mol.nao
        T1 = np.zeros((3, n, n, n, n))
        for i in range(o.nbas):
            for j in range(o.nbas):
                for k in range(o.nbas):
                    for l in range(o.nbas):
                        T1[:, off[i]:off[i + 1], off[j]:off[j + 1], off[k]:off[k + 1], off[l]:off[l + 1]] = o.eri_ip1_shell(i, j, k, l)
        _DENSE["x"] = (mol, o, T1, np.repeat(o.bas[:, 0], 2 * o.bas[:, 1] + 1), off)
    return _DENSE["x"]


def _density2(D, M, hyb, Q, s, R, t):
    """G of the E2 formula: E2 = 1/2 sum G_ijkl (ij|kl)."""
    G = np.einsum("ij,kl->ijkl", D, D) - 0.25 * hyb * (np.einsum("ik,jl->ijkl", D, D) + np.einsum("il,jk->ijkl", D, D))
    if M is not None:
        G -= 0.25 * hyb * (np.einsum("ik,jl->ijkl", M, M) + np.einsum("il,jk->ijkl", M, M))
    for k in range(len(s)):
        G += s[k] * np.einsum("ij,kl->ijkl", Q[k], Q[k])
    for m in range(len(t)):
        G += t[m] * (np.einsum("ik,jl->ijkl", R[m], R[m]) + np.einsum("il,jk->ijkl", R[m], R[m]))
    return G


def _dense_gradient(T1, aoatm, natm, G, mask=None):
    """G has the 8-fold symmetry of the integrals, so the four derivative positions contribute equally:
    dE2/dA = 1/2 . 4 sum_{mu on A} T1[mu nu kappa lambda] G_mu,nu,kappa,lambda.  mask: sum of |terms| over the masked elements."""
    E = 2.0 * T1 * G[None]
    per_ao = (np.abs(E) * mask[None]).sum(axis=(2, 3, 4)) if mask is not None else E.sum(axis=(2, 3, 4))
    g = np.zeros((natm, 3))
    np.add.at(g, aoatm, per_ao.T)
    return g


def _dropped_bound(o, mats, weights):
    """Bound of the part the Schwarz screening (q_ab q_cd < 1e-14) drops: for every matrix of the call the oracle's `qtol`
    output (the gradient carried by the dropped quartets) with |matrix| in place of D, at hyb 1 and at hyb 0, times its weight
    (1 for D and M, |s| for a pair matrix, 4 |t| for an exchange-pair matrix: ex(R, R) is -4 times the hyb-1-minus-hyb-0 part)."""
    tot = 0.0
    for Rm, w in zip(mats, weights):
        A = np.abs(Rm)
        _g1, d1 = o.grad_eri(A, None, hyb=1.0, qtol=QTOL)
        _g0, d0 = o.grad_eri(A, None, hyb=0.0, qtol=QTOL)
        tot += abs(w) * (np.abs(d1).max() + np.abs(d0).max())
    return tot


CASES = {
    "one antisymmetric, D = 0": dict(zero_d=True, hyb=1.0, spin=False, pairs=False, sym=(-1,), t=(-2.0,)),
    "antisymmetric pair of both signs": dict(zero_d=False, hyb=1.0, spin=False, pairs=False, sym=(-1, -1), t=(0.7, -1.3)),
    "mixed, with pairs and spin": dict(zero_d=False, hyb=0.2, spin=True, pairs=True, sym=(1, -1, -1, 1), t=(0.25, -2.0, 0.6, -0.4)),
    "eight mixed, hyb 0": dict(zero_d=False, hyb=0.0, spin=False, pairs=True, sym=(1, -1, 1, -1, -1, 1, -1, 1), t=T8),
}


@pytest.mark.parametrize("case", list(CASES))
def test_antisymmetric_and_mixed_exchange_pairs_match_the_dense_tensor(case):
    from mi355scf.engine import Engine
    c = CASES[case]
    mol, o, T1, aoatm, _off = _dense()
    n = mol.nao
    D = np.zeros((n, n)) if c["zero_d"] else _sym(n, 31)
    M = _sym(n, 32) if c["spin"] else None
    Q, s = ([_sym(n, 111), _sym(n, 112)], S2) if c["pairs"] else ([], ())
    R = [(_sym if sg > 0 else _asym)(n, 121 + m) for m, sg in enumerate(c["sym"])]
    ref = _dense_gradient(T1, aoatm, mol.natm, _density2(D, M, c["hyb"], Q, s, R, c["t"]))
    drop = _dropped_bound(o, [D] + ([M] if c["spin"] else []) + list(Q) + R, [1.0] + ([1.0] if c["spin"] else []) + list(s)
                          + [4.0 * w for w in c["t"]])
    tol = 1e-10 * max(1.0, np.abs(ref).max()) + 2 * drop
    eng = Engine(mol)
    eng.prepare_eri(QTOL)
    eng.set_option("grad_dtol", DTOL)
    g = _run(eng, mol, D, c["hyb"], M=M, pairs=(Q, s) if c["pairs"] else None, xpairs=(R, c["t"], c["sym"]))
    err = np.abs(g - ref).max()
    # the antisymmetric terms are not small: without them the reference moves by
    wo = _dense_gradient(T1, aoatm, mol.natm, _density2(D, M, c["hyb"], Q, s, [r for r, sg in zip(R, c["sym"]) if sg > 0],
                                                        [w for w, sg in zip(c["t"], c["sym"]) if sg > 0]))
    print(f"{case}: |g - g_ref| = {err:.2e} (tol {tol:.1e}, dropped-part bound {drop:.1e}, |g_ref|max {np.abs(ref).max():.1f}, "
          f"antisymmetric share {np.abs(ref - wo).max():.1f})")
    assert np.abs(ref - wo).max() > 1.0
    assert err < tol, (case, err, tol)


def test_dense_reference_agrees_with_the_oracle_gradient():
    """The NumPy contraction of the dense tensor is itself pinned: symmetric inputs against orc.grad_eri."""
    mol, o, T1, aoatm, _off = _dense()
    n = mol.nao
    D, M = _sym(n, 31), _sym(n, 32)
    ref = o.grad_eri(D, M, hyb=0.7)
    got = _dense_gradient(T1, aoatm, mol.natm, _density2(D, M, 0.7, [], (), [], ()))
    assert np.abs(got - ref).max() < 1e-11 * max(1.0, np.abs(ref).max())


# ---- 3. every route on benzene/cc-pVDZ ----------------------------------------------------------------------------------------------
def test_exchange_pairs_every_route_matches_exact_oracle(monkeypatch, capfd):
    """Symmetric R only, so the oracle reference stays exact: R = (M, 0.5 M, D) of test_gpu_grad_oracle's benzene inputs, whose
    g_K its cached reference holds -- no further oracle pass over benzene.  The closed-shell call (no spin density) carries the
    three exchange-pair terms; each route must be shown to have run."""
    from mi355scf import fixtures
    from mi355scf.engine import Engine
    mol = _mol(fixtures.BENZENE, "cc-pvdz")
    n = mol.nao
    assert n == 114 and mol.nbas == 54
    D, M = _sym(n, 41), _sym(n, 42)
    R, t = [M, 0.5 * M, D], (0.7, -1.3, 0.4)
    gJ, gKD, gKM, drop = _oracle_eri("benzene", mol, D, M)
    gKm = gKM - gKD
    eng = Engine(mol)
    eng.prepare_eri(QTOL)
    monkeypatch.setenv("MI355_DEBUG", "1")
    base = None
    report = []
    try:
        for name, opts, hyb in ROUTES:
            for k, v in {**DEFAULTS, **opts, "grad_dtol": DTOL}.items():
                eng.set_option(k, v)
            capfd.readouterr()
            g = _run(eng, mol, D, hyb, xpairs=(R, t, [1, 1, 1]))
            r = _routes(capfd.readouterr().err)
            base = base or r
            ref = gJ + hyb * gKD - 4.0 * (t[0] * gKm + t[1] * 0.25 * gKm + t[2] * gKD)
            tol = 1e-10 * max(1.0, np.abs(ref).max()) + 2 * drop * (1.0 + 4.0 * sum(abs(w) for w in t))
            err = np.abs(g - ref).max()
            report.append(f"route '{name}': classes on tpq {len(r['tpq'])}, rows {len(r['rows'])} (g32 {len(r['rows32'])}), pipeline "
                          f"{len(r['pipeline'])}; live lists {len(r['live'])}; |g - g_ref| = {err:.2e} (tol {tol:.1e})")
            assert err < tol, (name, err, tol)
            _check_routes(name, r, base)
    finally:
        eng.set_option("grad_rows_g32", 1)     # process-wide, not per context
        print("\n".join(report))


# ---- 4. the screening sees the exchange-pair term ---------------------------------------------------------------------------------
def test_screening_bound_includes_the_exchange_pair_term():
    """D = 0, one antisymmetric R, grad_dtol = 1e-10: the Hartree-Fock part of every bound vanishes, so a bound without the
    exchange-pair term would skip every quartet and return zero.  Tolerance: the quartets the bound MAY skip are those with
    q_ab q_cd (xmax_ac xmax_bd + xmax_ad xmax_bc) < grad_dtol, xmax_ab = sqrt|t| max_ab |R| (one term); the sum of the absolute
    values of their elements' contributions (taken at 2 grad_dtol, to cover rounding in q) is evaluated from the dense tensor and
    added twice to the 1e-10 of the other kernel tests."""
    from mi355scf.engine import Engine
    mol, o, T1, aoatm, off = _dense()
    n, nb = mol.nao, o.nbas
    R, t = _asym(n, 131), 0.7
    G = _density2(np.zeros((n, n)), None, 1.0, [], (), [R], (t,))
    ref = _dense_gradient(T1, aoatm, mol.natm, G)
    q = o.schwarz()
    xm = np.array([[np.sqrt(abs(t)) * np.abs(R[off[a]:off[a + 1], off[b]:off[b + 1]]).max() for b in range(nb)] for a in range(nb)])
    bound = (np.einsum("ab,cd,ac,bd->abcd", q, q, xm, xm) + np.einsum("ab,cd,ad,bc->abcd", q, q, xm, xm))
    sh = np.repeat(np.arange(nb), 2 * o.bas[:, 1] + 1)
    mask = (bound < 2e-10)[np.ix_(sh, sh, sh, sh)]
    may_skip = np.abs(_dense_gradient(T1, aoatm, mol.natm, G, mask=mask)).max()
    tol = 1e-10 * max(1.0, np.abs(ref).max()) + 2 * may_skip
    eng = Engine(mol)
    eng.prepare_eri(QTOL)
    eng.set_option("grad_dtol", 1e-10)
    g = _run(eng, mol, np.zeros((n, n)), 1.0, xpairs=([R], (t,), (-1,)))
    err = np.abs(g - ref).max()
    print(f"D = 0, K_x = 1, grad_dtol 1e-10: |g|max = {np.abs(g).max():.3f}, |g - g_ref| = {err:.2e} (tol {tol:.1e}; "
          f"{int(mask.sum())} of {mask.size} AO quadruples may be skipped, worth {may_skip:.1e})")
    assert np.abs(ref).max() > 1e-2
    assert err < tol


# ---- 5. K_x = 0 is mi_grad_eri_pairs ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spin", [False, True])
def test_no_exchange_pairs_reproduces_the_pair_entry_bit_for_bit(spin):
    from mi355scf.engine import Engine
    mol = _mol(*SYSTEMS["h2co/6-31g(d)"])
    n = mol.nao
    D, M = _sym(n, 31), (_sym(n, 32) if spin else None)
    Q = [_sym(n, 111), _sym(n, 112)]
    eng = Engine(mol)
    eng.prepare_eri(QTOL)
    eng.set_option("grad_dtol", DTOL)
    from test_gpu_casscf_grad import _grad_pairs   # calls mi_grad_eri_pairs itself
    for hyb in (0.2, 1.0):
        old = _grad_pairs(eng, mol, D, M, hyb, Q, S2)
        new = _run(eng, mol, D, hyb, M=M, pairs=(Q, S2), xpairs=([], (), ()))
        print(f"spin={spin} hyb={hyb}: max |new - old| = {np.abs(new - old).max():.1e}")
        assert np.array_equal(new, old), (spin, hyb, np.abs(new - old).max())
    plain = _run(eng, mol, D, 1.0, M=M)
    assert np.array_equal(_run(eng, mol, D, 1.0, M=M, xpairs=([], (), ())), _grad_pairs(eng, mol, D, M, 1.0, [], []))
    assert np.abs(plain - _run(eng, mol, D, 1.0, M=M, xpairs=([], (), ()))).max() <= 1e-13 * max(1.0, np.abs(plain).max())


# ---- 6. refusals ----------------------------------------------------------------------------------------------------------------------
def test_exchange_pair_entry_refuses_bad_arguments():
    from mi355scf import engine
    from mi355scf.engine import Engine
    mol = _mol(MOLECULES["h2o"], "sto-3g")
    n = mol.nao
    eng = Engine(mol)
    eng.prepare_eri()
    D = _sym(n, 1)
    # the Python wrapper, before any launch
    with pytest.raises(ValueError, match="at most 8"):
        _run(eng, mol, D, 1.0, xpairs=([D] * 9, [1.0] * 9, [1] * 9))
    with pytest.raises(ValueError, match="finite"):
        _run(eng, mol, D, 1.0, xpairs=([D], [float("nan")], [1]))
    with pytest.raises(ValueError, match="symmetry flags"):
        _run(eng, mol, D, 1.0, xpairs=([D], [1.0], [2]))
    with pytest.raises(ValueError, match="contiguous"):
        g = torch.zeros(mol.natm, 3, dtype=torch.float64, device=eng.device)
        eng.grad_eri(_dev(D, eng), 1.0, g, xpairs=(_dev(np.zeros((1, n, 2 * n)), eng)[:, :, ::2], [1.0], [1]))
    # the C entry point itself
    L = engine.lib()
    pd, pi = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int)
    Dd, Rd = _dev(D, eng), _dev(np.array([D] * 9), eng)
    g = torch.zeros(mol.natm, 3, dtype=torch.float64, device=eng.device)

    def call(e, R, t, sym, kx):
        t = np.asarray(t, dtype=np.float64)
        sym = np.asarray(sym, dtype=np.intc)
        return L.mi_grad_eri_xpairs(e._h, Dd.data_ptr(), None, 1.0, None, None, 0, R, t.ctypes.data_as(pd) if t.size else None,
                                    sym.ctypes.data_as(pi) if sym.size else None, kx, g.data_ptr(), 0, 1, None)
    for bad, msg in ((lambda: call(eng, Rd.data_ptr(), [1.0] * 9, [1] * 9, 9), "outside 0 .. 8"),
                     (lambda: call(eng, None, [1.0], [1], 1), "null"),
                     (lambda: call(eng, Rd.data_ptr(), [float("inf")], [1], 1), "not finite"),
                     (lambda: call(eng, Rd.data_ptr(), [1.0], [0], 1), "neither"),
                     (lambda: call(eng, Rd.data_ptr(), [1.0], [1], -1), "outside 0 .. 8")):
        with pytest.raises(RuntimeError, match=msg):
            engine._check(bad())
    lr = Engine(mol)
    lr.set_option("omega", 0.33)
    with pytest.raises(RuntimeError, match="long-range"):
        engine._check(call(lr, Rd.data_ptr(), [1.0], [1], 1))
    assert np.abs(g.cpu().numpy()).max() == 0.0      # nothing was launched
