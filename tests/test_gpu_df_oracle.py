"""The density-fitting drivers against the EXACT FP64 oracle (oracle/df.py: McMurchie-Davidson integrals and derivative integrals
on the combined shell list), element by element and at the launch shapes every DF user with a triple-zeta basis gets.

Test system: hand-made orbital and auxiliary sets (PySCF-format dicts, below) with s..f orbital and s..g auxiliary shells,
contracted and uncontracted, on  O, H, a ghost H and an H 17 Bohr away  (N = 75, N_aux = 109; no symmetry), the same atoms
with the ghost first (the unit function of the auxiliary context sits on atom 0), and O alone (every integral one-centre:
Rys argument 0, AB = 0).  `test_class_table_of_the_test_system` (CPU) keeps an edit of the dicts from dropping a class.

What is pinned, each at the bound the suite already applies to the same kernels:
  * (ij|P) and (P|Q) of `mi_df_build`, every element, 1e-10 max(1, |ref|max) (tests/test_gpu_eri_elements.py), default options
    and rys_fine = 0; finite, symmetric to the bit, untouched elements (dropped shell pairs) negligible in the oracle;
  * the several-pass loops of `mi_df_build` / `mi_df_grad` (option df_batch_max = 7): integrals bit-identical to one pass;
  * `mi_df_grad` with random symmetric Z3, Z2 against `oracle.df.grad`, 1e-10 max(1, |g_ref|max) (tests/test_gpu_grad_oracle.py);
  * `DF.get_jk` (dense and low-rank exchange) against `oracle.df.jk`, 1e-9 max(1, |ref|max) (tests/test_gpu_df.py);
  * `DF.grad_jk` (factorised and dense Z3 / Z2 algebra) against the docstring formulas written out in numpy on the oracle's
    integrals and pushed through `oracle.df.grad`, 1e-9 max(1, |g_ref|max): the fitted quantities are the metric solve of
    FP64 integrals good to ~1e-13, cond(V) <= 1e4 is asserted, the same argument as for J/K.  The numpy restatement itself is
    checked on the CPU against fourth-order differences of the numpy fitted energy.
Every test prints its worst error (pytest -rP)."""
import math

import numpy as np
import pytest
import torch

# PySCF-format shell lists [l, [exponent, coefficient], ...], sorted by l (the order Mole keeps)
ORB = {
    "O": [[0, [50.0, 0.05], [8.0, 0.30], [1.8, 0.70]], [0, [0.45, 1.0]],
          [1, [6.0, 0.30], [1.3, 0.80]], [1, [0.40, 1.0]],
          [2, [2.4, 0.40], [0.8, 0.70]],
          [3, [1.1, 1.0]], [3, [2.2, 0.50], [0.7, 0.60]]],
    "H": [[0, [3.0, 0.20], [0.35, 0.90]], [1, [0.9, 1.0]], [2, [1.0, 1.0]], [3, [1.2, 1.0]]],
}
AUX = {
    "O": [[0, [9.0, 0.40], [2.5, 0.70]], [1, [1.6, 1.0]], [2, [1.3, 1.0]], [3, [1.5, 1.0]],
          [4, [2.6, 0.50], [1.2, 0.60]], [4, [4.5, 1.0]]],
    "H": [[0, [0.9, 1.0]], [1, [1.1, 1.0]], [2, [1.2, 1.0]], [3, [1.4, 1.0]], [4, [1.6, 0.6], [3.0, 0.5]]],
}
GEOM = {
    "four": "O 0 0 0; H 0.76 0.59 0.1; Ghost:H -0.5 0.4 -0.8; H 0 0 9.0",
    "ghost-first": "Ghost:H -0.5 0.4 -0.8; O 0 0 0; H 0.76 0.59 0.1; H 0 0 9.0",
    "atom": "O 0 0 0",
}
LORB, LAUX = 3, 4
CLASSES3 = [(la, lb, lk) for la in range(LORB + 1) for lb in range(la + 1) for lk in range(LAUX + 1)]
CLASSES2 = [(lp, lk) for lp in range(LAUX + 1) for lk in range(LAUX + 1)]


def ncart(l):
    return (l + 1) * (l + 2) // 2


def ne_of(la, lb):
    """[e0| functions the Rys kernel hands over for a (la lb| pair: Cartesian shells la .. la + lb."""
    return sum(ncart(e) for e in range(la, la + lb + 1))


_MOL, _INT, _GRD = {}, {}, {}


def _mols(name):
    """(orbital Mole, auxiliary Mole as `DF.build` makes it), once per module."""
    if name not in _MOL:
        from mi355scf.mole import Mole
        mol = Mole(atom=GEOM[name], basis=ORB, verbose=0).build()
        aux = Mole(atom=[(s, xyz) for s, xyz in mol._atom], basis=AUX, unit="Bohr", verbose=0).build()
        _MOL[name] = (mol, aux)
    return _MOL[name]


def _ref_integrals(name):
    """The oracle's ((ij|P), (P|Q)), once per module, never modified."""
    if name not in _INT:
        from oracle import df as odf
        j3, j2 = odf.integrals(*_mols(name))
        j3.setflags(write=False)
        j2.setflags(write=False)
        _INT[name] = (j3, j2)
    return _INT[name]


def _sym(n, seed):
    a = np.random.default_rng(seed).standard_normal((n, n))
    return a + a.T


def _ref_grad(name):
    """(Z3, Z2, oracle gradient of Z3 alone, of Z2 alone): random symmetric densities of O(1) from fixed seeds."""
    if name not in _GRD:
        from oracle import df as odf
        mol, aux = _mols(name)
        n, na = mol.nao, aux.nao
        z3 = np.random.default_rng(71).standard_normal((n, n, na))
        z3 = z3 + z3.transpose(1, 0, 2)
        z2 = _sym(na, 72)
        _GRD[name] = (z3, z2, odf.grad(mol, aux, z3, None), odf.grad(mol, aux, None, z2))
    return _GRD[name]


def _dev(x, eng):
    return torch.as_tensor(np.ascontiguousarray(x), device=eng.device)


def _fitted(name, opts=None):
    """(orbital engine, DF built on it, engine of its auxiliary context); the DF's auxiliary Mole is the one the oracle got."""
    from mi355scf import df
    from mi355scf.engine import Engine
    mol, aux = _mols(name)
    eng = Engine(mol)
    for k, v in (opts or {}).items():
        eng.set_option(k, v)
    d = df.DF(mol, auxbasis=AUX).build(eng)
    assert np.array_equal(d.auxmol._bas, aux._bas) and np.array_equal(d.auxmol._env, aux._env) and d.naux == aux.nao
    return eng, d, Engine(d._aux_packed, device=eng.device)


# --- the test system itself (CPU) ---------------------------------------------------------------------------------------
def test_class_table_of_the_test_system():
    """Every angular class of `mi_df_build` / `mi_df_grad` for s..f orbitals and s..g auxiliaries occurs in the four-atom system
    as a one-centre triple, as a three-centre triple and with a contracted shell, and the classes and their differentiated
    partners reach all six instantiations of eri_rys_kernel<., 64> (1, 2, 4, 8, 16, 32 components per lane)."""
    mol, aux = _mols("four")
    assert (mol.nao, aux.nao) == (75, 109)
    R = mol.atom_coords()
    osh = [(int(b[0]), int(b[1]), int(b[2])) for b in mol._bas]       # (atom, l, primitives)
    ash = [(int(b[0]), int(b[1]), int(b[2])) for b in aux._bas]
    assert max(l for _, l, _ in osh) == LORB and max(l for _, l, _ in ash) == LAUX
    one, three, contracted = set(), set(), set()
    for ia, la, pa in osh:
        for ib, lb, pb in osh:
            if la < lb:
                continue
            for ik, lk, pk in ash:
                cls = (la, lb, lk)
                if ia == ib == ik:
                    one.add(cls)
                # orbital centres closer than 4 Bohr, one of them an H (exponents <= 3): mu r^2 < 48, no primitive pair is dropped
                if len({ia, ib, ik}) == 3 and np.linalg.norm(R[ia] - R[ib]) < 4.0:
                    three.add(cls)
                if max(pa, pb, pk) > 1:
                    contracted.add(cls)
    assert len(CLASSES3) == 50
    for have in (one, three, contracted):
        assert sorted(have) == CLASSES3
    assert max(e for sh in ORB["H"] for e, _c in sh[1:]) <= 3.0
    assert sorted({(lp, lk) for _, lp, _ in ash for _, lk, _ in ash}) == CLASSES2 and len(CLASSES2) == 25
    # the one-atom system has all of them as well (one-centre)
    m1, a1 = _mols("atom")
    assert sorted({(la, lb, lk) for la in m1._bas[:, 1] for lb in m1._bas[:, 1] if la >= lb for lk in a1._bas[:, 1]}) == CLASSES3
    assert sorted({(lp, lk) for lp in a1._bas[:, 1] for lk in a1._bas[:, 1]}) == CLASSES2

    def ranges(classes):
        """which of the ranges 1, 2, 3-4, 5-8, 9-16, 17-32 of ceil(ncomp / 64) the classes (l1 l2|lk) fall into"""
        out = set()
        for l1, l2, lk in classes:
            per = -(-ne_of(l1, l2) * ncart(lk) // 64)
            assert 1 <= per <= 32
            out.add(max(0, math.ceil(math.log2(per))))
        return out
    assert ne_of(3, 3) * ncart(4) == 1110 and ne_of(4, 3) * ncart(4) == 1500
    assert ranges(CLASSES3 + [(lp, 0, lk) for lp, lk in CLASSES2]) == set(range(6))
    # mi_df_grad: either shell of the pair differentiated (l + 1 and, for l >= 1, l - 1), and the auxiliary "pair" (P, unit)
    diff = []
    for la, lb, lk in CLASSES3:
        for l1, l2 in ((la, lb), (lb, la)):
            diff += [(l1 + 1, l2, lk)] + ([(l1 - 1, l2, lk)] if l1 else [])
    for lp, lk in CLASSES2:
        diff += [(lp + 1, 0, lk)] + ([(lp - 1, 0, lk)] if lp else [])
    assert ranges(diff) == set(range(6))


def test_metric_of_the_test_system_is_well_conditioned():
    """cond((P|Q)) <= 1e4 on the oracle's metric, which is what lets the fitted quantities keep 1e-9."""
    for name in GEOM:
        w = np.linalg.eigvalsh(_ref_integrals(name)[1])
        print(f"{name}: eigenvalues of (P|Q) {w[0]:.3e} .. {w[-1]:.3e}, cond {w[-1] / w[0]:.1f}")
        assert w[0] > 0 and w[-1] / w[0] <= 1e4
    j3 = _ref_integrals("four")[0]
    print(f"four: {np.mean(np.abs(j3) < 1e-30):.1%} of (ij|P) below 1e-30")
    assert np.mean(np.abs(j3) < 1e-30) > 0.25      # the far atom: pairs the driver drops


# --- test 1: the integrals, element by element ------------------------------------------------------------------------
def _class_report(tag, mol, aux, e3, e2, s3, s2):
    """One line per angular class: worst |got - ref| / max(1, |ref|max)."""
    lo = np.repeat(mol._bas[:, 1], 2 * mol._bas[:, 1] + 1)
    lx = np.repeat(aux._bas[:, 1], 2 * aux._bas[:, 1] + 1)
    for la, lb, lk in CLASSES3:
        blk = e3[np.ix_(lo == la, lo == lb, lx == lk)]
        print(f"{tag} ({'spdf'[la]}{'spdf'[lb]}|{'spdfg'[lk]}): {blk.max() / s3:.2e}")
    for lp, lk in CLASSES2:
        print(f"{tag} ({'spdfg'[lp]}|{'spdfg'[lk]}): {e2[np.ix_(lx == lp, lx == lk)].max() / s2:.2e}")


def _build_integrals(eng, aux_eng, n, na, fill=0.0):
    j3 = torch.full((n, n, na), fill, dtype=torch.float64, device=eng.device)
    j2 = torch.full((na, na), fill, dtype=torch.float64, device=eng.device)
    eng.df_build(aux_eng, j3, j2)
    torch.cuda.synchronize(eng.device)
    return j3, j2


def _check_integrals(name, opts, tag):
    mol, aux = _mols(name)
    r3, r2 = _ref_integrals(name)
    eng, _d, aux_eng = _fitted(name, opts)
    n, na = mol.nao, aux.nao
    t3, t2 = _build_integrals(eng, aux_eng, n, na)
    m3, m2 = _build_integrals(eng, aux_eng, n, na, fill=float("nan"))     # what the driver does not write stays NaN
    aux_eng.close()
    eng.close()
    j3, j2 = t3.cpu().numpy(), t2.cpu().numpy()
    untouched = torch.isnan(m3).cpu().numpy()
    assert not bool(torch.isnan(m2).any())                                 # every (P|Q) is written
    assert np.isfinite(j3).all() and np.isfinite(j2).all()
    assert np.array_equal(j3[~untouched], m3.cpu().numpy()[~untouched])    # and written with the same bits every time
    assert torch.equal(t2, m2)
    e3, e2 = np.abs(j3 - r3), np.abs(j2 - r2)
    s3, s2 = max(1.0, np.abs(r3).max()), max(1.0, np.abs(r2).max())
    _class_report(tag, mol, aux, e3, e2, s3, s2)
    left = np.abs(r3[untouched]).max() if untouched.any() else 0.0
    print(f"{tag}: (ij|P) {e3.max() / s3:.2e}, (P|Q) {e2.max() / s2:.2e} of max(1, |ref|max); {untouched.mean():.1%} of (ij|P) "
          f"left untouched, largest |ref| there {left:.1e}")
    assert e3.max() < 1e-10 * s3 and e2.max() < 1e-10 * s2
    assert np.array_equal(j3, j3.transpose(1, 0, 2))                       # (i,j,P) and (j,i,P) both written, equal
    assert np.array_equal(j2, j2.T)                                        # symmetric to the bit
    assert (j3[untouched] == 0.0).all() and left < 1e-25
    if name != "atom":
        assert untouched.mean() > 0.1                                      # the far atom's pairs with the others
    else:
        assert not untouched.any()
    return t3, t2, max(e3.max() / s3, e2.max() / s2)


@pytest.mark.gpu
@pytest.mark.parametrize("name,opts", [("four", {}), ("four", {"rys_fine": 0}), ("ghost-first", {}), ("atom", {})],
                         ids=["four", "four,rys_fine=0", "ghost-first", "atom"])
def test_df_integrals_elementwise(name, opts):
    """`Engine.df_build` into zero-filled tensors against `oracle.df.integrals`."""
    _check_integrals(name, opts, f"df_build {name} {opts}")


# --- test 2: several passes -----------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_df_several_passes_per_class():
    """df_batch_max = 7: at most seven tasks per pass, so nearly every class of `mi_df_build` and `mi_df_grad` runs several passes
    with a ragged last one.  A pass boundary changes no arithmetic: the integrals equal the one-pass ones to the bit (and 0, the
    default, is the one-pass run); the gradient is accumulated with atomics and gets the oracle bound."""
    one3, one2, _ = _check_integrals("four", {}, "df_build four, one pass")
    zero3, zero2, _ = _check_integrals("four", {"df_batch_max": 0}, "df_build four, df_batch_max=0")
    cap3, cap2, _ = _check_integrals("four", {"df_batch_max": 7}, "df_build four, df_batch_max=7")
    assert torch.equal(one3, zero3) and torch.equal(one2, zero2)
    assert torch.equal(one3, cap3) and torch.equal(one2, cap2)
    worst = _check_df_grad("four", {"df_batch_max": 7})
    print(f"df_grad four, df_batch_max=7: worst |g - g_ref| / max(1, |g_ref|max) = {worst:.2e}")
    from mi355scf.engine import Engine, EngineError
    eng = Engine(_mols("atom")[0])
    with pytest.raises(EngineError):
        eng.set_option("df_batch_max", -1)
    eng.close()


# --- test 3: mi_df_grad ---------------------------------------------------------------------------------------------------
def _check_df_grad(name, opts):
    mol, _aux = _mols(name)
    z3, z2, r3, r2 = _ref_grad(name)
    eng, _d, aux_eng = _fitted(name, opts)

    def run(a3, a2, rank=0, nranks=1):
        g = torch.zeros(mol.natm, 3, dtype=torch.float64, device=eng.device)
        eng.df_grad(aux_eng, _dev(a3, eng) if a3 is not None else None, _dev(a2, eng) if a2 is not None else None, g, rank, nranks)
        return g.cpu().numpy()
    worst = 0.0
    for a3, a2, ref in ((z3, None, r3), (None, z2, r2), (z3, z2, r3 + r2)):
        scale = max(1.0, np.abs(ref).max())
        for g in (run(a3, a2), sum(run(a3, a2, r, 3) for r in range(3))):
            err = np.abs(g - ref).max()
            worst = max(worst, err / scale)
            assert np.isfinite(g).all() and err < 1e-10 * scale, (a3 is not None, a2 is not None, err, scale)
            assert np.abs(g.sum(axis=0)).max() < 1e-9 * max(1.0, np.abs(g).max())      # translational invariance
    aux_eng.close()
    eng.close()
    return worst


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["four", "ghost-first"])
def test_df_grad_with_f_orbitals_matches_exact_oracle(name):
    """`mi_df_grad` up to the differentiated (g f|g .) class: Z3 only, Z2 only, both; one rank and the sum of three."""
    worst = _check_df_grad(name, {})
    print(f"df_grad {name}: worst |g - g_ref| / max(1, |g_ref|max) = {worst:.2e}")


@pytest.mark.gpu
def test_df_grad_of_one_atom_vanishes():
    """O alone: every derivative integral is added to and taken from the same atom.  What is left is rounding of sums whose
    terms are bounded by S = sum |Z| times the largest derivative integral (the oracle's, evaluated here)."""
    from oracle import df as odf
    from oracle import oracle as orc
    mol, aux = _mols("atom")
    z3, z2, r3, r2 = _ref_grad("atom")
    assert np.abs(r3).max() < 1e-12 and np.abs(r2).max() < 1e-12           # the oracle agrees that it is zero
    cm = odf._Combined(mol, aux)
    o = orc.Oracle(cm)
    ob, u = cm.nbas_orb, cm.nbas_orb + cm.nbas_aux
    d3 = max(np.abs(o.eri_ip1_shell(i, j, ob + p, u)).max() for i in range(mol.nbas) for j in range(mol.nbas) for p in range(aux.nbas))
    d2 = max(np.abs(o.eri_ip1_shell(ob + p, u, ob + q, u)).max() for p in range(aux.nbas) for q in range(aux.nbas))
    S = 2.0 * np.abs(z3).sum() * d3 + np.abs(z2).sum() * d2
    eng, _d, aux_eng = _fitted("atom")
    g = torch.zeros(1, 3, dtype=torch.float64, device=eng.device)
    eng.df_grad(aux_eng, _dev(z3, eng), _dev(z2, eng), g)
    g = g.cpu().numpy()
    aux_eng.close()
    eng.close()
    print(f"df_grad atom: |g|max = {np.abs(g).max():.2e}, S = {S:.3e} (largest derivative integrals {d3:.2f}, {d2:.2f})")
    assert np.isfinite(g).all() and np.abs(g).max() < 1e-10 * S


# --- test 4: fitted J/K and the Z3 / Z2 algebra of DF.grad_jk -----------------------------------------------------------------
def _psd(n, rank, seed):
    c = np.linalg.qr(np.random.default_rng(seed).standard_normal((n, rank)))[0]
    return c * np.sqrt(np.linspace(1.0, 0.5, rank))      # D = F F^T with eigenvalues 1 .. 0.5


def _spin_densities(n):
    """{case: [Da, Db]}: closed shell (D/2 twice, D of rank 5) and open shell (ranks 5 and 3)."""
    fa, fb = _psd(n, 5, 81), _psd(n, 3, 82)
    return {"closed": [fa @ fa.T, fa @ fa.T], "open": [fa @ fa.T, fb @ fb.T]}


def _e2_numpy(j3, j2, dms, hyb):
    """E2 of `DF.grad_jk`'s docstring in numpy."""
    D = dms[0] + dms[1]
    g = np.einsum("ijp,ij->p", j3, D)
    e = 0.5 * g @ np.linalg.solve(j2, g)
    if hyb:
        n, _, na = j3.shape
        C = np.linalg.solve(j2, j3.reshape(n * n, na).T).T.reshape(n, n, na)       # C[i,j,P] = sum_Q V^-1[P,Q] (Q|ij)
        for ds in dms:
            e -= 0.5 * hyb * np.einsum("ikp,ij,kl,jlp->", C, ds, ds, j3, optimize=True)
    return float(e)


def _z_numpy(j3, j2, dms, hyb):
    """Z3, Z2 of `DF.grad_jk`'s docstring in numpy: c = V^-1 g, C^P = sum_Q V^-1_PQ (Q|ij), Gs^P = Ds C^P Ds,
    Z3 = c_P D_ij - hyb sum_s Gs^P_ij,  Z2 = -1/2 c c^T + hyb/2 sum_s sum_ij C^P_ij Gs^Q_ij."""
    n, _, na = j3.shape
    D = dms[0] + dms[1]
    c = np.linalg.solve(j2, np.einsum("ijp,ij->p", j3, D))
    z3 = D[:, :, None] * c[None, None, :]
    z2 = -0.5 * np.outer(c, c)
    if hyb:
        C = np.linalg.solve(j2, j3.reshape(n * n, na).T).T.reshape(n, n, na)
        for ds in dms:
            G = np.einsum("ik,klp,lj->ijp", ds, C, ds, optimize=True)
            z3 -= hyb * G
            z2 += 0.5 * hyb * np.einsum("ijp,ijq->pq", C, G, optimize=True)
    return z3, 0.5 * (z2 + z2.T)


_GJK = {}
HYBS = (0.0, 1.0)


def _ref_grad_jk(case, hyb):
    """Exact gradient of the fitted two-electron energy of the four-atom system: numpy Z3 / Z2 on oracle integrals through the
    oracle's derivative integrals.  Nothing of the engine enters."""
    if (case, hyb) not in _GJK:
        from oracle import df as odf
        mol, aux = _mols("four")
        j3, j2 = _ref_integrals("four")
        z3, z2 = _z_numpy(j3, j2, _spin_densities(mol.nao)[case], hyb)
        _GJK[(case, hyb)] = odf.grad(mol, aux, z3, z2)
    return _GJK[(case, hyb)]


def test_numpy_restatement_of_the_fitted_gradient_matches_finite_differences():
    """The reference of `test_df_grad_jk_matches_numpy_on_oracle_integrals` against fourth-order central differences (h, 2h) of
    the numpy fitted energy on oracle integrals at displaced geometries: the bonded H, three directions, open shell, hyb = 1."""
    from mi355scf.mole import Mole
    from oracle import df as odf
    mol, _aux = _mols("four")
    dms = _spin_densities(mol.nao)["open"]
    g = _ref_grad_jk("open", 1.0)

    def E(x, h):
        R = mol.atom_coords().copy()
        R[1, x] += h
        m = mol.set_geom_(R, unit="Bohr", inplace=False)
        a = Mole(atom=[(s, xyz) for s, xyz in m._atom], basis=AUX, unit="Bohr", verbose=0).build()
        return _e2_numpy(*odf.integrals(m, a), dms, 1.0)
    h = 2e-3
    for x in range(3):
        d1 = (E(x, h) - E(x, -h)) / (2 * h)
        d2 = (E(x, 2 * h) - E(x, -2 * h)) / (4 * h)
        fd = (4.0 * d1 - d2) / 3.0
        print(f"dE2/dR[1,{x}]: analytic {g[1, x]:+.10f}, differences {fd:+.10f}")
        assert abs(g[1, x] - fd) < 1e-7 * max(1.0, np.abs(g).max()), (x, g[1, x], fd)


@pytest.mark.gpu
def test_df_jk_matches_oracle_dense_and_low_rank():
    """`DF.get_jk` on the f/g system: a random symmetric density (dense exchange route) and a rank-5 positive semi-definite one
    with rank_hint = 5 (pivoted-Cholesky route)."""
    from oracle import df as odf
    mol, _aux = _mols("four")
    j3, j2 = _ref_integrals("four")
    eng, d, aux_eng = _fitted("four")
    aux_eng.close()
    f = _psd(mol.nao, 5, 83)
    worst = 0.0
    for D, hint, path in ((0.5 * _sym(mol.nao, 84), None, "dense"), (f @ f.T, 5, "low rank")):
        d.rank_hint = hint
        J, K = d.get_jk(_dev(D, eng))
        assert d.k_path == path
        Jo, Ko = odf.jk(j3, j2, D)
        for got, ref in ((J, Jo), (K, Ko)):
            err = np.abs(got.cpu().numpy() - ref).max() / max(1.0, np.abs(ref).max())
            worst = max(worst, err)
            assert err < 1e-9, (path, err)
    eng.close()
    print(f"DF.get_jk four: worst |got - ref| / max(1, |ref|max) = {worst:.2e}")


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["closed", "open"])
def test_df_grad_jk_matches_numpy_on_oracle_integrals(case):
    """`DF.grad_jk` (hyb 0 and 1, factorised and dense route) against the engine-independent gradient of `_ref_grad_jk`."""
    mol, _aux = _mols("four")
    dms = _spin_densities(mol.nao)[case]
    eng, d, aux_eng = _fitted("four")
    aux_eng.close()
    worst = 0.0
    for hyb in HYBS:
        ref = _ref_grad_jk(case, hyb)
        scale = max(1.0, np.abs(ref).max())
        for factorize in (True, False):
            g = d.grad_jk([_dev(x, eng) for x in dms], hyb, factorize=factorize).cpu().numpy()
            err = np.abs(g - ref).max()
            worst = max(worst, err / scale)
            assert np.isfinite(g).all() and err < 1e-9 * scale, (case, hyb, factorize, err, scale)
    eng.close()
    print(f"DF.grad_jk four, {case} shell: worst |g - g_ref| / max(1, |g_ref|max) = {worst:.2e}")
