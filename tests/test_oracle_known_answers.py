"""Pins the CPU oracle (and the remembered basis tables) to every known answer available offline.

The reference holds no golden vectors for this path -> "parity unpinned" against
PySCF in the strict sense.  What is checked here:
  * Szabo & Ostlund, Modern Quantum Chemistry, H2 / STO-3G at R = 1.4 a0: S12, T, V, (ij|kl), E (textbook)
  * T. D. Crawford's programming project #3 H2O/STO-3G total energy (public teaching reference)
  * PySCF total energies remembered from its documentation/tests -- labelled UNVERIFIED-MEMORY
  * internal identities: 8-fold ERI symmetry, direct J/K == dense einsum, Boys function vs mpmath
  * committed oracle-generated fixtures tests/golden/energies.json (made by tests/golden/make_golden.py)
"""
import ctypes
import json
import os

import numpy as np
import pytest

from conftest import MOLECULES


def _mol(atom, basis, **kw):
    from mi355scf.mole import Mole
    return Mole(atom=atom, basis=basis, verbose=0, **kw).build()


def test_szabo_ostlund_h2_sto3g():
    from oracle import oracle as orc
    mol = _mol("H 0 0 0; H 0 0 1.4", "sto-3g", unit="Bohr")
    o = orc.Oracle(mol)
    S, T, V, _ = o.int1e()
    eri = o.eri_full()
    assert abs(S[0, 1] - 0.6593) < 1e-4
    assert abs(T[0, 0] - 0.7600) < 1e-4 and abs(T[0, 1] - 0.2365) < 1e-4
    assert abs(V[0, 0] - (-1.2266 - 0.6538)) < 2e-4 and abs(V[0, 1] - 2 * (-0.5974)) < 2e-4
    assert abs(eri[0, 0, 0, 0] - 0.7746) < 1e-4 and abs(eri[0, 0, 1, 1] - 0.5697) < 1e-4
    assert abs(eri[1, 0, 0, 0] - 0.4441) < 1e-4 and abs(eri[1, 0, 1, 0] - 0.2970) < 1e-4
    r = orc.rhf(mol)
    assert abs(r["e_tot"] - (-1.1167)) < 1e-4


def test_szabo_ostlund_heh_cation_sto3g():
    """Szabo & Ostlund, Modern Quantum Chemistry, section 3.5.3 / appendix B: HeH+ at R = 1.4632 a0, STO-3G with zeta(He) = 2.0925,
    zeta(H) = 1.24 (exponents scale with zeta^2).  Book values [MEM, 4 decimals]: S12 = 0.4508, T11 = 2.1643, T12 = 0.1670, T22 =
    0.7600, (11|11) = 1.3072, (21|11) = 0.4373, (21|21) = 0.1773, (22|11) = 0.6057, (22|21) = 0.3118, (22|22) = 0.7746, electronic
    energy -4.227529, total energy -2.860662 (the book's own SCF used the 4-decimal integrals: agreement to 1e-5)."""
    from oracle import oracle as orc
    base = [(2.227660584, 0.154328967), (0.405771156, 0.535328142), (0.109818, 0.444634542)]
    sto = lambda z: [[0] + [[a * z * z, c] for a, c in base]]
    mol = _mol("He 0 0 0; H 0 0 1.4632", {"He": sto(2.0925), "H": sto(1.24)}, unit="Bohr", charge=1)
    o = orc.Oracle(mol)
    S, T, V, _ = o.int1e()
    eri = o.eri_full()
    assert abs(S[0, 1] - 0.4508) < 1e-4
    assert abs(T[0, 0] - 2.1643) < 1e-4 and abs(T[0, 1] - 0.1670) < 1e-4 and abs(T[1, 1] - 0.7600) < 1e-4
    for (i, j, k, l), ref in (((0, 0, 0, 0), 1.3072), ((1, 0, 0, 0), 0.4373), ((1, 0, 1, 0), 0.1773), ((1, 1, 0, 0), 0.6057),
                              ((1, 1, 1, 0), 0.3118), ((1, 1, 1, 1), 0.7746)):
        assert abs(eri[i, j, k, l] - ref) < 1e-4, (i, j, k, l, eri[i, j, k, l])
    assert abs(mol.energy_nuc() - 1.366867) < 1e-6
    r = orc.rhf(mol)
    assert abs(r["e_tot"] - (-2.860662)) < 1e-5


def test_crawford_h2o_sto3g():
    from oracle import oracle as orc
    mol = _mol("O 0 -0.143225816552 0; H 1.638036840407 1.136548822547 0; H -1.638036840407 1.136548822547 0",
               "sto-3g", unit="Bohr")
    assert abs(mol.energy_nuc() - 8.002367061810450) < 1e-9
    r = orc.rhf(mol)
    assert abs(r["e_tot"] - (-74.942079928192)) < 1e-8


@pytest.mark.parametrize("name,basis,e_mem", [
    ("h2o", "6-31g", -75.9839484980),      # UNVERIFIED-MEMORY (PySCF docs/tests)
    ("h2o", "cc-pvdz", -76.0267656731),    # UNVERIFIED-MEMORY (PySCF README example)
    ("hf", "cc-pvdz", -99.9873974403),     # UNVERIFIED-MEMORY (PySCF examples)
])
def test_remembered_pyscf_rhf_energies(name, basis, e_mem):
    from oracle import oracle as orc
    r = orc.rhf(_mol(MOLECULES[name], basis))
    assert r["converged"] and abs(r["e_tot"] - e_mem) < 2e-9


def test_eri_symmetry_and_direct_jk_equals_dense():
    from oracle import oracle as orc
    mol = _mol(MOLECULES["h2o"], "6-31g*")
    o = orc.Oracle(mol)
    eri = o.eri_full()
    assert np.abs(eri - eri.transpose(1, 0, 2, 3)).max() < 1e-13
    assert np.abs(eri - eri.transpose(2, 3, 0, 1)).max() < 1e-13
    rng = np.random.default_rng(2)
    a = rng.normal(size=(mol.nao, mol.nao))
    D = a + a.T
    J, K = o.jk(D, tol=0.0)
    assert np.abs(J - np.einsum("ijkl,kl->ij", eri, D)).max() < 1e-11
    assert np.abs(K - np.einsum("ijkl,jl->ik", eri, D)).max() < 1e-11
    # per-shell entry point agrees with the full tensor (f shell case too)
    mol3 = _mol(MOLECULES["h2o"], "cc-pvtz")
    o3 = orc.Oracle(mol3)
    blk = o3.eri_shell(9, 4, 9, 0)      # (f p | f s)
    assert blk.shape == (7, 3, 7, 1)
    assert np.abs(blk - o3.eri_shell(9, 0, 9, 4).transpose(2, 3, 0, 1)).max() < 1e-13
    assert np.abs(blk - o3.eri_shell(4, 9, 0, 9).transpose(1, 0, 3, 2)).max() < 1e-13


def test_boys_function_vs_mpmath():
    import mpmath as mp
    from oracle import oracle as orc
    L = orc.lib()
    for x in [0.0, 1e-9, 0.3, 2.0, 11.0, 25.0, 36.5, 41.0, 120.0]:
        F = np.zeros(13)
        L.orc_boys(12, ctypes.c_double(x), F.ctypes.data_as(ctypes.POINTER(ctypes.c_double)))
        for m in (0, 3, 12):
            ref = float(mp.quad(lambda t: t ** (2 * m) * mp.exp(-x * t * t), [0, 1]))
            assert abs(F[m] - ref) < 1e-14 + 2e-13 * ref


def test_oracle_reproduces_committed_golden_energies():
    from oracle import oracle as orc
    from mi355scf import fixtures
    g = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "energies.json")))
    for key, atom, basis in [("h2o_631g_rhf", fixtures.H2O, "6-31g"), ("h2co_631gd_rhf", fixtures.H2CO, "6-31g(d)")]:
        r = orc.rhf(_mol(atom, basis))
        assert abs(r["e_tot"] - g[key]["e_tot"]) < 1e-9
    assert g["benzene_ccpvdz_rhf"]["nao"] == 114 and g["benzene_ccpvdz_rhf"]["converged"]


def test_oracle_dft_grid_and_functionals():
    from oracle import dft as odft
    mol = _mol(MOLECULES["h2o"], "sto-3g")
    c, w = odft.build_grids(mol, 3)
    assert len(w) == 33698  # level 3: O (75,302) + 2 H (50,302), NWChem pruning
    assert abs((w * np.exp(-(c ** 2).sum(1))).sum() - np.pi ** 1.5) < 1e-6
    rho = np.array([0.3, 1.2, 0.01])
    sig = np.array([0.1, 2.0, 0.0004])
    for xc in ("LDA,VWN", "B3LYP", "PBE", "BLYP"):
        _, terms = odft.parse_xc(xc)
        e, vr, vs = odft.eval_xc(terms, rho, sig)
        h = 1e-6
        fr = (odft.energy_density(terms, rho + h, sig) - odft.energy_density(terms, rho - h, sig)) / (2 * h)
        fs = (odft.energy_density(terms, rho, sig * (1 + h)) - odft.energy_density(terms, rho, sig * (1 - h))) / (2 * h * sig)
        assert np.abs(vr - fr).max() < 1e-8 and np.abs(vs - fs).max() < 1e-7
    # closed-shell LYP compact form (the one the HIP kernel codes) == spin-resolved form
    a, b, c_, d = 0.04918, 0.132, 0.2533, 0.349
    t = rho ** (-1 / 3)
    Dn = 1 + d * t
    om = np.exp(-c_ * t) / Dn * rho ** (-11 / 3)
    dl = c_ * t + d * t / Dn
    cf = 0.3 * (3 * np.pi ** 2) ** (2 / 3)
    compact = -a * rho / Dn - a * b * om * (cf * rho ** (14 / 3) - rho ** 2 * sig * (1 / 24 + 7 * dl / 72))
    assert np.abs(compact - odft._lyp(rho / 2, rho / 2, sig / 4, sig / 4, sig / 4)).max() < 1e-15


def test_oracle_reproduces_committed_golden_vectors():
    from oracle import oracle as orc
    from mi355scf import fixtures
    g = np.load(os.path.join(os.path.dirname(__file__), "golden", "h2co_631gd_vectors.npz"))
    mol = _mol(fixtures.H2CO, "6-31g(d)")
    o = orc.Oracle(mol)
    S, T, V, dip = o.int1e()
    assert np.abs(S - g["S"]).max() < 1e-13 and np.abs(V - g["V"]).max() < 1e-12
    J, K = o.jk(g["D"], tol=0.0)
    assert np.abs(J - g["J"]).max() < 1e-11 and np.abs(K - g["K"]).max() < 1e-11


@pytest.mark.parametrize("formula,basis,e_lit,tol", [
    ("h2o", "cc-pvdz", -76.0268, 1e-4),     # literature RHF at the experimental geometry (r = 0.9572 A, 104.52 deg)
    ("h2o", "cc-pvtz", -76.0571, 1e-4),     #   (CCCBDB-style tabulations; UNVERIFIED-MEMORY, 4 decimals)
    ("h2o", "def2-tzvp", -76.0590, 2e-4),
    ("ch4", "cc-pvdz", -40.1987, 1e-4),     # r(CH) = 1.087 A, T_d
    ("ch4", "cc-pvtz", -40.2134, 1e-4),
    ("co", "cc-pvdz", -112.7493, 1e-4),     # r(CO) = 1.128 A (CCCBDB-style tabulation; UNVERIFIED-MEMORY, 4 decimals)
    ("co", "cc-pvtz", -112.7804, 1.5e-4),   #   pins the carbon AND oxygen cc-pVTZ tables in one molecule
])
def test_literature_rhf_energies_pin_the_remembered_tz_tables(formula, basis, e_lit, tol):
    """A wrong digit in a remembered exponent/coefficient moves these energies by far more than `tol`."""
    import math
    from oracle import oracle as orc
    if formula == "h2o":
        r, th = 0.9572, math.radians(104.52)
        atom = f"O 0 0 0; H {r * math.sin(th / 2):.6f} 0 {r * math.cos(th / 2):.6f}; H {-r * math.sin(th / 2):.6f} 0 {r * math.cos(th / 2):.6f}"
    elif formula == "co":
        atom = "C 0 0 0; O 0 0 1.128"
    else:
        a = 0.6276
        atom = f"C 0 0 0; H {a} {a} {a}; H {-a} {-a} {a}; H {-a} {a} {-a}; H {a} {-a} {-a}"
    res = orc.rhf(_mol(atom, basis))
    assert res["converged"] and abs(res["e_tot"] - e_lit) < tol, res["e_tot"]


def test_atomic_uhf_energies_and_hf_limit_brackets_pin_carbon_and_oxygen_tz_tables():
    """carbon/def2-TZVP and oxygen/cc-pVTZ.  (i) UHF energies of the 3P atoms in cc-pVTZ, remembered
    to 4 decimals (UNVERIFIED-MEMORY): C -37.6916, O -74.8118.  (ii) def2-TZVP has no remembered molecular value, so it is
    bracketed: the variational principle puts every basis-set energy ABOVE the Hartree-Fock limit (numerical HF: C atom UHF
    -37.6937, O atom UHF -74.8188, CH4 -40.2171, CO -112.7909 [MEM]); a wrong digit in a remembered exponent or contraction
    coefficient can only RAISE the energy, and def2-TZVP is known to sit at or slightly below cc-pVTZ for first-row
    Hartree-Fock energies, so `E_limit < E(def2-TZVP) < E(cc-pVTZ) + 0.5 mHa` is a two-sided pin a few mHa wide."""
    from oracle import oracle as orc
    from mi355scf.mole import Mole
    def atom_uhf(el, basis):
        return orc.uhf(Mole(atom=f"{el} 0 0 0", basis=basis, spin=2, verbose=0).build())[0]
    e_c, e_o = atom_uhf("C", "cc-pvtz"), atom_uhf("O", "cc-pvtz")
    assert abs(e_c - (-37.6916)) < 1e-4, e_c
    assert abs(e_o - (-74.8118)) < 1e-4, e_o
    for el, e_tz, e_lim in (("C", e_c, -37.6937), ("O", e_o, -74.8188)):
        e = atom_uhf(el, "def2-tzvp")
        assert e_lim < e < e_tz + 5e-4, (el, e)
    a = 0.6276
    ch4 = f"C 0 0 0; H {a} {a} {a}; H {-a} {-a} {a}; H {-a} {a} {-a}; H {a} {-a} {-a}"
    for atom, e_tz, e_lim in ((ch4, -40.2134, -40.2171), ("C 0 0 0; O 0 0 1.128", -112.7804, -112.7909)):
        res = orc.rhf(_mol(atom, "def2-tzvp"))
        assert res["converged"] and e_lim < res["e_tot"] < e_tz + 5e-4, res["e_tot"]


def test_oracle_uhf_and_spin_functionals_known_answers():
    """Open-shell checkers: H atom UHF energies (exact in the basis: STO-3G -0.46658185, cc-pVDZ -0.49927840 [MEM]);
    UHF == RHF for a closed shell; spin-polarised functionals reduce to the closed-shell forms at zeta = 0, LYP vanishes
    for a fully polarised density, and the PW92 / VWN5 uniform-gas energies match the tabulated values
    (PW92 Table: rs=1: -0.0598 / -0.0316, rs=2: -0.0448 / -0.0239 Ha for zeta = 0 / 1 [MEM])."""
    import numpy as np
    from mi355scf.mole import Mole
    from oracle import oracle as orc
    from oracle import dft as od
    for basis, ref in (("sto-3g", -0.46658185), ("cc-pvdz", -0.49927840)):
        m = Mole(atom="H 0 0 0", basis=basis, spin=1, verbose=0).build()
        assert abs(orc.uhf(m)[0] - ref) < 2e-8
    m = Mole(atom="O 0 0 0; H 0 -0.757 0.587; H 0 0.757 0.587", basis="6-31g", verbose=0).build()
    assert abs(orc.uhf(m)[0] - orc.rhf(m)["e_tot"]) < 1e-8
    rng = np.random.default_rng(0)
    rho = rng.uniform(0.01, 2.0, 64)
    sig = rng.uniform(0, 1.0, 64) * rho ** 2
    for name in ("B3LYP", "PBE", "LDA", "BLYP"):
        _h, terms = od.parse_xc(name)
        e0, vr, vs = od.eval_xc(terms, rho, sig)
        e1, d = od.eval_xc_spin(terms, rho / 2, rho / 2, sig / 4, sig / 4, sig / 4)
        assert np.abs(e0 - e1).max() < 1e-13 and np.abs(vr - d[0]).max() < 1e-12 and np.abs(vr - d[1]).max() < 1e-12
        assert np.abs(4 * vs - (d[2] + d[3] + d[4])).max() < 1e-11   # d/dsigma = (d_aa + d_ab + d_bb)/4 at zeta = 0
    e, _d = od.eval_xc_spin([(1.0, "lyp")], rho, 0 * rho, sig, 0 * rho, 0 * rho)
    assert np.abs(e).max() < 1e-14
    for rs, para, ferro in ((1.0, -0.0598, -0.0316), (2.0, -0.0448, -0.0239)):
        r = 3 / (4 * np.pi * rs ** 3)
        for fn in (od._pbe_c_spin, lambda a, b, *s: od._vwn5_spin(a, b)):
            e_p = np.real(fn(np.array([r / 2 + 0j]), np.array([r / 2 + 0j]), 0, 0, 0))[0] / r
            e_f = np.real(fn(np.array([r * (1 - 1e-12) + 0j]), np.array([r * 1e-12 + 0j]), 0, 0, 0))[0] / r
            assert abs(e_p - para) < 4e-4 and abs(e_f - ferro) < 4e-4


# ------------------------------------------------------------------------------------------------
# Derivative integrals of the oracle (the exact references of the GPU gradient tests, test_gpu_grad_oracle.py), pinned to
# fourth-order central differences of the oracle's own integrals and energies.
# ------------------------------------------------------------------------------------------------

def _fd4(f, h):
    """(-f(2h) + 8 f(h) - 8 f(-h) + f(-2h)) / 12h of a function of the step."""
    return (-f(2 * h) + 8 * f(h) - 8 * f(-h) + f(-2 * h)) / (12 * h)


def _displaced(mol, ia, x, h):
    R = mol.atom_coords().copy()
    R[ia, x] += h
    return mol.set_geom_(R, unit="Bohr", inplace=False)


def _one_shell_per_l(lmax):
    """Four atoms (He, Be, C, O: even electron count), each carrying one two-primitive shell of every l <= lmax; the exponents
    differ per atom.  Shell index of (atom a, l) = a * (lmax + 1) + l."""
    basis = {}
    for a, el in enumerate(("He", "Be", "C", "O")):
        basis[el] = [[l, [1.3 + 0.2 * a + 0.1 * l, 0.6], [0.45 + 0.05 * a, 0.5]] for l in range(lmax + 1)]
    atom = "He 0 0 0; Be 0.3 1.1 -0.4; C -0.9 0.2 0.8; O 0.5 -0.7 0.6"
    return _mol(atom, basis, unit="Bohr")


def test_eri_ip1_matches_finite_differences_all_classes_to_f():
    """orc_eri_ip1_shell for every (l1 l2|l3 l4) class up to f: shell i is the only shell of the quartet on atom 0, so moving atom 0
    moves exactly the differentiated shell.  The four centre derivatives sum to zero (translational invariance)."""
    from oracle import oracle as orc
    mol = _one_shell_per_l(3)
    o = orc.Oracle(mol)
    classes = [(a, b, c, d) for a in range(4) for b in range(4) for c in range(4) for d in range(4)]
    quart = {cl: (cl[0], 4 + cl[1], 8 + cl[2], 12 + cl[3]) for cl in classes}
    ana = {cl: o.eri_ip1_shell(*q) for cl, q in quart.items()}
    h = 1e-3
    worst = 0.0
    for x in range(3):
        blocks = {s: {cl: orc.Oracle(_displaced(mol, 0, x, s)).eri_shell(*q) for cl, q in quart.items()} for s in (2 * h, h, -h, -2 * h)}
        for cl in classes:
            fd = _fd4(lambda s: blocks[s][cl], h)
            err = np.abs(ana[cl][x] - fd).max() / max(1.0, np.abs(fd).max())
            worst = max(worst, err)
            assert err < 1e-8, (cl, x, err)
    for cl, (i, j, k, l) in quart.items():
        tot = (ana[cl] + o.eri_ip1_shell(j, i, k, l).transpose(0, 2, 1, 3, 4) + o.eri_ip1_shell(k, l, i, j).transpose(0, 3, 4, 1, 2)
               + o.eri_ip1_shell(l, k, i, j).transpose(0, 3, 4, 2, 1))
        assert np.abs(tot).max() < 1e-12 * max(1.0, np.abs(ana[cl]).max()), cl


def test_eri_ip1_g_shell_three_and_two_centre():
    """A g shell in the differentiated and in the plain positions of (ij|P 1) and (P 1|Q 1) with the exponent-0 unit function --
    how oracle/df.py uses it: l = 5 inside the derivative.  Also: the unit function's own derivative is exactly zero."""
    import math
    from oracle import oracle as orc
    basis = {"He": [[4, [1.1, 1.0]], [2, [0.8, 1.0]]], "Be": [[3, [0.9, 1.0]], [4, [0.7, 0.5], [2.1, 0.5]]]}

    def with_unit(m):
        class P:
            pass
        p = P()
        env = np.concatenate([m._env, [0.0, math.sqrt(4 * math.pi)]])
        p._atm, p._env, p.nao = m._atm, env, m.nao + 1
        p._bas = np.vstack([m._bas, [[0, 0, 1, 1, 0, len(m._env), len(m._env) + 1, 0]]]).astype(np.int32)
        return p
    mol = _mol("He 0 0 0; Be 0.4 -0.9 1.2", basis, unit="Bohr")
    u = mol.nbas
    sh = {(int(b[0]), int(b[1])): n for n, b in enumerate(mol._bas)}
    hg, hd, bf, bg = sh[0, 4], sh[0, 2], sh[1, 3], sh[1, 4]
    cases = [(hg, bf, bg, u), (bf, hg, hd, u), (bg, u, hg, u), (hg, u, bf, u), (hd, bg, bf, u), (bg, hd, hg, u)]
    o = orc.Oracle(with_unit(mol))
    h = 1e-3
    for (i, j, k, l) in cases:
        ana = o.eri_ip1_shell(i, j, k, l)
        ia = int(mol._bas[i, 0])
        assert all(int(mol._bas[s, 0]) != ia for s in (j, k) if s < u), "the moved atom must carry only shell i of the quartet"
        for x in range(3):
            fd = _fd4(lambda s: orc.Oracle(with_unit(_displaced(mol, ia, x, s))).eri_shell(i, j, k, l), h)
            assert np.abs(ana[x] - fd).max() < 1e-8 * max(1.0, np.abs(fd).max()), ((i, j, k, l), x)
    assert np.abs(o.eri_ip1_shell(u, 0, 3, u)).max() == 0.0


def test_df_gradient_oracle_matches_finite_differences():
    """oracle/df.py grad (Z3 and Z2 together) against differences of oracle/df.py integrals, water/6-31G(d): its generated
    auxiliary set reaches g."""
    from mi355scf import df
    from mi355scf.mole import Mole
    from oracle import df as odf
    mol = _mol(MOLECULES["h2o"], "6-31g(d)")

    def aux(m):
        return Mole(atom=[(s_, xyz) for s_, xyz in m._atom], basis=df.even_tempered_aux(m), unit="Bohr", verbose=0).build()
    am = aux(mol)
    assert am._bas[:, 1].max() == 4
    n, na = mol.nao, am.nao
    rng = np.random.default_rng(21)
    z3 = rng.standard_normal((n, n, na))
    z3 = 0.5 * (z3 + z3.transpose(1, 0, 2))
    a = rng.standard_normal((na, na))
    z2 = 0.5 * (a + a.T)
    g = odf.grad(mol, am, z3, z2)
    assert np.abs(g.sum(axis=0)).max() < 1e-10 * np.abs(g).max()

    def F(m):
        j3, j2 = odf.integrals(m, aux(m))
        return float((z3 * j3).sum() + (z2 * j2).sum())
    for x in range(3):   # the oxygen: orbital, auxiliary and g shells all move
        fd = _fd4(lambda s: F(_displaced(mol, 0, x, s)), 1e-3)
        assert abs(g[0, x] - fd) < 1e-8 * max(1.0, np.abs(g).max()), (x, g[0, x], fd)


def test_grad_eri_oracle_matches_finite_differences():
    """orc_grad_eri against differences of the oracle's own J/K energy 1/2 D.J[D] - hyb/4 (D.K[D] + M.K[M]), water/6-31G(d),
    random non-idempotent D and M, hyb 0 and 1, with and without M."""
    from oracle import oracle as orc
    mol = _mol(MOLECULES["h2o"], "6-31g(d)")
    n = mol.nao
    rng = np.random.default_rng(5)
    a, b = rng.standard_normal((n, n)), rng.standard_normal((n, n))
    D, M = a + a.T, b + b.T
    o = orc.Oracle(mol)

    def parts(m):
        om = orc.Oracle(m)
        J, K = om.jk(D, tol=0.0)
        _, KM = om.jk(M, tol=0.0)
        return np.array([0.5 * np.sum(D * J), -0.25 * np.sum(D * K), -0.25 * np.sum(M * KM)])
    fd = np.zeros((mol.natm, 3, 3))
    for ia in range(mol.natm):
        for x in range(3):
            fd[ia, x] = _fd4(lambda s: parts(_displaced(mol, ia, x, s)), 1e-3)
    for hyb in (0.0, 1.0):
        for spin in (None, M):
            g = o.grad_eri(D, spin, hyb=hyb)
            ref = fd[..., 0] + hyb * fd[..., 1] + (hyb * fd[..., 2] if spin is not None else 0.0)
            assert np.abs(g - ref).max() < 1e-8 * max(1.0, np.abs(ref).max()), (hyb, spin is not None, np.abs(g - ref).max())
            assert np.abs(g.sum(axis=0)).max() < 1e-11 * max(1.0, np.abs(g).max())
    # what a Schwarz threshold drops is reported separately and is part of the whole
    g, gs = o.grad_eri(D, M, hyb=1.0, qtol=1e-3)
    assert np.abs(gs).max() > 0 and np.abs(g - o.grad_eri(D, M, hyb=1.0)).max() == 0.0


def test_grad_1e_oracle_matches_finite_differences_with_ghost_atoms():
    """orc_int1e_ip contracted like mi_grad_1e (basis motion + Hellmann-Feynman term) against differences of orc_int1e, water with
    a ghost water: the ghost nuclei carry no charge but their basis functions move."""
    from oracle import oracle as orc
    mol = _mol("O 0 0 0; H 0 -0.757 0.587; H 0 0.757 0.587; Ghost:O 0.1 0.2 2.9; Ghost:H 0.7 0 3.5; Ghost:H -0.7 0.1 3.6",
               "6-31g(d)")
    assert list(mol._atm[:, 0]) == [8, 1, 1, 0, 0, 0]
    n = mol.nao
    rng = np.random.default_rng(6)
    a, b = rng.standard_normal((n, n)), rng.standard_normal((n, n))
    D, W = a + a.T, b + b.T
    g = orc.Oracle(mol).grad_1e(D, W)

    def E(m):
        S, T, V, _ = orc.Oracle(m).int1e()
        return float(np.sum(D * (T + V)) - np.sum(W * S))
    ref = np.array([[_fd4(lambda s: E(_displaced(mol, ia, x, s)), 1e-3) for x in range(3)] for ia in range(mol.natm)])
    assert np.abs(g - ref).max() < 1e-8 * max(1.0, np.abs(ref).max()), np.abs(g - ref).max()
    assert np.abs(g[3:]).max() > 1.0      # the ghost atoms' basis functions do feel forces
    assert np.abs(g.sum(axis=0)).max() < 1e-11 * np.abs(g).max()


def test_eval_ao_second_derivatives_match_finite_differences():
    """oracle/dft.py eval_ao(deriv=2) (xx, xy, xz, yy, yz, zz after value and gradient) against differences of deriv=1, and
    deriv=2's first four components equal deriv=1 exactly; water/cc-pVTZ (f shells)."""
    from oracle import dft as odft
    mol = _mol(MOLECULES["h2o"], "cc-pvtz")
    coords = np.random.default_rng(7).normal(size=(40, 3)) * 1.5
    a2 = odft.eval_ao(mol, coords, 2)
    assert a2.shape == (10, 40, mol.nao)
    assert np.array_equal(a2[:4], odft.eval_ao(mol, coords, 1))
    for m, (i, j) in enumerate([(0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)]):
        def d1(s):
            c = coords.copy()
            c[:, j] += s
            return odft.eval_ao(mol, c, 1)[1 + i]
        fd = _fd4(d1, 1e-4)
        assert np.abs(a2[4 + m] - fd).max() < 1e-8 * max(1.0, np.abs(fd).max()), (i, j)
