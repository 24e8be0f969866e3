"""CASSCF nuclear gradients on the GPU.

Kernel (`mi_grad_eri_pairs`: the two-particle density of every derivative quartet is the Hartree-Fock form plus
sum_k s_k Q^k_ab Q^k_cd) against the EXACT FP64 derivative integrals of the CPU oracle, which knows no pair term: the reference is
    orc.grad_eri(D, M or None, hyb) + sum_k s_k orc.grad_eri(Q^k, None, 0.0)
(the Coulomb-only gradient of a density Q is the gradient of 1/2 (Q|Q)).  Inputs and tolerance as in test_gpu_grad_oracle.py:
random symmetric O(1) matrices from fixed seeds, prepare_eri(1e-14), grad_dtol 1e-30, |g - g_ref| <= 1e-10 max(1, |g_ref|max) +
2 (drop_D + sum_k |s_k| drop_k) with `drop` the oracle's own value of the Schwarz-skipped part.

Driver (`mc.nuc_grad_method()`): the RHF limit, central finite differences of the CASSCF energy, and an optimisation.
Each test prints its figures (pytest -rP shows them)."""
import ctypes
import functools
import re

import numpy as np
import pytest
import torch

from conftest import MOLECULES

pytestmark = pytest.mark.gpu

QTOL = 1e-14
DTOL = 1e-30
GHOST = MOLECULES["h2o"] + "; Ghost:O 0.1 0.2 2.9; Ghost:H 0.7 0 3.5; Ghost:H -0.7 0.1 3.6"
SYSTEMS = {"h2o/cc-pvtz": (MOLECULES["h2o"], "cc-pvtz"), "h2co/6-31g(d)": (MOLECULES["h2co"], "6-31g(d)"),
           "h2o+ghost/cc-pvdz": (GHOST, "cc-pvdz")}
S3 = (0.7, -1.3, 0.4)


def _mol(atom, basis):
    from mi355scf.mole import Mole
    return Mole(atom=atom, basis=basis, verbose=0).build()


def _sym(n, seed):
    a = np.random.default_rng(seed).standard_normal((n, n))
    return a + a.T


def _dev(x, eng):
    return torch.as_tensor(np.ascontiguousarray(x), dtype=torch.float64, device=eng.device)


_REF = {}


def _oracle(key, mol, D, M, Qs, s):
    """{(hyb, spin): (g_ref, tol)} for hyb 0 and 1 (E2 is linear in hyb; without exchange the spin density does not enter)."""
    if key not in _REF:
        from oracle import oracle as orc
        o = orc.Oracle(mol)
        gJ, dJ = o.grad_eri(D, None, hyb=0.0, qtol=QTOL)
        gD, dD = o.grad_eri(D, None, hyb=1.0, qtol=QTOL)
        gM, dM = (o.grad_eri(D, M, hyb=1.0, qtol=QTOL) if M is not None else (gD, dD))
        gQ, dropQ = np.zeros_like(gJ), 0.0
        for sk, Q in zip(s, Qs):
            g, d = o.grad_eri(Q, None, hyb=0.0, qtol=QTOL)
            gQ += sk * g
            dropQ += abs(sk) * np.abs(d).max()
        drop = max(np.abs(d).max() for d in (dJ, dD, dM))
        _REF[key] = (gJ, gD - gJ, gM - gJ, gQ, drop + dropQ)
    return _REF[key]


def _ref(key, mol, D, M, Qs, s, hyb, spin):
    gJ, gKD, gKM, gQ, drop = _oracle(key, mol, D, M, Qs, s)
    g = gJ + hyb * (gKM if spin else gKD) + gQ
    return g, 1e-10 * max(1.0, np.abs(g).max()) + 2 * drop


def _grad_pairs(eng, mol, D, M, hyb, Qs, s, rank=0, nranks=1):
    """`mi_grad_eri_pairs` itself (`Engine.grad_eri` reaches the pair term through `mi_grad_eri_xpairs`)."""
    from mi355scf import engine
    g = torch.zeros(mol.natm, 3, dtype=torch.float64, device=eng.device)
    Dd, Md = _dev(D, eng), (_dev(M, eng) if M is not None else None)
    Q = _dev(np.array(Qs), eng) if len(s) else None
    s = np.ascontiguousarray(np.asarray(s, dtype=np.float64))
    engine._check(engine.lib().mi_grad_eri_pairs(eng._h, Dd.data_ptr(), Md.data_ptr() if Md is not None else None, float(hyb),
                                                 Q.data_ptr() if Q is not None else None,
                                                 s.ctypes.data_as(ctypes.POINTER(ctypes.c_double)) if s.size else None, int(s.size),
                                                 g.data_ptr(), rank, nranks, eng._stream()))
    return g.cpu().numpy()


# ---- 1. the kernel against exact integrals ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spin", [False, True])
@pytest.mark.parametrize("system", list(SYSTEMS))
def test_pair_kernel_matches_exact_oracle(system, spin):
    from mi355scf.engine import Engine
    mol = _mol(*SYSTEMS[system])
    n = mol.nao
    D, M = _sym(n, 31), _sym(n, 32)
    Qs = [_sym(n, 71 + k) for k in range(3)]
    eng = Engine(mol)
    eng.prepare_eri(QTOL)
    eng.set_option("grad_dtol", DTOL)
    Ms = M if spin else None
    worst = 0.0
    for hyb in (0.0, 1.0):
        ref, tol = _ref(system, mol, D, M, Qs, S3, hyb, spin)
        g = _grad_pairs(eng, mol, D, Ms, hyb, Qs, S3)
        err = np.abs(g - ref).max()
        worst = max(worst, err / max(1.0, np.abs(ref).max()))
        print(f"{system} spin={spin} hyb={hyb}: |g - g_ref| = {err:.2e} (tol {tol:.1e}, |g_ref|max {np.abs(ref).max():.1f})")
        assert err < tol, (system, spin, hyb, err, tol)
        if hyb == 1.0:
            parts = [_grad_pairs(eng, mol, D, Ms, hyb, Qs, S3, r, 3) for r in range(3)]
            assert all(np.abs(p).max() > 0 for p in parts)
            err3 = np.abs(sum(parts) - ref).max()
            print(f"{system} spin={spin}: three-way rank split |sum - g_ref| = {err3:.2e}")
            assert err3 < tol, (system, spin, "rank split", err3, tol)
    # K = 0 through the new entry is the plain entry (same kernels; the atomics' summation order is the only difference)
    g0 = _grad_pairs(eng, mol, D, Ms, 1.0, [], [])
    from mi355scf import engine
    g1 = torch.zeros(mol.natm, 3, dtype=torch.float64, device=eng.device)
    Dd, Md = _dev(D, eng), (_dev(Ms, eng) if spin else None)
    engine._check(engine.lib().mi_grad_eri_sharded(eng._h, Dd.data_ptr(), Md.data_ptr() if spin else None, 1.0, g1.data_ptr(), 0, 1, eng._stream()))
    g1 = g1.cpu().numpy()
    d0 = np.abs(g0 - g1).max()
    print(f"{system} spin={spin}: K = 0 against mi_grad_eri_sharded {d0:.2e}; worst relative error {worst:.2e}")
    assert d0 <= 1e-13 * max(1.0, np.abs(g1).max())


def test_pair_entry_refuses_bad_arguments():
    from mi355scf.engine import Engine
    mol = _mol(MOLECULES["h2o"], "sto-3g")
    n = mol.nao
    eng = Engine(mol)
    eng.prepare_eri()
    D = _sym(n, 1)
    with pytest.raises(RuntimeError, match="finite"):
        _grad_pairs(eng, mol, D, None, 1.0, [_sym(n, 2)], [float("nan")])
    with pytest.raises(RuntimeError, match="136"):
        _grad_pairs(eng, mol, D, None, 1.0, [D] * 137, [1.0] * 137)
    with pytest.raises(ValueError, match="pairs"):
        g = torch.zeros(mol.natm, 3, dtype=torch.float64, device=eng.device)
        eng.grad_eri(_dev(D, eng), 1.0, g, pairs=(_dev(np.zeros((1, n, n + 1)), eng), [1.0]))


# ---- 2. every route of the gradient on benzene/cc-pVDZ (114 AOs, 54 shells) -------------------------------------------------------
DEFAULTS = {"eri_tpq": 1, "tpq_maxprim": 32, "grad_rows": 1, "grad_rows_min": 20, "grad_rows_g32": 1, "grad_live": 1,
            "task_table": 1, "grad_work_mb": 1024}
ROUTES = [
    ("default", {}, 1.0),
    ("tpq off", {"eri_tpq": 0}, 0.0),
    ("pipeline only", {"grad_rows": 0}, 0.0),
    ("rows everywhere, g32", {"grad_rows_min": 1, "grad_rows_g32": 1}, 1.0),
    ("rows everywhere, no g32", {"grad_rows_min": 1, "grad_rows_g32": 0}, 0.0),
    ("screen per wave, small batches", {"grad_live": 0, "task_table": 0, "grad_rows": 0, "eri_tpq": 0, "grad_work_mb": 1}, 1.0),
]
_LINE = re.compile(r"\[mi355\] grad class \((\d\d)\|(\d\d)\) perm \d: (\d+) quartets, [0-9.]+ s(?: \((thread per quartet|row kernel, "
                   r"\d rows x (\d+) lanes)\))?$")
_LIVE = re.compile(r"\[mi355\] grad class pair \((\d\d)\|(\d\d)\): \d+ of (\d+) quartets live$")


def _routes(err):
    out = {"tpq": set(), "rows": set(), "rows32": set(), "pipeline": set(), "live": set(), "pipeline_big": set()}
    for line in err.splitlines():
        m = _LINE.search(line)
        if m:
            key, big = (m.group(1), m.group(2)), int(m.group(3)) >= 65536
            kind = m.group(4) or ""
            if kind.startswith("thread"):
                out["tpq"].add(key)
            elif kind.startswith("row"):
                out["rows"].add(key)
                if m.group(5) == "32":
                    out["rows32"].add(key)
            else:
                out["pipeline"].add(key)
                if big:
                    out["pipeline_big"].add(key)
        m = _LIVE.search(line)
        if m:
            out["live"].add((m.group(1), m.group(2)))
    return out


def _check_routes(name, r, base):
    if name == "default":
        assert r["tpq"] and r["rows"] and r["live"] and r["rows32"], r
    elif name == "tpq off":
        assert not r["tpq"] and r["rows"] and r["live"], r
    elif name == "pipeline only":
        assert not r["rows"] and r["pipeline"] and r["live"], r
    elif name == "rows everywhere, g32":
        assert len(r["rows"]) > len(base["rows"]) and r["rows32"], (r["rows"], base["rows"])
    elif name == "rows everywhere, no g32":
        assert len(r["rows"]) > len(base["rows"]) and not r["rows32"], r["rows"]
    elif name == "screen per wave, small batches":
        assert not r["live"] and not r["rows"] and not r["tpq"] and r["pipeline_big"], r


def test_pair_kernel_every_route_matches_exact_oracle(monkeypatch, capfd):
    from mi355scf import fixtures
    from mi355scf.engine import Engine
    mol = _mol(fixtures.BENZENE, "cc-pvdz")
    n = mol.nao
    assert n == 114 and mol.nbas == 54
    D = _sym(n, 41)
    Qs, s = [_sym(n, 81), _sym(n, 82)], (0.7, -1.3)
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
            g = _grad_pairs(eng, mol, D, None, hyb, Qs, s)
            r = _routes(capfd.readouterr().err)
            base = base or r
            ref, tol = _ref("benzene", mol, D, None, Qs, s, hyb, False)     # one oracle reference, cached across the routes
            err = np.abs(g - ref).max()
            report.append(f"route '{name}': classes on tpq {len(r['tpq'])}, rows {len(r['rows'])} (g32 {len(r['rows32'])}), pipeline "
                          f"{len(r['pipeline'])}; live lists {len(r['live'])}; |g - g_ref| = {err:.2e} (tol {tol:.1e})")
            assert err < tol, (name, err, tol)
            _check_routes(name, r, base)
    finally:
        eng.set_option("grad_rows_g32", 1)     # process-wide, not per context
        print("\n".join(report))


# ---- 3. the screening sees the pair term ----------------------------------------------------------------------------------------
def test_screening_bound_includes_the_pair_term():
    """D = 0: every quartet's Hartree-Fock density block vanishes; a bound without qmax_ab qmax_cd would skip them all."""
    from mi355scf.engine import Engine
    from oracle import oracle as orc
    mol = _mol(MOLECULES["h2o"], "cc-pvdz")
    n = mol.nao
    Q, s = _sym(n, 91), 0.7
    eng = Engine(mol)
    eng.prepare_eri(QTOL)
    eng.set_option("grad_dtol", 1e-10)
    g = _grad_pairs(eng, mol, np.zeros((n, n)), None, 1.0, [Q], [s])
    ref = s * orc.Oracle(mol).grad_eri(Q, None, hyb=0.0, qtol=QTOL)[0]
    err = np.abs(g - ref).max()
    print(f"D = 0, K = 1, grad_dtol 1e-10: |g|max = {np.abs(g).max():.3f}, |g - s g_J(Q)| = {err:.2e}")
    assert np.abs(ref).max() > 1e-2
    assert err <= 1e-6 * max(1.0, np.abs(ref).max())


# ---- driver -----------------------------------------------------------------------------------------------------------------------
H2_14 = "H 0 0 0; H 0 0 1.4"
H2_074 = "H 0 0 0; H 0 0 0.74"


def _rhf(mol, dm0=None, conv_tol_grad=None):
    from pyscf import scf
    mf = scf.RHF(mol)
    mf.conv_tol = 1e-11
    mf.conv_tol_grad = conv_tol_grad
    mf.kernel(dm0=dm0)
    assert mf.converged
    return mf


def _casscf(mf, ncas, nelecas, **kw):
    from pyscf import mcscf
    mc = mcscf.CASSCF(mf, ncas, nelecas)
    mc.conv_tol, mc.conv_tol_grad, mc.max_cycle_macro = 1e-11, 1e-7, 200
    for k, v in kw.items():
        setattr(mc, k, v)
    return mc


# ---- 4. RHF limit -------------------------------------------------------------------------------------------------------------------
def test_fully_occupied_active_space_gives_the_rhf_gradient():
    """The two gradients are the same expectation value only at a stationary point: `grad.Gradients` contracts W = 1/2 D F D (the
    occupied-occupied block of F), this driver C . 1/2 (F + F^T) . C^T, which also holds the occupied-virtual block F_ia -- the SCF's
    own residual.  They differ by (residual) x (orbital response, O(1)), so the 1e-8 bound needs the SCF's orbital gradient below
    it: conv_tol = 1e-11 alone stops at |g| < sqrt(conv_tol) = 3e-6 (measured difference there: 4.9e-8), hence conv_tol_grad = 1e-8."""
    from pyscf import gto
    mol = gto.M(atom=MOLECULES["h2o"], basis="6-31g(d)", verbose=0)
    mf = _rhf(mol, conv_tol_grad=1e-8)
    g_rhf = mf.nuc_grad_method().kernel()
    mc = _casscf(mf, 1, 2)
    mc.kernel()
    assert mc.converged and abs(mc.e_tot - mf.e_tot) < 1e-9
    grad = mc.nuc_grad_method()
    g = grad.kernel()
    R = mol.atom_coords()
    d, net, torque = np.abs(g - g_rhf).max(), np.abs(g.sum(axis=0)).max(), np.abs(np.cross(R, g).sum(axis=0)).max()
    print(f"CAS(2,1) water: K = {grad.npairs}, |g - g_RHF| = {d:.2e}, |sum g| = {net:.2e}, |sum R x g| = {torque:.2e}")
    assert d < 1e-8 and net < 1e-8 and torque < 1e-7


# ---- 5. finite differences of the CASSCF energy -------------------------------------------------------------------------------------
FD_STEP = 2e-3
FD_CASES = {"h2o-cas44": ("h2o", "6-31g(d)", 4, 4, None, 2), "h2co-cas22": ("h2co", "6-31g(d)", 2, 2, (7, 9), 2),
            "h2-cas22": ("h2", "6-31g(d,p)", 2, 2, None, 1)}


def _directions(R, ndir, seed):
    """Unit displacement directions [natm, 3]: the breathing mode about the centroid (totally symmetric: it keeps the point group;
    for a diatomic it is the bond direction) and one from a fixed seed."""
    u = R - R.mean(axis=0)
    out = [u / np.linalg.norm(u)]
    if ndir > 1:
        v = np.random.default_rng(seed).standard_normal(R.shape)
        out.append(v / np.linalg.norm(v))
    return out


@pytest.mark.parametrize("case", list(FD_CASES))
def test_gradient_matches_finite_differences_of_the_energy(case):
    from pyscf import gto
    from mi355scf.casscf_grad import lowdin_orthonormalize
    name, basis, ncas, nelecas, caslst, ndir = FD_CASES[case]
    mol = gto.M(atom=MOLECULES.get(name, H2_14), basis=basis, verbose=0)
    mf = _rhf(mol)
    mc = _casscf(mf, ncas, nelecas)
    mc.kernel(mc.sort_mo(list(caslst)) if caslst else None)
    assert mc.converged
    grad = mc.nuc_grad_method()
    assert grad.algorithm == "pairs"
    g = grad.kernel()
    K = grad.npairs
    loop = mc.nuc_grad_method()
    loop.algorithm = "loop"
    g_loop = loop.kernel()
    d_alg = np.abs(g - g_loop).max()
    print(f"{case}: E = {mc.e_tot:.10f}, K = {K}, |g|max = {np.abs(g).max():.6f}, |pairs - loop| = {d_alg:.2e}, "
          f"timings pairs {grad.timing['grad_eri']:.3f} s, loop {loop.timing['grad_eri']:.3f} s")
    assert d_alg < 1e-9
    if case == "h2o-cas44":
        assert K > 0
    mo, ci, dm0 = np.array(mc.mo_coeff), mc.ci, mf.make_rdm1()
    R = mol.atom_coords()
    tol = 5e-6 * max(1.0, np.abs(g).max())
    for i, u in enumerate(_directions(R, ndir, 17)):
        e = []
        for sign in (1.0, -1.0):
            mol_d = mol.set_geom_(R + sign * FD_STEP * u, unit="Bohr", inplace=False)
            mol_d.verbose = 0
            mf_d = _rhf(mol_d, dm0)
            mc_d = _casscf(mf_d, ncas, nelecas, stability_check=False)
            mc_d.kernel(lowdin_orthonormalize(mo, mf_d.get_ovlp()), ci0=ci)
            assert mc_d.converged
            e.append(mc_d.e_tot)
        fd = (e[0] - e[1]) / (2 * FD_STEP)
        an = float(np.sum(g * u))
        print(f"{case} direction {i}: analytic {an:+.9f}, finite difference {fd:+.9f}, difference {an - fd:+.2e} (tol {tol:.1e})")
        assert abs(an - fd) < tol, (case, i, an, fd)


# ---- 6. optimisation ----------------------------------------------------------------------------------------------------------------
def test_optimize_h2_casscf():
    from pyscf import gto
    from pyscf.geomopt.geometric_solver import optimize
    mol = gto.M(atom=H2_074, basis="6-31g(d,p)", verbose=0)
    r_rhf = optimize(_rhf(mol))
    assert r_rhf._opt_converged
    mc = _casscf(_rhf(mol), 2, 2)
    e0 = mc.kernel()[0]
    seen = {}

    def callback(env):
        seen["scanner"] = env["energy_grad"]
        seen.setdefault("e", []).append(env["e"])
    mol_opt = optimize(mc, callback=callback)
    assert mol_opt._opt_converged
    assert seen["scanner"].converged and mc.converged
    g = mc.nuc_grad_method().kernel()
    bond = lambda m: float(np.linalg.norm(m.atom_coords()[0] - m.atom_coords()[1]))
    print(f"H2 CAS(2,2)/6-31G(d,p): {mol_opt._opt_steps} steps, E {e0:.8f} -> {mc.e_tot:.8f}, r = {bond(mol_opt):.5f} Bohr "
          f"(RHF {bond(r_rhf):.5f}), max|g| = {np.abs(g).max():.2e}")
    assert np.abs(g).max() < 4.5e-4
    assert mc.e_tot <= e0 and seen["e"][-1] <= e0
    assert np.abs(mc.mol.atom_coords() - mol_opt.atom_coords()).max() < 1e-12
    assert bond(mol_opt) > bond(r_rhf) + 1e-3
