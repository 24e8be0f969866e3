"""The nuclear-gradient kernels against EXACT FP64 derivative integrals of the CPU oracle (orc_grad_eri, orc_int1e_ip,
oracle/df.py grad, oracle/dft.py eval_ao(deriv=2); pinned to finite differences in test_oracle_known_answers.py).

Inputs are random symmetric, non-idempotent D, M, W, Z3, Z2 of O(1) from fixed seeds, so every quartet matters.  The target is
|g - g_ref| <= 1e-10 max(1, |g_ref|max), where g_ref sums every unique quartet without screening.  The GPU skips two kinds of
quartets:
  * Schwarz, q_ab q_cd < 1e-14 (prepare_eri): the oracle evaluates exactly the part of its gradient that comes from those
    quartets (orc_grad_eri's `qtol` output, same q definition), and its size is added to the tolerance.
  * density, q_ab q_cd max|G| < grad_dtol = DTOL (1e-30; it must be > 0, or the live-quartet list never runs): every element of
    a skipped derivative block is below (2 a_max + l) q_ab q_cd ~ 1e5 q_ab q_cd for these bases, times |G| <= max|G|, so each
    skipped quartet moves the gradient by less than 1e5 * 100 elements * DTOL = 1e-23, and the ~1e6 quartets by < 1e-16.
Each test prints its worst error (pytest -rP shows it).
"""
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


def _mol(atom, basis):
    from mi355scf.mole import Mole
    return Mole(atom=atom, basis=basis, verbose=0).build()


def _sym(n, seed):
    a = np.random.default_rng(seed).standard_normal((n, n))
    return a + a.T


def _dev(x, eng):
    return torch.as_tensor(np.ascontiguousarray(x), device=eng.device)


_REF = {}


def _oracle_eri(key, mol, D, M):
    """(g_J, g_K[D], g_K[D] + g_K[M], |dropped part|max): E2 is linear in hyb, g(hyb) = g_J + hyb g_K."""
    if key not in _REF:
        from oracle import oracle as orc
        o = orc.Oracle(mol)
        gJ, sJ = o.grad_eri(D, None, hyb=0.0, qtol=QTOL)
        gD, sD = o.grad_eri(D, None, hyb=1.0, qtol=QTOL)
        gM, sM = o.grad_eri(D, M, hyb=1.0, qtol=QTOL)
        drop = max(np.abs(s).max() for s in (sJ, sD, sM))
        _REF[key] = (gJ, gD - gJ, gM - gJ, drop)
    return _REF[key]


def _ref(key, mol, D, M, hyb, spin):
    gJ, gKD, gKM, drop = _oracle_eri(key, mol, D, M)
    g = gJ + hyb * (gKM if spin else gKD)
    # the dropped part enters at most with weight max(1, hyb) (it is the sum of J- and K-parts of the skipped quartets)
    return g, 1e-10 * max(1.0, np.abs(g).max()) + 2 * drop


def _grad_eri(eng, mol, D, M, hyb, rank=0, nranks=1):
    g = torch.zeros(mol.natm, 3, dtype=torch.float64, device=eng.device)
    eng.grad_eri(_dev(D, eng), hyb, g, spin_density=_dev(M, eng) if M is not None else None, rank=rank, nranks=nranks)
    return g.cpu().numpy()


@pytest.mark.parametrize("spin", [False, True])
@pytest.mark.parametrize("system", list(SYSTEMS))
def test_grad_eri_matches_exact_oracle(system, spin):
    """mi_grad_eri_sharded, closed shell and with a spin density, hyb 0 / 0.2 / 1, and a three-way rank split whose partial
    gradients add up to the whole."""
    from mi355scf.engine import Engine
    mol = _mol(*SYSTEMS[system])
    n = mol.nao
    D, M = _sym(n, 31), _sym(n, 32)
    eng = Engine(mol)
    eng.prepare_eri(QTOL)
    eng.set_option("grad_dtol", DTOL)
    worst = 0.0
    for hyb in (0.0, 0.2, 1.0):
        ref, tol = _ref(system, mol, D, M, hyb, spin)
        g = _grad_eri(eng, mol, D, M if spin else None, hyb)
        err = np.abs(g - ref).max()
        worst = max(worst, err / max(1.0, np.abs(ref).max()))
        assert err < tol, (system, spin, hyb, err, tol)
        if hyb == 0.2:
            parts = [_grad_eri(eng, mol, D, M if spin else None, hyb, r, 3) for r in range(3)]
            assert all(np.abs(p).max() > 0 for p in parts)
            assert np.abs(sum(parts) - ref).max() < tol, (system, spin, "rank split")
    print(f"grad_eri {system} spin={spin}: worst |g - g_ref| / max(1, |g_ref|) = {worst:.2e}")


# --- every route of mi_grad_eri on benzene/cc-pVDZ (114 AOs, 54 shells, class pairs up to 251k tasks) ----------------------
DEFAULTS = {"eri_tpq": 1, "tpq_maxprim": 32, "grad_rows": 1, "grad_rows_min": 20, "grad_rows_g32": 1, "grad_live": 1,
            "task_table": 1, "grad_work_mb": 1024, "tpq_min_tasks": 32768}
# (name, options on top of DEFAULTS, hyb): the routes each one must show are asserted in _check_routes
ROUTES = [
    ("default", {}, 1.0),
    ("tpq off", {"eri_tpq": 0}, 0.2),
    ("tpq deep", {"tpq_maxprim": 1e9}, 1.0),
    ("pipeline only", {"grad_rows": 0}, 0.2),
    ("rows everywhere, g32", {"grad_rows_min": 1, "grad_rows_g32": 1}, 1.0),
    ("rows everywhere, no g32", {"grad_rows_min": 1, "grad_rows_g32": 0}, 0.2),
    ("task table (no live list)", {"grad_live": 0, "eri_tpq": 0}, 1.0),
    ("screen per wave, small batches", {"grad_live": 0, "task_table": 0, "grad_rows": 0, "eri_tpq": 0, "grad_work_mb": 1}, 0.2),
]
_LINE = re.compile(r"\[mi355\] grad class \((\d\d)\|(\d\d)\) perm \d: (\d+) quartets, [0-9.]+ s(?: \((thread per quartet|row kernel, "
                   r"\d rows x (\d+) lanes)\))?$")
_LIVE = re.compile(r"\[mi355\] grad class pair \((\d\d)\|(\d\d)\): \d+ of (\d+) quartets live$")


def _routes(err):
    """{route: set of derivative classes (l1 l2|lc ld), ...; "live": class pairs with a live list} from the MI355_DEBUG lines."""
    out = {"tpq": set(), "rows": set(), "rows32": set(), "pipeline": set(), "live": set(), "pipeline_big": set(), "rows_big": set()}
    for line in err.splitlines():
        m = _LINE.search(line)
        if m:
            key, big = (m.group(1), m.group(2)), int(m.group(3)) >= 65536
            kind = m.group(4) or ""
            if kind.startswith("thread"):
                out["tpq"].add(key)
            elif kind.startswith("row"):
                out["rows"].add(key)
                if big:
                    out["rows_big"].add(key)
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
    elif name == "tpq deep":
        assert len(r["tpq"]) > len(base["tpq"]), (r["tpq"], base["tpq"])
    elif name == "pipeline only":
        assert not r["rows"] and r["pipeline"] and r["live"], r
    elif name == "rows everywhere, g32":
        assert len(r["rows"]) > len(base["rows"]) and r["rows32"], (r["rows"], base["rows"])
    elif name == "rows everywhere, no g32":
        assert len(r["rows"]) > len(base["rows"]) and not r["rows32"], r["rows"]
    elif name == "task table (no live list)":
        # ntask >= 65536 without a live list: the launches walk the precomputed task table
        assert not r["live"] and not r["tpq"] and (r["rows_big"] or r["pipeline_big"]), r
    elif name == "screen per wave, small batches":
        # grad_work_mb 1 -> 8 MiB per buffer: the 251k-task (p s|s s) pair needs several batches
        assert not r["live"] and not r["rows"] and r["pipeline_big"], r


def test_grad_eri_every_route_matches_exact_oracle(monkeypatch, capfd):
    from mi355scf import fixtures
    from mi355scf.engine import Engine
    mol = _mol(fixtures.BENZENE, "cc-pvdz")
    n = mol.nao
    assert n == 114 and mol.nbas == 54
    D, M = _sym(n, 41), _sym(n, 42)
    eng = Engine(mol)
    eng.prepare_eri(QTOL)
    monkeypatch.setenv("MI355_DEBUG", "1")
    base = None
    worst = 0.0
    report = []     # printed at the end: capfd.readouterr() would swallow what is printed inside the loop
    try:
        for name, opts, hyb in ROUTES:
            for k, v in {**DEFAULTS, **opts, "grad_dtol": DTOL}.items():
                eng.set_option(k, v)
            capfd.readouterr()
            g = _grad_eri(eng, mol, D, M, hyb)
            r = _routes(capfd.readouterr().err)
            base = base or r
            ref, tol = _ref("benzene", mol, D, M, hyb, True)
            err = np.abs(g - ref).max()
            worst = max(worst, err / max(1.0, np.abs(ref).max()))
            report.append(f"route '{name}': derivative classes on tpq {len(r['tpq'])}, rows {len(r['rows'])} (g32 {len(r['rows32'])}), "
                          f"pipeline {len(r['pipeline'])}; live lists {len(r['live'])}; |g - g_ref| = {err:.2e} (tol {tol:.1e})")
            assert err < tol, (name, err, tol)
            _check_routes(name, r, base)
    finally:
        eng.set_option("grad_rows_g32", 1)     # process-wide, not per context
    print("\n".join(report))
    print(f"routes: worst |g - g_ref| / max(1, |g_ref|) = {worst:.2e}")


# --- every class of every route, inside and beyond the Rys root tables ----------------------------------------------------
def _ne(la, lb):
    return sum((e + 1) * (e + 2) // 2 for e in range(la, la + lb + 1))


def test_grad_eri_every_class_on_every_route_beyond_the_root_tables(monkeypatch, capfd):
    """The synthetic s..f molecule with its ghost centre at (9, -5, 3) Bohr (test_gpu_eri_elements.synthetic_mol("far"): every
    derivative class (l1 l2|lc ld), l <= 3, that mi_grad_eri can launch, Rys arguments from 0 to 260, see rys_branch_coverage): every class of the
    thread-per-quartet switch on that kernel (`tpq_min_tasks = 1`), every class with a row kernel there (with and without two
    quartets per wave), and all of them on the Rys -> hand-over -> contraction pipeline.

    Observed on the MI355X: |g - g_ref| = 7.3e-11 .. 7.9e-11 of |g_ref|max 283 on the four routes (bound 2.8e-8)."""
    from mi355scf.engine import Engine
    from test_gpu_eri_elements import rys_branch_coverage, switch_classes, synthetic_mol
    mol = synthetic_mol("far")
    cover = rys_branch_coverage([synthetic_mol("near"), mol], extra=1)
    n = mol.nao
    D, M = _sym(n, 71), _sym(n, 72)
    # The derivative classes (l1 l2|lc ld) a molecule can show: class pairs (B | Kc), B >= Kc in the order of the pair classes,
    # derivative on B's second shell, on Kc's first and on Kc's second (the fourth force follows from the other three).  131 of
    # the 160 ordered classes, all of them here.  Nine classes of the thread-per-quartet switch are not among them -- (ps|ss),
    # (ds|ss), (ds|ps), (ds|pp), (dp|ss), (dp|ps), (fs|ss), (fs|ps), (fp|ss) never get a launch from mi_grad_eri.
    pairs = [(a, b) for a in range(4) for b in range(a + 1)]
    every = set()
    for i, B in enumerate(pairs):
        for Kc in pairs[:i + 1]:
            every |= {(B[1], B[0]) + Kc, Kc + B, (Kc[1], Kc[0]) + B}
    switch = switch_classes("TPQG_CASE")
    tpq = switch & every
    rows = {k for k in every if k[2:] in switch_classes("ROWS_CASE") and _ne(k[0] + 1, k[1]) + (_ne(k[0] - 1, k[1]) if k[0] else 0) <= 192}
    assert len(every) == 131 and len(switch - every) == 9 and len(tpq) == 28 and len(rows) == 99
    as_key = lambda ks: {(f"{a}{b}", f"{c}{d}") for a, b, c, d in ks}
    forced = {"tpq_min_tasks": 1, "tpq_maxprim": 1e9}
    routes = [("thread per quartet", forced),
              ("rows, g32", {"eri_tpq": 0, "grad_rows_min": 1, "grad_rows_g32": 1}),
              ("rows, no g32", {"eri_tpq": 0, "grad_rows_min": 1, "grad_rows_g32": 0}),
              ("pipeline", {"eri_tpq": 0, "grad_rows": 0})]
    # _ref's bound at hyb = 1 with the spin density, from ONE oracle call (4 s) instead of _oracle_eri's three
    from oracle import oracle as orc
    ref, dropped = orc.Oracle(mol).grad_eri(D, M, hyb=1.0, qtol=QTOL)
    tol = 1e-10 * max(1.0, np.abs(ref).max()) + 2 * np.abs(dropped).max()
    eng = Engine(mol)
    eng.prepare_eri(QTOL)
    monkeypatch.setenv("MI355_DEBUG", "1")
    report = []
    try:
        for name, opts in routes:
            for k, v in {**DEFAULTS, **opts, "grad_dtol": DTOL}.items():
                eng.set_option(k, v)
            capfd.readouterr()
            g = _grad_eri(eng, mol, D, M, 1.0)
            r = _routes(capfd.readouterr().err)
            err = np.abs(g - ref).max()
            report.append(f"route '{name}': classes on tpq {len(r['tpq'])}, rows {len(r['rows'])} (g32 {len(r['rows32'])}), pipeline "
                          f"{len(r['pipeline'])}; |g - g_ref| = {err:.2e} of {np.abs(ref).max():.1f} (tol {tol:.1e})")
            assert err < tol, (name, err, tol)
            assert r["tpq"] | r["rows"] | r["pipeline"] == as_key(every), name
            if name == "thread per quartet":
                assert r["tpq"] == as_key(tpq), sorted(r["tpq"] ^ as_key(tpq))
            elif name.startswith("rows"):
                assert not r["tpq"] and r["rows"] == as_key(rows), sorted(r["rows"] ^ as_key(rows))
                assert bool(r["rows32"]) == (name == "rows, g32")
            else:
                assert not r["tpq"] and not r["rows"] and r["pipeline"] == as_key(every)
    finally:
        for k, v in DEFAULTS.items():
            eng.set_option(k, v)                   # grad_rows_g32 is process-wide, not per context
    print("\n".join(report))
    print(f"x range per root count: {cover}")


# --- one-electron -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("system", ["h2o/cc-pvtz", "h2co/6-31g(d)", "benzene/cc-pvdz", "h2o+ghost/cc-pvdz"])
def test_grad_1e_matches_exact_oracle(system):
    """mi_grad_1e (basis motion and the Hellmann-Feynman term; ghost nuclei: no operator, moving basis functions)."""
    from mi355scf import fixtures
    from mi355scf.engine import Engine
    from oracle import oracle as orc
    atom, basis = SYSTEMS[system] if system in SYSTEMS else (fixtures.BENZENE, "cc-pvdz")
    mol = _mol(atom, basis)
    n = mol.nao
    D, W = _sym(n, 51), _sym(n, 52)
    eng = Engine(mol)
    g = torch.zeros(mol.natm, 3, dtype=torch.float64, device=eng.device)
    eng.grad_1e(_dev(D, eng), _dev(W, eng), g)
    g = g.cpu().numpy()
    ref = orc.Oracle(mol).grad_1e(D, W)
    err = np.abs(g - ref).max()
    print(f"grad_1e {system}: |g - g_ref| = {err:.2e} of max |g_ref| {np.abs(ref).max():.1f}")
    assert err < 1e-10 * max(1.0, np.abs(ref).max()), (system, err)


def test_grad_1e_matches_exact_oracle_every_class():
    """int1e_grad_kernel<LA,LB> at each of its 16 ordered angular classes on the synthetic s..f molecule with a ghost centre:
    for every class one one-centre and one two-centre shell pair (i, j) -- the basis has one shell of each l per centre, so the
    one-centre pair of an l_i = l_j class is the diagonal (i, i), the only place a diagonal pair runs alone -- with D and W zero
    outside the blocks (i, j) and (j, i) (symmetric, fixed seed), then full random symmetric D, W.  Bound of
    test_grad_1e_matches_exact_oracle: |g - g_ref| < 1e-10 max(1, |g_ref|max).

    Observed on the MI355X: 2.5e-16 .. 1.3e-14 over the 32 block cases (|g_ref|max 0.4 .. 14), 4.6e-15 with full D, W."""
    from mi355scf.engine import Engine
    from oracle import oracle as orc
    from test_gpu_pcm_kernels import _synthetic_with_ghost
    mol = _synthetic_with_ghost()
    n, nb = mol.nao, mol._bas.shape[0]
    l, at, loc = mol._bas[:, 1], mol._bas[:, 0], mol.ao_loc_nr()
    eng, oracle = Engine(mol), orc.Oracle(mol)
    rng = np.random.default_rng(53)

    def rel_err(D, W):
        g = torch.zeros(mol.natm, 3, dtype=torch.float64, device=eng.device)
        eng.grad_1e(_dev(D, eng), _dev(W, eng), g)
        ref = oracle.grad_1e(D, W)
        assert np.abs(ref).max() > 1e-3
        return np.abs(g.cpu().numpy() - ref).max() / max(1.0, np.abs(ref).max())

    bad = []
    for la in range(4):
        for lb in range(4):
            one = next((i, j) for i in range(nb) for j in range(nb) if (l[i], l[j]) == (la, lb) and at[i] == at[j] == 1)
            two = next((i, j) for i in range(nb) for j in range(nb) if (l[i], l[j]) == (la, lb) and (at[i], at[j]) == (2, 3))
            assert (one[0] == one[1]) == (la == lb)
            errs = []
            for i, j in (one, two):
                D, W = np.zeros((n, n)), np.zeros((n, n))
                for M in (D, W):
                    blk = rng.standard_normal((loc[i + 1] - loc[i], loc[j + 1] - loc[j]))
                    if i == j:
                        blk = blk + blk.T
                    M[loc[i]:loc[i + 1], loc[j]:loc[j + 1]] = blk
                    M[loc[j]:loc[j + 1], loc[i]:loc[i + 1]] = blk.T
                errs.append(rel_err(D, W))
            print(f"int1e_grad<{la},{lb}>: one-centre {one} {errs[0]:.1e}, two-centre {two} {errs[1]:.1e}")
            if not max(errs) < 1e-10:
                bad.append(((la, lb), errs))
    full = rel_err(_sym(n, 51), _sym(n, 52))
    print(f"int1e_grad, full random D, W: {full:.1e}")
    assert not bad, bad
    assert full < 1e-10


# --- density fitting ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,basis", [("h2o", "6-31g(d)"), ("h2co", "6-31g")])
def test_df_grad_matches_exact_oracle(name, basis):
    """mi_df_grad with Z3 only, Z2 only, both, and split over three ranks; water/6-31G(d)'s auxiliary set reaches g."""
    from mi355scf import df
    from mi355scf.engine import Engine
    from oracle import df as odf
    mol = _mol(MOLECULES[name], basis)
    eng = Engine(mol)
    d = df.DF(mol).build(eng)
    if basis == "6-31g(d)":
        assert d.auxmol._bas[:, 1].max() == 4
    n, na = mol.nao, d.naux
    rng = np.random.default_rng(61)
    z3 = rng.standard_normal((n, n, na))
    z3 = z3 + z3.transpose(1, 0, 2)
    z2 = _sym(na, 62)
    aux_eng = Engine(d._aux_packed, device=eng.device)
    r3, r2 = odf.grad(mol, d.auxmol, z3, None), odf.grad(mol, d.auxmol, None, z2)

    def run(a3, a2, rank=0, nranks=1):
        g = torch.zeros(mol.natm, 3, dtype=torch.float64, device=eng.device)
        eng.df_grad(aux_eng, _dev(a3, eng) if a3 is not None else None, _dev(a2, eng) if a2 is not None else None, g, rank, nranks)
        return g.cpu().numpy()
    worst = 0.0
    for a3, a2, ref in ((z3, None, r3), (None, z2, r2), (z3, z2, r3 + r2)):
        tol = 1e-10 * max(1.0, np.abs(ref).max())
        for g in (run(a3, a2), sum(run(a3, a2, r, 3) for r in range(3))):
            err = np.abs(g - ref).max()
            worst = max(worst, err / max(1.0, np.abs(ref).max()))
            assert err < tol, (a3 is not None, a2 is not None, err, tol)
    aux_eng.close()
    print(f"df_grad {name}/{basis}: worst |g - g_ref| / max(1, |g_ref|) = {worst:.2e}")


# --- AO second derivatives ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ng", [1, 255, 256, 257, 1000])
def test_eval_ao_second_derivatives_match_exact_oracle(ng):
    """mi_eval_ao(deriv=2) (10 components: value, x, y, z, xx, xy, xz, yy, yz, zz) on water/cc-pVTZ at random points, a point
    exactly on each nucleus, and points so far out that every exponential underflows (exact zeros); 256-thread blocks."""
    from mi355scf.engine import Engine
    from oracle import dft as odft
    mol = _mol(MOLECULES["h2o"], "cc-pvtz")
    R = mol.atom_coords()
    special = np.vstack([R, R[0] + [0.0, 0.0, 100.0], R[1] + [-70.0, 80.0, 0.0], R[2] + [0.0, 9.0, 0.0]])
    pts = np.random.default_rng(ng).normal(size=(ng, 3)) * 2.0
    pos = list(dict.fromkeys([0, ng - 1, ng // 2, 255 % ng, 256 % ng, (ng - 2) % ng]))   # block edges, without repeats
    for p, s in zip(pos, special):
        pts[p] = s
    eng = Engine(mol)
    ao = eng.eval_ao(_dev(pts, eng), deriv=2).cpu().numpy()
    ref = odft.eval_ao(mol, pts, 2).transpose(0, 2, 1)
    assert ao.shape == ref.shape == (10, mol.nao, ng)
    worst = 0.0
    for c in range(10):
        scale = max(1.0, np.abs(ref[c]).max())
        err = np.abs(ao[c] - ref[c]).max()
        worst = max(worst, err / scale)
        assert err < 1e-12 * scale, (c, err, scale)
    far = [p for p in range(ng) if np.linalg.norm(pts[p] - R, axis=1).min() > 50]
    assert len(far) == min(2, max(0, len(pos) - 3))
    assert np.all(ao[:, :, far] == 0.0) and np.all(ref[:, :, far] == 0.0)
    print(f"eval_ao deriv=2 ng={ng}: worst |ao - ref| / max(1, |ref|) = {worst:.2e}")
