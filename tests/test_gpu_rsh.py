"""CAM-B3LYP on the MI355X: the long-range ERI store (`omega` option), the short-range B88 kernel (XC_B88_SR), RKS / UKS
energies, TDA / TDDFT roots and the UV-template flow, each against an independent NumPy reference (test_rsh_host.py: the
McMurchie-Davidson ERIs with the erf hook and the ITYH energy density, both validated there without a GPU)."""
import io

import numpy as np
import pytest

from conftest import MOLECULES
from test_rsh_host import CAM_OMEGA, MDEri, b88_sr, b88_sr_channel

pytestmark = pytest.mark.gpu

CAM = (CAM_OMEGA, 0.65, 0.19)   # (omega, alpha, hyb)
OH = "O 0 0 0; H 0 0 0.97"
_CACHE = {}


def _mol(atom, basis, spin=0):
    from pyscf import gto
    return gto.M(atom=atom, basis=basis, spin=spin, verbose=0)


def _engine(mol, omega, **opts):
    from mi355scf import engine
    e = engine.Engine(mol)
    e.set_option("omega", omega)
    for k, v in opts.items():
        e.set_option(k, v)
    e.prepare_eri(1e-13)
    return e


def _md_lr(mol, key):
    if key not in _CACHE:
        _CACHE[key] = MDEri(mol, CAM_OMEGA).full()
    return _CACHE[key]


# ---------------------------------------------------------------------------------------------
# 1. the long-range store
# ---------------------------------------------------------------------------------------------
PATHS = [dict(eri_tpq=1, eri_fused=0), dict(eri_tpq=0, eri_fused=0), dict(eri_tpq=0, eri_fused=1)]


@pytest.mark.parametrize("opts", PATHS, ids=["tpq", "pair", "fused"])
def test_lr_store_whole_tensor_h2o_631gd(opts):
    mol = _mol(MOLECULES["h2o"], "6-31g(d)")
    eng = _engine(mol, CAM_OMEGA, **opts)
    got = eng.eri_dense().cpu().numpy()
    ref = _md_lr(mol, "h2o")
    assert np.abs(got - ref).max() < 1e-10, np.abs(got - ref).max()
    eng.close()


def _sample_quartets(mol, per_class, seed):
    """A seeded sample of shell quartets, `per_class` of every angular class (la >= lb, lc >= ld, (la,lb) >= (lc,ld))."""
    rng = np.random.default_rng(seed)
    ls = [int(mol._bas[s, 1]) for s in range(mol.nbas)]
    classes = {}
    nb = mol.nbas
    for i in range(nb):
        for j in range(nb):
            for k in range(nb):
                for l in range(nb):
                    key = (ls[i], ls[j], ls[k], ls[l])
                    if key[0] >= key[1] and key[2] >= key[3] and key[:2] >= key[2:]:
                        classes.setdefault(key, []).append((i, j, k, l))
    out = []
    for key in sorted(classes):
        q = classes[key]
        for t in rng.choice(len(q), size=min(per_class, len(q)), replace=False):
            out.append(q[t])
    return out, sorted(classes)


@pytest.mark.parametrize("opts", PATHS[1:], ids=["pair", "fused"])
def test_lr_store_sampled_quartets_h2o_ccpvtz(opts):
    """Every angular class up to (ff|ff) on H2O/cc-pVTZ."""
    mol = _mol(MOLECULES["h2o"], "cc-pvtz")
    eng = _engine(mol, CAM_OMEGA, **opts)
    md = MDEri(mol, CAM_OMEGA)
    quartets, classes = _sample_quartets(mol, 3, seed=11)
    assert (3, 3, 3, 3) in classes
    worst = 0.0
    for q in quartets:
        worst = max(worst, np.abs(eng.eri_read_quartet(*q) - md.shell_block(*q)).max())
    assert worst < 1e-10, worst
    eng.close()


def test_lr_store_thread_per_quartet_kernels():
    """Benzene/6-31G(d) has enough low-class quartets (>= 32768 per class pair) for the thread-per-quartet kernels; the forced
    (tpq_maxprim high) and the disabled path both match the reference."""
    from mi355scf import smiles_fixtures
    sym, xyz = smiles_fixtures.lookup("c1ccccc1")
    from pyscf import gto
    mol = gto.M(atom=[(s, tuple(x)) for s, x in zip(sym, xyz)], basis="6-31g(d)", unit="Angstrom", verbose=0)
    md = MDEri(mol, CAM_OMEGA)
    quartets = [q for q in _sample_quartets(mol, 4, seed=5)[0] if sum(int(mol._bas[s, 1]) for s in q) <= 3]
    for opts in (dict(eri_tpq=1, tpq_maxprim=1e9), dict(eri_tpq=0)):
        eng = _engine(mol, CAM_OMEGA, **opts)
        worst = max(np.abs(eng.eri_read_quartet(*q) - md.shell_block(*q)).max() for q in quartets)
        assert worst < 1e-10, (opts, worst)
        eng.close()


def _synthetic_sample(seed):
    """{"near" / "far": shell quartets} of the synthetic s..f molecule (test_gpu_eri_elements.synthetic_mol; shell 4 c + l is the
    l shell of centre c, centre 0 = He, 3 = the ghost): for every angular class one all-one-centre quartet, one quartet of a
    one-centre pair on the far ghost and a one-centre pair on He (far geometry: Rys argument 57 .. 204, beyond the root tables),
    one four-centre quartet, and a seeded random one (three quartets per class on the near geometry, four on the far one)."""
    rng = np.random.default_rng(seed)
    out = {"near": [], "far": []}
    for la in range(4):
        for lb in range(la + 1):
            for lc in range(la + 1):
                for ld in range(lc + 1):
                    if (lc, ld) > (la, lb):
                        continue
                    ls = (la, lb, lc, ld)
                    at = lambda cs: tuple(4 * c + l for c, l in zip(cs, ls))
                    one, fn, four = int(rng.integers(4)), (3, 3, 0, 0), tuple(int(c) for c in rng.permutation(4))
                    rand = [tuple(int(c) for c in rng.integers(0, 4, 4)) for _ in range(2)]
                    out["near"] += [at(c) for c in [(one,) * 4, four] + rand[:1]]
                    out["far"] += [at(c) for c in [(one,) * 4, fn, four] + rand[1:]]
    return out


LR_OMEGA_LARGE = 2.0


def test_lr_store_every_tpq_class_inside_and_beyond_the_root_tables(monkeypatch, capfd):
    """The long-range store with every class of the thread-per-quartet switch on those kernels (`tpq_min_tasks = 1`; the f-shell
    classes included, asserted from the MI355_DEBUG lines), and the same quartets on the wave-per-quartet pair, against
    MDEri.shell_block.  The sample holds, per angular class, an all-one-centre quartet (x = 0), a far/near one-centre x
    one-centre quartet and a four-centre one.

    The attenuated kernels evaluate the roots at theta x, theta = omega^2 / (omega^2 + rho).  With omega = CAM_OMEGA theta is
    about 0.05 .. 0.2 and NO quartet of either geometry leaves the root tables (asserted: the largest theta x stays below every
    table end), so that case covers the Chebyshev branch and x = 0 only.  The asymptotic branch under omega > 0 is reached by the
    far geometry at omega = LR_OMEGA_LARGE (theta 0.7 .. 0.9): rys_branch_coverage asserts all three cases on theta x for every
    root count there, and the same sample is compared again.

    Observed on the MI355X: worst block 2.0e-14 (near) and 1.9e-14 (far) at CAM_OMEGA, the same on both routes."""
    from test_gpu_eri_elements import FORCED_TPQ, _eval_routes, rys_branch_coverage, rys_table_ends, switch_classes, synthetic_mol
    mols = {w: synthetic_mol(w) for w in ("near", "far")}
    rys_branch_coverage(list(mols.values()))                               # the un-attenuated arguments, as the issue states them
    ends = rys_table_ends()
    cam = rys_branch_coverage(list(mols.values()), omega=CAM_OMEGA, require=False)
    assert all(hi < ends[n] for n, (_lo, hi) in cam.items()), cam       # CAM_OMEGA: nothing beyond the tables (see above)
    cover = rys_branch_coverage(list(mols.values()), omega=LR_OMEGA_LARGE)
    assert all(hi > ends[n] for n, (_lo, hi) in cover.items())
    sample = _synthetic_sample(seed=23)
    classes = {tuple(s % 4 for s in q) for q in sample["far"]}
    assert len(classes) == 55 and switch_classes("TPQ_CASE") <= classes
    monkeypatch.setenv("MI355_DEBUG", "2")
    for which, omega in (("near", CAM_OMEGA), ("far", CAM_OMEGA), ("far", LR_OMEGA_LARGE)):
        mol = mols[which]
        md = MDEri(mol, omega)
        ref = {q: md.shell_block(*q) for q in sample[which]}
        if which == "far":
            assert (12, 12, 0, 0) in ref and np.abs(ref[(12, 12, 0, 0)]).max() > 0.05       # nothing screens the far/near quartets
        report = []
        for opts in (FORCED_TPQ, dict(eri_tpq=0)):
            capfd.readouterr()
            eng = _engine(mol, omega, **opts)
            routes = _eval_routes(capfd.readouterr().err)
            on_tpq = {k for k, v in routes.items() if v.startswith("thread-per-quartet fused kernel")}
            assert on_tpq == (switch_classes("TPQ_CASE") if opts is FORCED_TPQ else set()), (which, omega, opts, sorted(on_tpq))
            err = {q: np.abs(eng.eri_read_quartet(*q) - ref[q]).max() for q in sample[which]}
            eng.close()
            worst = max(err, key=err.get)
            report.append(f"{which} omega={omega} {opts}: {len(err)} quartets, worst {worst} {err[worst]:.2e}")
            assert err[worst] < 1e-10, (which, omega, opts, worst, err[worst])
        print("\n".join(report))


def test_huge_omega_is_the_full_store():
    """omega = 1e8: theta = 1 - O(rho / omega^2) for every primitive pair, the store equals the full-Coulomb one."""
    mol = _mol(MOLECULES["h2o"], "cc-pvtz")
    full = _engine(mol, 0.0).eri_dense().cpu().numpy()
    lr = _engine(mol, 1e8).eri_dense().cpu().numpy()
    assert np.abs(full - lr).max() < 1e-10, np.abs(full - lr).max()


def test_grad_eri_refuses_a_long_range_context():
    import torch
    from mi355scf import engine
    mol = _mol(MOLECULES["h2o"], "6-31g(d)")
    eng = _engine(mol, CAM_OMEGA)
    D = torch.eye(mol.nao, dtype=torch.float64, device=eng.device)
    g = torch.zeros(mol.natm, 3, dtype=torch.float64, device=eng.device)
    with pytest.raises(engine.EngineError, match="omega"):
        eng.grad_eri(D, 0.19, g)
    with pytest.raises(engine.EngineError):
        engine.Engine(mol).set_option("omega", -1.0)


# ---------------------------------------------------------------------------------------------
# 2. the short-range B88 kernel
# ---------------------------------------------------------------------------------------------
def _grid_points(n=400, seed=2):
    rng = np.random.default_rng(seed)
    rho = 10.0 ** rng.uniform(-9.7, 2, n)       # both sides of the series switch (a = 1 near rho = 1.5e-4)
    g = rho ** (4.0 / 3) * 10.0 ** rng.uniform(-2, 1.5, n)   # |grad rho| over a wide range of reduced gradients
    u = rng.standard_normal((3, n))
    u /= np.linalg.norm(u, axis=0)
    return rho, g * u


def _ityh_a(rho, sigma, omega=CAM_OMEGA):
    """a = omega / (2 k_s) of one spin channel of a closed-shell point (the argument of the ITYH factor)."""
    r, s = 0.5 * rho, 0.25 * sigma
    x = np.sqrt(s) / r ** (4.0 / 3)
    K = 1.5 * (6 / np.pi) ** (1.0 / 3) + 2 * 0.0042 * x * x / (1 + 6 * 0.0042 * x * np.arcsinh(x))
    return omega / (2 * np.sqrt(9 * np.pi / K) * r ** (1.0 / 3))


def test_b88_sr_kernel_matches_reference():
    import torch
    from mi355scf import engine
    rho, grad = _grid_points()
    sigma = (grad * grad).sum(axis=0)
    dev = torch.device("cuda", 0)
    eng = engine.Engine(_mol(MOLECULES["h2o"], "sto-3g"))
    R = torch.as_tensor(np.vstack([rho, grad]), device=dev)
    w = torch.ones(len(rho), dtype=torch.float64, device=dev)
    e, wv, vr, vs = eng.xc_eval([(1.0, 12)], R, w, 1, want_raw=True, params=[CAM_OMEGA])
    h = 1e-30
    er = b88_sr(rho, sigma)
    vr_ref = np.imag(b88_sr(rho + 1j * h, sigma + 0j)) / h
    vs_ref = np.imag(b88_sr(rho + 0j, sigma + 1j * h)) / h
    # vsigma carries F(a) + a F'(a) / 2, whose leading 1/(36 a^2) terms cancel; the kernel and the host mirror form it from the
    # series without that cancellation from a = 1 on, so 2e-9 holds at every a (tests/test_gpu_xc_edges.py pins both to mpmath)
    a = _ityh_a(rho, sigma)
    assert (a < 1.0).any() and ((a > 2.0) & (a < 4.0)).any() and (a > 4.0).any() and (a > 50.0).any()
    for got, ref, what, tol in ((e, er, "e", 2e-9), (vr, vr_ref, "vrho", 2e-9), (vs, vs_ref, "vsigma", 2e-9)):
        got = got.cpu().numpy()
        assert np.all(np.abs(got - ref) <= tol * np.abs(ref) + 1e-300), (what, np.max(np.abs(got - ref) / np.abs(ref)))
    # the parameter is required
    with pytest.raises(engine.EngineError):
        eng.xc_eval([(1.0, 12)], R, w, 1)


def test_b88_sr_spin_kernel():
    import torch
    from mi355scf import engine
    rho, grad = _grid_points(300, seed=4)
    dev = torch.device("cuda", 0)
    eng = engine.Engine(_mol(MOLECULES["h2o"], "sto-3g"))
    w = torch.full((len(rho),), 0.7, dtype=torch.float64, device=dev)
    terms, prm = [(1.0, 12)], [CAM_OMEGA]
    # rho_a = rho_b: the closed-shell kernel
    half = torch.as_tensor(0.5 * np.vstack([rho, grad]), device=dev)
    e_s, wva, wvb = eng.xc_eval_spin(terms, half, half, w, 1, params=prm)
    e_c, wv = eng.xc_eval(terms, torch.as_tensor(np.vstack([rho, grad]), device=dev), w, 1, params=prm)
    assert torch.allclose(e_s, e_c, rtol=1e-12, atol=0) and torch.allclose(wva, wv, rtol=1e-11, atol=1e-300)
    assert torch.equal(wva, wvb)
    # rho_a != rho_b against the per-channel reference
    rng = np.random.default_rng(9)
    fa = rng.uniform(0.05, 0.95, len(rho))
    ra, rb = fa * rho, (1 - fa) * rho
    ga, gb = grad * fa, grad * (1 - fa) + 0.1 * grad[::-1] * (1 - fa)
    saa, sbb = (ga * ga).sum(axis=0), (gb * gb).sum(axis=0)
    e, wva, wvb = eng.xc_eval_spin(terms, torch.as_tensor(np.vstack([ra, ga]), device=dev),
                                   torch.as_tensor(np.vstack([rb, gb]), device=dev), w, 1, params=prm)
    h = 1e-30
    ref = b88_sr_channel(ra, saa, CAM_OMEGA) + b88_sr_channel(rb, sbb, CAM_OMEGA)
    assert np.all(np.abs(e.cpu().numpy() - ref) <= 1e-9 * np.abs(ref))
    for wvs, r_, s_, g_ in ((wva, ra, saa, ga), (wvb, rb, sbb, gb)):
        vr = np.imag(b88_sr_channel(r_ + 1j * h, s_ + 0j, CAM_OMEGA)) / h
        vss = np.imag(b88_sr_channel(r_ + 0j, s_ + 1j * h, CAM_OMEGA)) / h
        got = wvs.cpu().numpy()
        assert np.all(np.abs(got[0] - 0.35 * vr) <= 1e-9 * np.abs(0.35 * vr))
        ref_g = 0.7 * 2 * vss * g_
        assert np.abs(got[1:] - ref_g).max() <= 1e-9 * np.abs(ref_g).max()


# ---------------------------------------------------------------------------------------------
# 3.-4. SCF energies against references built from the oracle's integrals and functionals
# ---------------------------------------------------------------------------------------------
OTHER_TERMS = [(0.35, "b88"), (0.19, "vwn5"), (0.81, "lyp")]   # the oracle's part of CAM-B3LYP; + 0.46 B88_SR below


def _xc_closed(ao, w, dm, rho_cut=1e-10):
    """(E_xc, V_xc) of CAM-B3LYP's semilocal part for a closed-shell density on the points of `ao`."""
    from oracle import dft as odft

    def edens(r, s):
        return odft.energy_density(OTHER_TERMS, r, s) + 0.46 * b88_sr(r, s)
    c0 = ao[0] @ dm
    rho = np.einsum("gi,gi->g", ao[0], c0)
    grad = np.array([2 * np.einsum("gi,gi->g", ao[1 + k], c0) for k in range(3)])
    sigma = (grad * grad).sum(axis=0)
    ok = rho > rho_cut
    r, s = np.where(ok, rho, 1.0), np.where(ok, sigma, 1.0)
    h = 1e-30
    e = np.where(ok, np.real(edens(r + 0j, s + 0j)), 0.0)
    vr = np.where(ok, np.imag(edens(r + 1j * h, s + 0j)) / h, 0.0)
    vs = np.where(ok, np.imag(edens(r + 0j, s + 1j * h)) / h, 0.0)
    aow = ao[0] * (0.5 * w * vr)[:, None]
    for k in range(3):
        aow += ao[1 + k] * (2 * w * vs * grad[k])[:, None]
    v = ao[0].T @ aow
    return float(w @ e), v + v.T


def _xc_spin(ao, w, dm, rho_cut=1e-10):
    """(E_xc, [V_a, V_b]) of CAM-B3LYP's semilocal part for spin densities dm[2]."""
    from oracle import dft as odft
    rho, grad = [], []
    for s_ in range(2):
        c0 = ao[0] @ dm[s_]
        rho.append(np.maximum(np.einsum("gi,gi->g", ao[0], c0), 0.0))
        grad.append(np.array([2 * np.einsum("gi,gi->g", ao[1 + k], c0) for k in range(3)]))
    ok = rho[0] + rho[1] > rho_cut
    args = [np.where(ok, rho[0], 0.5), np.where(ok, rho[1], 0.5), np.where(ok, (grad[0] ** 2).sum(0), 0.0),
            np.where(ok, (grad[0] * grad[1]).sum(0), 0.0), np.where(ok, (grad[1] ** 2).sum(0), 0.0)]

    def edens(ra, rb, saa, sab, sbb):
        e = odft.energy_density_spin(OTHER_TERMS, ra, rb, saa, sab, sbb)
        for r_, s_ in ((ra, saa), (rb, sbb)):
            live = np.real(r_) > odft.CHANNEL_FLOOR
            e = e + 0.46 * np.where(live, b88_sr_channel(np.where(live, r_, 1.0), np.where(live, s_, 1.0), CAM_OMEGA), 0.0)
        return e
    h = 1e-30
    a = [np.asarray(x, dtype=complex) for x in args]
    e = np.where(ok, np.real(edens(*a)), 0.0)
    d = []
    for i in range(5):
        b = [x.copy() for x in a]
        b[i] = b[i] + 1j * h
        d.append(np.where(ok, np.imag(edens(*b)) / h, 0.0))
    V = []
    for vr, vss, g_own, g_oth in ((d[0], d[2], grad[0], grad[1]), (d[1], d[4], grad[1], grad[0])):
        aow = ao[0] * (0.5 * w * vr)[:, None]
        for k in range(3):
            aow += ao[1 + k] * (w * (2 * vss * g_own[k] + d[3] * g_oth[k]))[:, None]
        m = ao[0].T @ aow
        V.append(m + m.T)
    return float(w @ e), np.array(V)


def _rks(name, basis="6-31g(d)"):
    key = ("rks", name, basis)
    if key not in _CACHE:
        import gpu4pyscf
        mol = _mol(MOLECULES[name], basis)
        mf = gpu4pyscf.dft.RKS(mol).to_gpu()
        mf.xc = "CAM-B3LYP"
        mf.conv_tol = 1e-11
        mf.kernel()
        _CACHE[key] = (mol, mf)
    return _CACHE[key]


@pytest.mark.parametrize("name", ["h2o", "h2co"])
def test_rks_cam_b3lyp_energy_matches_reference_scf(name):
    from oracle import dft as odft, oracle as orc
    mol, mf = _rks(name)
    assert mf.converged
    ao = odft.eval_ao(mol, mf.grids.coords.cpu().numpy(), 1)
    w = mf.grids.weights.cpu().numpy()
    o = orc.Oracle(mol)
    eri_lr = _md_lr(mol, name)
    _omega, alpha, hyb = CAM

    def veff(dm):
        J, K = o.jk(dm)
        Klr = np.einsum("ijkl,jl->ik", eri_lr, dm)
        Keff = hyb * K + (alpha - hyb) * Klr
        exc, vxc = _xc_closed(ao, w, dm)
        return J - 0.5 * Keff + vxc, 0.5 * float(np.sum(dm * J)) - 0.25 * float(np.sum(dm * Keff)) + exc

    ref = orc.rhf(mol, dm0=np.asarray(mf.make_rdm1()), conv_tol=1e-11, veff_fn=veff, oracle=o)
    assert abs(mf.e_tot - ref["e_tot"]) < 1e-8, (mf.e_tot, ref["e_tot"])
    # the functional is really range-separated: B3LYP-like global hybrid at 19 % differs by far more
    assert abs(mf.e_tot - ref["e_tot"]) < 1e-3 * abs(mf.e_tot)


def test_uks_closed_shell_equals_rks():
    import gpu4pyscf
    mol, mf = _rks("h2o")
    mu = gpu4pyscf.dft.UKS(mol).to_gpu()
    mu.xc = "CAM-B3LYP"
    mu.conv_tol = 1e-11
    mu.kernel()
    assert mu.converged and abs(mu.e_tot - mf.e_tot) < 1e-9, (mu.e_tot, mf.e_tot)


def test_uks_open_shell_oh_matches_reference():
    """OH radical: the reference functional (oracle J/K/XC, NumPy K_LR and B88_SR) evaluated at the engine's converged spin
    densities gives the engine's energy, and its Fock matrices commute with them (the same stationary point)."""
    import gpu4pyscf
    from oracle import dft as odft, oracle as orc
    mol = _mol(OH, "6-31g(d)", spin=1)
    mf = gpu4pyscf.dft.UKS(mol).to_gpu()
    mf.xc = "CAM-B3LYP"
    mf.conv_tol = 1e-11
    mf.kernel()
    assert mf.converged
    dm = np.asarray(mf.make_rdm1())
    ao = odft.eval_ao(mol, mf.grids.coords.cpu().numpy(), 1)
    w = mf.grids.weights.cpu().numpy()
    o = orc.Oracle(mol)
    S, T, V, _ = o.int1e()
    h = T + V
    eri_lr = MDEri(mol, CAM_OMEGA).full()
    _omega, alpha, hyb = CAM
    J = sum(o.jk(dm[s_])[0] for s_ in range(2))
    Keff = [hyb * o.jk(dm[s_])[1] + (alpha - hyb) * np.einsum("ijkl,jl->ik", eri_lr, dm[s_]) for s_ in range(2)]
    exc, vxc = _xc_spin(ao, w, dm)
    D = dm[0] + dm[1]
    e = float(np.sum(D * h)) + 0.5 * float(np.sum(D * J)) - 0.5 * sum(float(np.sum(dm[s_] * Keff[s_])) for s_ in range(2)) + exc
    e += mol.energy_nuc()
    assert abs(mf.e_tot - e) < 1e-8, (mf.e_tot, e)
    for s_ in range(2):
        F = h + J - Keff[s_] + vxc[s_]
        comm = F @ dm[s_] @ S - S @ dm[s_] @ F
        assert np.abs(comm).max() < 1e-5, np.abs(comm).max()


# ---------------------------------------------------------------------------------------------
# 5. TDA / TDDFT against dense A, B
# ---------------------------------------------------------------------------------------------
def test_tda_tddft_cam_b3lyp_match_dense_reference():
    from pyscf import tdscf
    from oracle import dft as odft, oracle as orc
    mol, mf = _rks("h2o")
    ao = odft.eval_ao(mol, mf.grids.coords.cpu().numpy(), 1)
    w = mf.grids.weights.cpu().numpy()
    eri = orc.Oracle(mol).eri_full()
    eri_lr = _md_lr(mol, "h2o")
    _omega, alpha, hyb = CAM
    C, eps = np.asarray(mf.mo_coeff), np.asarray(mf.mo_energy)
    no = int((np.asarray(mf.mo_occ) > 0).sum())
    Co, Cv = C[:, :no], C[:, no:]
    nv = Cv.shape[1]
    n = no * nv

    def blocks(g):
        ovov = np.einsum("pqrs,pi,qa,rj,sb->iajb", g, Co, Cv, Co, Cv, optimize=True).reshape(n, n)
        oovv = np.einsum("pqrs,pi,qj,ra,sb->ijab", g, Co, Co, Cv, Cv, optimize=True).transpose(0, 2, 1, 3).reshape(n, n)
        ovvo = np.einsum("pqrs,pi,qa,rj,sb->iajb", g, Co, Cv, Co, Cv, optimize=True).transpose(0, 3, 2, 1).reshape(n, n)
        return ovov, oovv, ovvo
    ovov, oovv, ovvo = blocks(eri)
    _, oovv_lr, ovvo_lr = blocks(eri_lr)
    D0 = np.asarray(mf.make_rdm1())

    def dvxc(M, step=1e-4):
        s = step / np.abs(M).max()
        return (_xc_closed(ao, w, D0 + s * M)[1] - _xc_closed(ao, w, D0 - s * M)[1]) / (2 * s)
    fxc = np.zeros((n, n))
    for j in range(no):
        for b in range(nv):
            Dt = np.outer(Co[:, j], Cv[:, b]) + np.outer(Cv[:, b], Co[:, j])
            fxc[:, j * nv + b] = (Co.T @ dvxc(Dt) @ Cv).reshape(-1)
    de = (eps[no:][None, :] - eps[:no, None]).reshape(-1)
    A = np.diag(de) + 2 * ovov - hyb * oovv - (alpha - hyb) * oovv_lr + fxc
    B = 2 * ovov - hyb * ovvo - (alpha - hyb) * ovvo_lr + fxc
    A, B = 0.5 * (A + A.T), 0.5 * (B + B.T)
    ns = 5
    td = tdscf.TDA(mf)
    td.nstates, td.conv_tol = ns, 1e-11
    e, _ = td.kernel()
    assert td.converged.all()
    assert np.abs(e - np.linalg.eigvalsh(A)[:ns]).max() < 1e-6, (e, np.linalg.eigvalsh(A)[:ns])
    rp = tdscf.TDDFT(mf)
    rp.nstates, rp.conv_tol = ns, 1e-11
    e2, xy = rp.kernel()
    ref = np.sort(np.sqrt(np.linalg.eigvals((A - B) @ (A + B)).real))[:ns]
    assert rp.converged.all()
    assert np.abs(e2 - ref).max() < 1e-6, (e2, ref)
    for x, y in xy:
        assert abs((x * x).sum() - (y * y).sum() - 0.5) < 1e-9


# ---------------------------------------------------------------------------------------------
# 6. the UV template's flow with --method CAM-B3LYP
# ---------------------------------------------------------------------------------------------
def test_benzoquinone_uv_flow_cam_b3lyp():
    import gpu4pyscf
    from pyscf import gto, tdscf
    from mi355scf import smiles_fixtures
    sym, xyz = smiles_fixtures.lookup("O=C1C=CC(=O)C=C1")
    mol = gto.M(atom=[(s, tuple(x)) for s, x in zip(sym, xyz)], basis="6-31G*", unit="Angstrom", verbose=0)
    mf = gpu4pyscf.dft.RKS(mol).to_gpu()
    mf.xc = "CAM-B3LYP"
    mf.kernel()
    assert mf.converged
    td = tdscf.TDDFT(mf)
    td.nstates = 10
    e, xy = td.kernel()
    td.stdout = io.StringIO()
    td.verbose = 4
    td.analyze()
    log = td.stdout.getvalue()
    assert log.count("Excited State") == 10 and " eV " in log and " nm " in log and "f=" in log
    f = np.asarray(td.oscillator_strength())
    e = np.asarray(e)
    assert len(e) == 10 and td.converged.all()
    assert np.all(e > 0) and np.all(np.diff(e) >= 0) and np.all(f >= 0)


# ---------------------------------------------------------------------------------------------
# 7. refusals
# ---------------------------------------------------------------------------------------------
def test_paths_without_long_range_exchange_refuse():
    import gpu4pyscf
    from pyscf import solvent
    from pyscf.geomopt.geometric_solver import optimize
    mol, mf = _rks("h2o")
    with pytest.raises(NotImplementedError):
        mf.nuc_grad_method()
    with pytest.raises(NotImplementedError):
        optimize(mf)
    with pytest.raises(NotImplementedError):
        solvent.PCM(mf)
    m2 = gpu4pyscf.dft.RKS(mol).to_gpu()
    m2.xc = "CAM-B3LYP"
    with pytest.raises(NotImplementedError):
        m2.density_fit()
    m3 = gpu4pyscf.dft.RKS(mol).to_gpu()
    m3.xc = "CAM-B3LYP"
    m3.omega = 0.4
    with pytest.raises(NotImplementedError):
        m3.kernel()
