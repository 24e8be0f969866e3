"""The point-charge embedding kernels (`pc_*` in csrc/mi355scf.hip) against exact FP64 references at every angular class, on the
synthetic three-atom s..f molecule of test_gpu_pcm_kernels.py (48 AOs, every class on one centre and across two).

References, both exact FP64 and independent of the kernels' Rys quadrature (the oracle is McMurchie-Davidson):
  * Gaussian charges: (mn|kk) and d/dA (mn|kk) with one s shell of exponent zeta^2 / 2 per point (`_with_points`);
  * point charges: `Oracle.int1e()` V and `Oracle.int1e_ip()` dV of a copy of the molecule whose own nuclear charges are zero and
    which carries one unit-charged centre per point.
Each test prints its figures (pytest -rP shows them)."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from test_gpu_dense_kernels import U, assert_guard, guarded
from test_gpu_pcm import _oracle_B
from test_gpu_pcm_kernels import NPTS, _derivative_blocks, _dev, _engine, _pair_classes, _points, _synthetic

pytestmark = pytest.mark.gpu

TOL = 1e-11
_CACHE = {}
ON_BE, FAR, ZETA_LO, ZETA_HI, Q_ZERO = 1, 64, 30, 66, 5


def _sites():
    """The 70 points of the PCM kernel tests with every even one turned into a point charge (zeta = 0) except the two ends of
    the zeta range: a Gaussian charge exactly on Be, a point charge 56 Bohr away, zeta = 0.05 and 60, charges of mixed sign
    and one q = 0."""
    if "sites" not in _CACHE:
        pts = _points()[0].copy()
        point = (np.arange(NPTS) % 2 == 0)
        point[[ZETA_LO, ZETA_HI]] = False
        pts[point, 3] = 0.0
        assert not point[ON_BE] and point[FAR] and pts[ZETA_LO, 3] == 0.05 and pts[ZETA_HI, 3] == 60.0
        d = np.linalg.norm(pts[point, None, :3] - _synthetic().atom_coords()[None], axis=2)
        assert d.min() > 0.05 and d.max() > 50.0
        q = np.random.default_rng(5).uniform(0.3, 1.2, NPTS) * np.where(np.arange(NPTS) % 3 == 0, -1.0, 1.0)
        q[Q_ZERO] = 0.0
        _CACHE["sites"] = (pts, q, point)
    return _CACHE["sites"]


def _with_unit_centres(mol, coords):
    """`mol` with its own nuclear charges zeroed plus one centre of charge +1 per point (no basis functions on them)."""
    atm = mol._atm.copy()
    atm[:, 0] = 0
    env = list(mol._env)
    rows = []
    for c in coords:
        pc = len(env)
        env.extend(list(c) + [0.0])
        rows.append([1, pc, 1, 0, 0, 0])
    atm = np.concatenate([atm, np.asarray(rows, dtype=np.int32).reshape(-1, 6)])
    return SimpleNamespace(_atm=atm, _bas=mol._bas.copy(), _env=np.asarray(env), nao=mol.nao)


def _point_charge_V(mol, coords):
    """[n, nao, nao] of (m| 1/|r - r_k| |n): minus the oracle's nuclear attraction of one unit centre at a time."""
    from oracle import oracle as orc
    return np.stack([-orc.Oracle(_with_unit_centres(mol, c[None]))
                     .int1e()[2] for c in coords])


def _per_point_V():
    """G[k] = (m| g_k |n) for the 70 sites, from the oracle."""
    if "G" not in _CACHE:
        mol = _synthetic()
        pts, _q, point = _sites()
        G = np.zeros((NPTS, mol.nao, mol.nao))
        gi = np.flatnonzero(~point)
        G[gi] = _oracle_B(mol, pts[gi, :3], pts[gi, 3])
        G[point] = _point_charge_V(mol, pts[point, :3])
        assert np.isfinite(G).all()
        _CACHE["G"] = G
    return _CACHE["G"]


def _per_point_dV(eng):
    """dG[k, x, m, n] = d/dA_x (m| g_k |n), A the centre of m's shell, for the 70 sites, from the oracle."""
    if "dG" not in _CACHE:
        from oracle import oracle as orc
        mol = _synthetic()
        pts, _q, point = _sites()
        pairs = eng.pcm_pairs(ordered=True)
        dI = _derivative_blocks(pairs)                    # Gaussian kind, all 70 points with the PCM tests' widths
        loc = mol.ao_loc_nr()
        dG = np.zeros((NPTS, 3, mol.nao, mol.nao))
        for p, (i, j) in enumerate(pairs):
            dG[:, :, loc[i]:loc[i + 1], loc[j]:loc[j + 1]] = dI[p]
        pi = np.flatnonzero(point)
        dV = orc.Oracle(_with_unit_centres(mol, pts[pi, :3])).int1e_ip()[2]
        dG[pi] = -dV[mol._atm.shape[0]:]
        assert np.isfinite(dG).all()
        _CACHE["dG"] = dG
    return _CACHE["dG"]


def _ld(nao):
    n = nao * (nao + 1) // 2
    return n + (n & 1)


# ---- 1. pc_fock_kernel<LA,LB> -----------------------------------------------------------------------------------------------
def test_pc_fock_matches_oracle_every_class_and_extreme_points():
    """V = sum_k q_k (m|g_k|n) over the 70 mixed sites against the oracle, |V - ref| < 1e-11 per element, reported per class
    (10 classes, each on one centre and across two); guard doubles behind V and the work buffer stay untouched, a second call
    gives the same bits, V is exactly symmetric.  Observed on the MI355X: 1.1e-15 .. 8.0e-15 per class at |ref|max 6.2."""
    mol, eng = _engine("synthetic", _synthetic)
    pts, q, _point = _sites()
    nao, ld = mol.nao, _ld(mol.nao)
    ref = np.einsum("k,kmn->mn", q, _per_point_V())
    pairs = eng.pcm_pairs(ordered=False)
    cls = _pair_classes(mol, pairs)
    assert sorted(cls) == [(a, b) for a in range(4) for b in range(a + 1)]
    nwork = eng.pc_fock_chunks(NPTS, ld) * ld
    fw, fV = guarded(nwork), guarded(nao * nao)
    V = fV[:nao * nao].view(nao, nao)
    dp, dq = _dev(pts, eng), _dev(q, eng)
    eng.pc_fock(dp, dq, V, work=fw[:nwork])
    torch.cuda.synchronize()
    assert_guard(fw, nwork, "pc_fock work")
    assert_guard(fV, nao * nao, "pc_fock V")
    assert torch.equal(V, V.T)
    again = torch.empty_like(V)
    eng.pc_fock(dp, dq, again)
    assert torch.equal(V, again), "pc_fock: two calls differ (fixed-order sums promised)"
    got = V.cpu().numpy()
    loc = mol.ao_loc_nr()
    bad, lines = [], []
    for c in sorted(cls):
        err = max(np.abs(got[loc[i]:loc[i + 1], loc[j]:loc[j + 1]] - ref[loc[i]:loc[i + 1], loc[j]:loc[j + 1]]).max()
                  for i, j in pairs[cls[c]])
        lines.append(f"pc_fock<{c[0]},{c[1]}>: |err|max = {err:.2e}")
        if not err < TOL:
            bad.append(lines[-1])
    print("\n".join(lines) + f"\n|ref|max = {np.abs(ref).max():.3e}")
    assert not bad, "classes over 1e-11:\n" + "\n".join(bad)


@pytest.mark.parametrize("k", [ON_BE, FAR, ZETA_LO, ZETA_HI, Q_ZERO, 0])
def test_pc_fock_single_sites(k):
    """One site at a time (npts = 1: one lane of one chunk): the Gaussian charge on Be, the point charge 56 Bohr away, the two
    ends of the zeta range, q = 0 (V exactly zero) and an ordinary point charge, each to 1e-11 per element."""
    mol, eng = _engine("synthetic", _synthetic)
    pts, q, _point = _sites()
    V = torch.empty(mol.nao, mol.nao, dtype=torch.float64, device=eng.device)
    eng.pc_fock(_dev(pts[k:k + 1], eng), _dev(q[k:k + 1], eng), V)
    err = np.abs(V.cpu().numpy() - q[k] * _per_point_V()[k]).max()
    print(f"pc_fock site {k} (zeta = {pts[k, 3]}, q = {q[k]:.3f}): |err|max = {err:.2e}")
    assert err < TOL
    if k == Q_ZERO:
        assert torch.count_nonzero(V) == 0


def _pool(n):
    """n sites around the synthetic molecule (alternating kinds) with their per-point matrices from the oracle, computed once for
    the largest count and shared: the first n of the pool."""
    if "pool" not in _CACHE:
        mol = _synthetic()
        nmax = max(_counts())
        rng = np.random.default_rng(77)
        pts = np.zeros((nmax, 4))
        pts[:, :3] = 3.0 * rng.standard_normal((nmax, 3))
        gauss = np.arange(nmax) % 2 == 1
        pts[gauss, 3] = np.exp(rng.uniform(np.log(0.3), np.log(5.0), int(gauss.sum())))
        d = np.linalg.norm(pts[~gauss, None, :3] - mol.atom_coords()[None], axis=2)
        assert d.min() > 0.02
        q = rng.standard_normal(nmax)
        G = np.zeros((nmax, mol.nao, mol.nao))
        G[gauss] = _oracle_B(mol, pts[gauss, :3], pts[gauss, 3])
        G[~gauss] = _point_charge_V(mol, pts[~gauss, :3])
        _CACHE["pool"] = (pts, q, G)
    pts, q, G = _CACHE["pool"]
    return pts[:n], q[:n], G[:n]


def _counts():
    from mi355scf.engine import Engine
    ld = _ld(48)
    edge = next(n for n in range(2, 4096) if Engine.pc_fock_chunks(n, ld) == 2) - 1      # the largest one-chunk count
    assert Engine.pc_fock_chunks(edge, ld) == 1 and edge % 64 == 0
    return (1, 63, 64, 65, edge - 1, edge, edge + 1)


@pytest.mark.parametrize("idx", range(7))
def test_pc_fock_chunk_edges_within_rounding_bound(idx):
    """Point counts at every branch of the chunk loops -- 1, 63, 64, 65 (a partial wave, a full one, one lane's second trip) and
    one chunk minus 1, exact, plus 1 (the second chunk holds a single point) -- against the long-double sum of the per-point
    oracle matrices.  Bound per element: 2 n u sum_k |q_k G_k| (the forward error of a length-n FP64 sum, doubled for the
    lane / butterfly / chunk split, as test_pcm_fock_within_rounding_bound) plus the integrals' own error, for which the
    per-element bound of the 70-site test is taken per site and unit charge: (1e-11 / 70) sum_k |q_k|.  V = and V += 0.5 x.
    Observed on the MI355X: worst |err| / bound 8e-3 (one site), 3e-4 .. 6e-4 otherwise; |err|max / |ref|max at most 2.2e-15,
    with accumulate=True 7e-16 (the issue's 1e-13)."""
    mol, eng = _engine("synthetic", _synthetic)
    n = _counts()[idx]
    pts, q, G = _pool(n)
    nao, ld = mol.nao, _ld(mol.nao)
    Gl = G.astype(np.longdouble)
    s = np.einsum("k,kmn->mn", q.astype(np.longdouble), Gl)
    mag = np.einsum("k,kmn->mn", np.abs(q).astype(np.longdouble), np.abs(Gl))
    V0 = np.random.default_rng(n).standard_normal((nao, nao))
    V0 = V0 + V0.T
    nwork = eng.pc_fock_chunks(n, ld) * ld
    dp, dq = _dev(pts, eng), _dev(q, eng)
    for scale, acc in ((1.0, False), (0.5, True)):
        fw, fV = guarded(nwork), guarded(nao * nao, V0 if acc else None)
        V = fV[:nao * nao].view(nao, nao)
        eng.pc_fock(dp, dq, V, scale=scale, accumulate=acc, work=fw[:nwork])
        torch.cuda.synchronize()
        assert_guard(fw, nwork, "pc_fock work")
        assert_guard(fV, nao * nao, "pc_fock V")
        fV2 = guarded(nao * nao, V0 if acc else None)
        eng.pc_fock(dp, dq, fV2[:nao * nao].view(nao, nao), scale=scale, accumulate=acc)
        assert torch.equal(fV[:nao * nao], fV2[:nao * nao])
        got = V.cpu().numpy().astype(np.longdouble)
        ref = scale * s + (V0 if acc else 0.0)
        bound = 2.0 * (n + int(acc)) * U * (abs(scale) * mag + (np.abs(V0) if acc else 0.0)) + abs(scale) * TOL / 70 * np.abs(q).sum()
        ratio = float(np.max(np.abs(got - ref) / bound))
        rel = float(np.abs(got - ref).max() / np.abs(ref).max())
        print(f"[rounding] pc_fock n = {n} chunks = {eng.pc_fock_chunks(n, ld)} scale = {scale} acc = {acc}: worst |err| / bound = "
              f"{ratio:.3g}, |err|max / |ref|max = {rel:.2e}")
        assert ratio <= 1.0, (n, scale, acc, ratio)
        if acc:
            assert rel < 1e-13, "accumulate=True with scale=0.5: 1e-13 relative"


def test_pc_fock_no_points_leaves_V_untouched():
    mol, eng = _engine("synthetic", _synthetic)
    V0 = np.random.default_rng(1).standard_normal((mol.nao, mol.nao))
    empty = torch.zeros(0, 4, dtype=torch.float64, device=eng.device)
    for acc in (False, True):
        V = _dev(V0, eng)
        eng.pc_fock(empty, empty[:, 0].contiguous(), V, scale=2.0, accumulate=acc)
        assert np.array_equal(V.cpu().numpy(), V0)
    ga, gp = eng.pc_grad(empty, empty[:, 0].contiguous(), _dev(V0 + V0.T, eng))
    assert torch.count_nonzero(ga) == 0 and gp.shape == (0, 3)


def test_pc_entry_points_refuse_bad_input():
    from mi355scf.engine import EngineError
    mol, eng = _engine("synthetic", _synthetic)
    pts, q, _point = _sites()
    V = torch.zeros(mol.nao, mol.nao, dtype=torch.float64, device=eng.device)
    for what, (p, c) in {"nan coordinate": (np.where(np.arange(4) == 1, np.nan, pts[:3]), q[:3]),
                         "inf charge": (pts[:3], np.array([1.0, np.inf, 0.5]))}.items():
        with pytest.raises(EngineError, match="not finite"):
            eng.pc_fock(_dev(p, eng), _dev(c, eng), V)
        with pytest.raises(EngineError, match="not finite"):
            eng.pc_grad(_dev(p, eng), _dev(c, eng), V)


# ---- 2. pc_grad_kernel<LA,LB> -----------------------------------------------------------------------------------------------
def _class_density(mol, D, c):
    """D with every shell block outside the ordered class c = (l_i, l_j) zeroed: only the pairs of that class contribute."""
    l = np.repeat(mol._bas[:, 1], 2 * mol._bas[:, 1] + 1)
    return np.where((l[:, None] == c[0]) & (l[None, :] == c[1]), D, 0.0)


def test_pc_grad_matches_exact_derivative_integrals_every_class():
    """For each of the 16 ordered classes the density restricted to the class' shell blocks, so that exactly its pairs -- on
    one centre and across two -- make up both outputs: g_atoms[A] = 2 sum_k q_k sum_{m on A, n} D_mn d/dA (m|g_k|n) and
    g_pts[k] = -2 q_k sum_mn D_mn d/dA (m|g_k|n) against the oracle, bound 1e-11 max(1, |ref|max); sum_atoms + sum_points = 0
    per component to 1e-10 of the largest term; guards behind both outputs and the work buffer; two calls give the same bits.
    Observed on the MI355X: worst class <3,2> with 5.7e-14 (atoms) and 4.6e-14 (sites) at |ref|max 78; all classes together
    1.0e-13 and 6.2e-14 at 73; sum rule at most 5.7e-14 of 78."""
    mol, eng = _engine("synthetic", _synthetic)
    pts, q, _point = _sites()
    dG = _per_point_dV(eng)
    aoatm = np.repeat(mol._bas[:, 0], 2 * mol._bas[:, 1] + 1)
    A = np.random.default_rng(23).standard_normal((mol.nao, mol.nao))
    D = A + A.T
    dp, dq = _dev(pts, eng), _dev(q, eng)
    nwork, natm = eng.pc_grad_work(NPTS), mol.natm
    bad, lines = [], []
    for c in [(a, b) for a in range(4) for b in range(4)] + ["all"]:
        Dc = D if c == "all" else _class_density(mol, D, c)
        per_ao = 2.0 * np.einsum("k,kxmn,mn->mx", q, dG, Dc)
        ref_a = np.zeros((natm, 3))
        np.add.at(ref_a, aoatm, per_ao)
        ref_p = -2.0 * q[:, None] * np.einsum("kxmn,mn->kx", dG, Dc)
        fw, fa, fp = guarded(nwork), guarded(3 * natm), guarded(3 * NPTS)
        out = (fa[:3 * natm].view(natm, 3), fp[:3 * NPTS].view(NPTS, 3))
        eng.pc_grad(dp, dq, _dev(Dc, eng), work=fw[:nwork], out=out)
        torch.cuda.synchronize()
        for f, n, what in ((fw, nwork, "work"), (fa, 3 * natm, "g_atoms"), (fp, 3 * NPTS, "g_pts")):
            assert_guard(f, n, f"pc_grad {what}")
        ga2, gp2 = eng.pc_grad(dp, dq, _dev(Dc, eng))
        assert torch.equal(ga2, out[0]) and torch.equal(gp2, out[1]), "pc_grad: two calls differ"
        ga, gp = out[0].cpu().numpy(), out[1].cpu().numpy()
        scale = max(1.0, np.abs(ref_a).max(), np.abs(ref_p).max())
        ea, ep = np.abs(ga - ref_a).max(), np.abs(gp - ref_p).max()
        big = max(np.abs(ga).max(), np.abs(gp).max())
        inv = np.abs(ga.sum(axis=0) + gp.sum(axis=0)).max()
        name = "all classes" if c == "all" else f"<{c[0]},{c[1]}>"
        lines.append(f"pc_grad {name}: atoms |err| = {ea:.2e}, sites |err| = {ep:.2e}, |ref|max = {scale:.2e}, "
                     f"sum rule {inv:.1e} of {big:.2e}")
        if not (ea <= TOL * scale and ep <= TOL * scale and inv <= 1e-10 * big):
            bad.append(lines[-1])
    print("\n".join(lines))
    assert not bad, "over the bound:\n" + "\n".join(bad)


NPOOL = 514


def _grad_pool(eng):
    """514 sites (every fourth one Gaussian) with d/dA (m|g_k|n) of the oracle, computed once and shared by the block-edge counts."""
    if "gpool" not in _CACHE:
        from oracle import oracle as orc
        from test_gpu_pcm import _with_points
        mol = _synthetic()
        rng = np.random.default_rng(91)
        pts = np.zeros((NPOOL, 4))
        pts[:, :3] = 3.0 * rng.standard_normal((NPOOL, 3))
        gauss = np.arange(NPOOL) % 4 == 1
        pts[gauss, 3] = np.exp(rng.uniform(np.log(0.3), np.log(5.0), int(gauss.sum())))
        assert np.linalg.norm(pts[~gauss, None, :3] - mol.atom_coords()[None], axis=2).min() > 0.02
        q = rng.standard_normal(NPOOL)
        loc, nb = mol.ao_loc_nr(), mol._bas.shape[0]
        dG = np.zeros((NPOOL, 3, mol.nao, mol.nao))
        gi, pi = np.flatnonzero(gauss), np.flatnonzero(~gauss)
        o = orc.Oracle(_with_points(mol, pts[gi, :3], pts[gi, 3]))
        for i, j in eng.pcm_pairs(ordered=True):
            for t, g in enumerate(gi):
                dG[g, :, loc[i]:loc[i + 1], loc[j]:loc[j + 1]] = o.eri_ip1_shell(i, j, nb + t, nb + t)[:, :, :, 0, 0]
        dG[pi] = -orc.Oracle(_with_unit_centres(mol, pts[pi, :3])).int1e_ip()[2][mol._atm.shape[0]:]
        A = rng.standard_normal((mol.nao, mol.nao))
        D = A + A.T
        per_site = np.einsum("kxmn,mn->kxm", dG, D)          # [k, x, m]: summed over n
        _CACHE["gpool"] = (pts, q, D, per_site)
    return _CACHE["gpool"]


@pytest.mark.parametrize("n", [1, 63, 64, 65, 511, 512, 513])
def test_pc_grad_point_block_edges(n):
    """Site counts around the one-wave block these counts run with (1, 63, 64, 65: a partial block, a full one, a second block of
    one site) and eight blocks minus one, exact and plus one (511, 512, 513) against the oracle, both outputs to
    1e-11 max(1, |ref|max), the sum rule to 1e-10 of the largest term, guards behind the outputs and the work buffer.
    Observed on the MI355X: atoms 6e-15 .. 3.4e-13, sites 5e-15 .. 1.9e-13 at |ref|max 3.6 .. 220; sum rule below 1e-13."""
    mol, eng = _engine("synthetic", _synthetic)
    pts, q, D, per_site = _grad_pool(eng)
    aoatm = np.repeat(mol._bas[:, 0], 2 * mol._bas[:, 1] + 1)
    natm, nwork = mol.natm, eng.pc_grad_work(n)
    ref_a = np.zeros((natm, 3))
    np.add.at(ref_a, aoatm, 2.0 * np.einsum("k,kxm->mx", q[:n], per_site[:n]))
    ref_p = -2.0 * q[:n, None] * per_site[:n].sum(axis=2)
    fw, fa, fp = guarded(nwork), guarded(3 * natm), guarded(3 * n)
    ga, gp = eng.pc_grad(_dev(pts[:n], eng), _dev(q[:n], eng), _dev(D, eng), work=fw[:nwork],
                         out=(fa[:3 * natm].view(natm, 3), fp[:3 * n].view(n, 3)))
    torch.cuda.synchronize()
    for f, m, what in ((fw, nwork, "work"), (fa, 3 * natm, "g_atoms"), (fp, 3 * n, "g_pts")):
        assert_guard(f, m, f"pc_grad {what}")
    ga, gp = ga.cpu().numpy(), gp.cpu().numpy()
    scale = max(1.0, np.abs(ref_a).max(), np.abs(ref_p).max())
    ea, ep = np.abs(ga - ref_a).max(), np.abs(gp - ref_p).max()
    big = max(np.abs(ga).max(), np.abs(gp).max())
    inv = np.abs(ga.sum(axis=0) + gp.sum(axis=0)).max()
    print(f"pc_grad n = {n}: atoms |err| = {ea:.2e}, sites |err| = {ep:.2e}, |ref|max = {scale:.2e}, sum rule {inv:.1e} of {big:.2e}")
    assert ea <= TOL * scale and ep <= TOL * scale and inv <= 1e-10 * big


@pytest.mark.parametrize("n", [4097, 78 * 512 + 1])
def test_pc_grad_many_sites_wider_blocks_and_several_pairs_per_workgroup(n):
    """The planner's other branches, which no count with an oracle reference reaches: 4 097 sites are the first with blocks of
    128 sites (33 blocks, the last of one site; up to 4 096 a block is one wave), 39 937 sites have blocks of 512 (79, the last of
    one site) and, the site partials being held to 128 MB, two of a class' nine pairs per workgroup.  Reference: the same sites in
    runs of at most 512 (one-wave blocks, one pair per workgroup), which the tests above pin to 1e-11 max(1, |ref|max) of the exact
    integrals; the two results, each within that bound of the exact value, may differ by twice it (sites) and by the slices' bounds
    added up (atoms).  Guard behind the work buffer; two calls give the same bits."""
    mol, eng = _engine("synthetic", _synthetic)
    npair = len(eng.pcm_pairs(ordered=True))
    assert npair == 144 and eng.pc_grad_work(512) == 3 * (npair * 8 + npair * 512)
    assert eng.pc_grad_work(n) == (3 * (npair * 33 + npair * n) if n == 4097 else 3 * (npair * 79 + 80 * n))
    rng = np.random.default_rng(17)
    pts = np.zeros((n, 4))
    pts[:, :3] = 4.0 * rng.standard_normal((n, 3))
    pts[1::2, 3] = np.exp(rng.uniform(np.log(0.3), np.log(5.0), n // 2))
    assert np.linalg.norm(pts[::2, None, :3] - mol.atom_coords()[None], axis=2).min() > 1e-3
    q = rng.standard_normal(n)
    A = rng.standard_normal((mol.nao, mol.nao))
    D, dp, dq = _dev(A + A.T, eng), _dev(pts, eng), _dev(q, eng)
    nwork = eng.pc_grad_work(n)
    fw = guarded(nwork)
    ga, gp = eng.pc_grad(dp, dq, D, work=fw[:nwork])
    torch.cuda.synchronize()
    assert_guard(fw, nwork, "pc_grad work")
    ga2, gp2 = eng.pc_grad(dp, dq, D)
    assert torch.equal(ga, ga2) and torch.equal(gp, gp2)
    sa, sp, tol_a = torch.zeros_like(ga), torch.empty_like(gp), 0.0
    for s0 in range(0, n, 512):
        a, p = eng.pc_grad(dp[s0:s0 + 512], dq[s0:s0 + 512], D)
        sa += a
        sp[s0:s0 + 512] = p
        tol_a += TOL * max(1.0, float(a.abs().max()))
    ea, ep = float((ga - sa).abs().max()), float((gp - sp).abs().max())
    scale_p = max(1.0, float(sp.abs().max()))
    tol_a += TOL * max(1.0, float(ga.abs().max()))
    print(f"pc_grad n = {n}: atoms |big - slices| = {ea:.2e} (tol {tol_a:.2e}), sites {ep:.2e} (|g|max {scale_p:.2e})")
    assert ea <= tol_a and ep <= 2 * TOL * scale_p
