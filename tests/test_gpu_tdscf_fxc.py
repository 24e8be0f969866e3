"""Analytic XC response of closed-shell TDDFT (mi_xc_fxc_prep / mi_xc_fxc_apply) and DFT triplets.

Per point: the kernel coefficients against central differences of the first derivatives of mi_xc_eval / mi_xc_eval_spin.
Per molecule: the analytic dV against the difference quotient of the XC potential (xc_response = "fd"), triplet roots against
dense A, B from the oracle's ERI tensor and an f_T from central differences of the oracle's spin-polarised XC potential, the
HF limit against RHF triplets, and CAM-B3LYP triplets against dense operators built from the engine's full and long-range
ERI tensors."""
import numpy as np
import pytest

from conftest import MOLECULES

pytestmark = pytest.mark.gpu

OMEGA = 0.33
KINDS = [1, 2, 3, 4, 5, 6, 7, 12]
LDA_KINDS = (1, 3, 4)
_MF = {}


def _points(n=400, seed=2):
    """Densities 1e-9.7 .. 1e2 with reduced gradients 1e-2 .. 10^1.5, random directions."""
    rng = np.random.default_rng(seed)
    rho = 10.0 ** rng.uniform(-9.7, 2, n)
    g = rho ** (4.0 / 3) * 10.0 ** rng.uniform(-2, 1.5, n)
    u = rng.standard_normal((3, n))
    u /= np.linalg.norm(u, axis=0)
    return rho, g * u


def _ityh_a(rho, sigma):
    """Argument a of the ITYH factor of a closed-shell point (its closed form and series meet at a = 4)."""
    r, s = 0.5 * rho, 0.25 * sigma
    x = np.sqrt(s) / r ** (4.0 / 3)
    K = 1.5 * (6 / np.pi) ** (1.0 / 3) + 2 * 0.0042 * x * x / (1 + 6 * 0.0042 * x * np.arcsinh(x))
    return OMEGA / (2 * np.sqrt(9 * np.pi / K) * r ** (1.0 / 3))


def _engine():
    from pyscf import gto
    from mi355scf import engine
    if "eng" not in _MF:
        _MF["eng"] = engine.Engine(gto.M(atom=MOLECULES["h2o"], basis="sto-3g", verbose=0))
    return _MF["eng"]


def _mask(kind, rho, sigma):
    """Points where differences of the first derivatives are a sound reference: B88-SR's vsigma is only good to ~1e-6 near
    the switch of the ITYH factor (test_gpu_rsh), which differences would amplify, and loses digits again far out on the
    series (a > 50, rho < ~1e-9), where the leading 1/(36 a^2) terms of F and a F'/2 cancel."""
    if kind != 12:
        return np.ones(rho.shape, dtype=bool)
    a = _ityh_a(rho, sigma)
    return (a < 1.0) | ((a > 6.0) & (a < 50.0))


def _diff(f, x, h):
    """Richardson-extrapolated central differences (error O(h^4)) of f, which returns a tuple of arrays, and the change
    against the plain difference at h/2 as the uncertainty of each: at low density the functionals vary on a scale of
    rho / 100 (LYP's exp(-c rho^(-1/3))), too fast for a plain difference at h = 1e-4 rho."""
    d1 = [(p - m) / (2 * h) for p, m in zip(f(x + h), f(x - h))]
    d2 = [(p - m) / h for p, m in zip(f(x + 0.5 * h), f(x - 0.5 * h))]
    return [(4 * b - a) / 3 for a, b in zip(d1, d2)], [np.abs(b - a) for a, b in zip(d1, d2)]


@pytest.mark.parametrize("kind", KINDS)
def test_singlet_coefficients_match_differences(kind):
    """w {f_rr, f_rs, f_ss, v_s} of the closed-shell channel against central differences of vrho, vsigma (mi_xc_eval): f_rr =
    d vrho/drho, f_rs = d vsigma/drho, f_ss = d vsigma/dsigma (d vrho/dsigma is ill-conditioned: vrho hardly depends on
    sigma at small reduced gradients).  Densities from 1e-8 up: below, LYP's exp(-c rho^(-1/3)) underflows and the differences
    carry no digits (the apply test below covers those points through the potential)."""
    import torch
    eng = _engine()
    dev = eng.device
    rho, grad = _points()
    keep = rho > 1e-8
    rho, grad = rho[keep], grad[:, keep]
    sigma = (grad * grad).sum(axis=0)
    gga = kind not in LDA_KINDS
    terms, prm = [(1.0, kind)], ([OMEGA] if kind == 12 else None)
    w = torch.full((len(rho),), 0.7, dtype=torch.float64, device=dev)
    R = torch.as_tensor(np.vstack([rho, grad]) if gga else rho[None], device=dev).contiguous()
    coef = eng.xc_fxc_prep(terms, R, w, gga, triplet=False, params=prm).cpu().numpy() / 0.7

    def raw(r, s):
        # the gradient along x with |grad|^2 = s
        g = np.vstack([r, np.sqrt(s), 0 * r, 0 * r]) if gga else r[None]
        _e, _wv, vr, vs = eng.xc_eval(terms, torch.as_tensor(g, device=dev).contiguous(), w, gga, want_raw=True, params=prm)
        return vr.cpu().numpy(), vs.cpu().numpy()
    vr, vs = raw(rho, sigma)
    hr, hs = 1e-4 * rho, 1e-4 * sigma
    (f_rr, f_rs), (u_rr, u_rs) = _diff(lambda r: raw(r, sigma), rho, hr)
    assert np.all(np.isfinite(coef))
    ok = _mask(kind, rho, sigma) & np.isfinite(f_rr)
    assert np.all(np.abs(coef[0] - f_rr)[ok] <= (1e-6 * (np.abs(f_rr) + 1e-3 * np.abs(vr) / rho) + u_rr)[ok]), kind
    if not gga:
        assert coef.shape[0] == 1
        return
    (_f_sr, f_ss), (_u_sr, u_ss) = _diff(lambda s: raw(rho, s), sigma, hs)
    ok &= np.isfinite(f_rs) & np.isfinite(f_ss)
    for what, got, ref, unc, scale in (("f_rs", coef[1], f_rs, u_rs, np.abs(vs) / rho), ("f_ss", coef[2], f_ss, u_ss, np.abs(vs) / sigma),
                                       ("v_s", coef[3], vs, 0.0 * vs, np.abs(vs))):
        # B88-SR's first derivatives are good to ~2e-9 of their scale (test_gpu_rsh); differences over steps of 1e-4 rho
        # turn that into up to ~2e-9 / 1e-4 of |vsigma| / rho (1.1e-8 seen where f_rs itself is small)
        tol = 1e-6 * (np.abs(ref) + 1e-3 * scale) + unc + (1e-7 * scale if kind == 12 else 0.0)
        err = np.abs(got - ref)
        bad = ok & (err > tol)
        assert not bad.any(), (kind, what, (err / tol)[bad], rho[bad], sigma[bad], got[bad], ref[bad], unc[bad] if np.ndim(unc) else unc)
    assert ok.sum() > 200


def _linearised(coef, rho0, rho1, gga):
    """wv1 of the apply kernel's formula in numpy, and the scale (sum of absolute terms) of each component."""
    c = coef
    if not gga:
        t = 0.5 * c[0] * rho1[0]
        return t[None], np.abs(t)[None]
    s1 = 2 * (rho0[1:] * rho1[1:]).sum(axis=0)
    a, b = 0.5 * c[0] * rho1[0], 0.5 * c[1] * s1
    out, sc = [a + b], [np.abs(a) + np.abs(b)]
    t = 2 * (c[1] * rho1[0] + c[2] * s1)
    for k in range(3):
        x, y = t * rho0[1 + k], 2 * c[3] * rho1[1 + k]
        out.append(x + y)
        sc.append(2 * (np.abs(c[1] * rho1[0]) + np.abs(c[2] * s1)) * np.abs(rho0[1 + k]) + np.abs(y))
    return np.array(out), np.array(sc)


@pytest.mark.parametrize("triplet", [False, True], ids=["singlet", "triplet"])
@pytest.mark.parametrize("kind", KINDS)
def test_apply_matches_differences_of_the_potential(kind, triplet):
    """wv1 of a batch of trial densities against d/dh of mi_xc_eval's wv at rho0 + h rho1 (singlet) or of mi_xc_eval_spin's
    wv_alpha at rho_a = (rho0 + h rho1)/2, rho_b = (rho0 - h rho1)/2 (triplet) -- every coefficient of the channel enters."""
    import torch
    eng = _engine()
    dev = eng.device
    rho, grad = _points(300, seed=5)
    gga = kind not in LDA_KINDS
    nc = 4 if gga else 1
    terms, prm = [(1.0, kind)], ([OMEGA] if kind == 12 else None)
    rng = np.random.default_rng(11)
    rho0 = np.vstack([rho, grad])[:nc]
    w = torch.as_tensor(rng.uniform(0.1, 2.0, len(rho)), device=dev)
    m = 3
    rho1 = np.empty((m, nc, len(rho)))
    for j in range(m):
        rho1[j, 0] = rho * rng.uniform(-1, 1, len(rho))
        if gga:
            rho1[j, 1:] = np.linalg.norm(grad, axis=0) * rng.uniform(-1, 1, (3, len(rho)))
    R0 = torch.as_tensor(rho0, device=dev).contiguous()
    coef = eng.xc_fxc_prep(terms, R0, w, gga, triplet=triplet, params=prm)
    wv1 = eng.xc_fxc_apply(R0, coef, torch.as_tensor(rho1, device=dev).contiguous(), gga).cpu().numpy()
    coef = coef.cpu().numpy()
    sigma = (grad * grad).sum(axis=0)
    ok = _mask(kind, rho, sigma)
    for j in range(m):
        ref_formula, scale = _linearised(coef, rho0, rho1[j], gga)
        assert np.array_equal(np.isfinite(wv1[j]), np.ones_like(wv1[j], dtype=bool))
        assert np.all(np.abs(wv1[j] - ref_formula) <= 1e-12 * scale + 1e-300)
        h = 1e-4

        def wv_at(s):
            if triplet:
                a = torch.as_tensor(0.5 * (rho0 + s * rho1[j]), device=dev).contiguous()
                b = torch.as_tensor(0.5 * (rho0 - s * rho1[j]), device=dev).contiguous()
                return eng.xc_eval_spin(terms, a, b, w, gga, params=prm)[1].cpu().numpy()
            r = torch.as_tensor(rho0 + s * rho1[j], device=dev).contiguous()
            return eng.xc_eval(terms, r, w, gga, params=prm)[1].cpu().numpy()
        (ref,), (unc,) = _diff(lambda s: (wv_at(s),), 0.0, h)
        # components whose response vanishes (PBE correlation's triplet gradient part: it depends on the total sigma only)
        # are judged against the potential itself: 1e-8 of |wv(rho0)|
        floor = 1e-8 * np.abs(wv_at(0.0))
        # the first-derivative kernels return NaN at a few extreme points of PBE correlation (rho ~ 1e-9, large gradients)
        okj = ok[None, :] & np.isfinite(ref)
        assert okj.sum() > 0.9 * ok.sum() * ref.shape[0]
        tol = 1e-6 * (np.abs(ref) + scale) + unc + floor
        err = np.abs(wv1[j] - ref)
        bad = okj & (err > tol)
        assert not bad.any(), (kind, triplet, j, rho[np.nonzero(bad)[1]], (err / tol)[bad])


def test_meta_gga_kinds_are_refused():
    import torch
    from mi355scf import engine
    eng = _engine()
    R = torch.ones(4, 8, dtype=torch.float64, device=eng.device)
    w = torch.ones(8, dtype=torch.float64, device=eng.device)
    for kind in (8, 9, 10, 11):
        with pytest.raises(engine.EngineError):
            eng.xc_fxc_prep([(1.0, kind)], R, w, True)


# ---------------------------------------------------------------------------------------------
# molecules
# ---------------------------------------------------------------------------------------------
def _rks(xc, name="h2o"):
    key = (xc, name)
    if key not in _MF:
        from pyscf import gto, dft
        mol = gto.M(atom=MOLECULES[name], basis="6-31g(d)", verbose=0)
        mf = dft.RKS(mol)
        mf.xc = xc
        mf.conv_tol = 1e-11
        mf.kernel()
        assert mf.converged
        _MF[key] = (mol, mf)
    return _MF[key]


@pytest.mark.parametrize("xc", ["SVWN", "BLYP", "PBE", "B3LYP", "PBE0", "CAM-B3LYP"])
def test_analytic_response_matches_difference_quotient(xc):
    import torch
    from pyscf import tdscf
    mol, mf = _rks(xc)
    td = tdscf.TDA(mf)
    td._setup()
    rng = np.random.default_rng(3)
    a = rng.standard_normal((3, mol.nao, mol.nao)) * 0.1
    Ms = torch.as_tensor(0.5 * (a + a.transpose(0, 2, 1)), device=td._de.device)
    for triplet in (False, True):
        td.xc_response = "analytic"
        got = td._dvxc(Ms, triplet=triplet).cpu().numpy()
        td.xc_response = "fd"
        ref = td._dvxc(Ms, triplet=triplet).cpu().numpy()
        for m in range(Ms.shape[0]):
            assert np.abs(got[m] - ref[m]).max() <= 1e-6 * np.abs(ref[m]).max(), (xc, triplet, np.abs(got[m] - ref[m]).max())
    assert td.stats["xc_vectors"] == 4 * Ms.shape[0]
    # singlet roots of both routes
    for cls in (tdscf.TDA, tdscf.TDDFT):
        e = []
        for route in ("analytic", "fd"):
            t = cls(mf)
            t.nstates, t.conv_tol, t.xc_response = 5, 1e-11, route
            e.append(t.kernel()[0])
            assert t.converged.all()
        assert np.abs(e[0] - e[1]).max() < 1e-7, (xc, cls.__name__, e)


def _oracle_vxc_alpha(ao, w, terms, Da, Db, rho_cut=1e-10):
    """The oracle's V_xc of spin alpha (oracle.dft.eval_xc_spin) on the points of `ao`, with the engine's cut-off."""
    from oracle import dft as odft
    rho, grad = [], []
    for D in (Da, Db):
        c0 = ao[0] @ D
        rho.append(np.maximum(np.einsum("gi,gi->g", ao[0], c0), 0.0))
        grad.append(np.array([2 * np.einsum("gi,gi->g", ao[1 + k], c0) for k in range(3)]))
    ok = rho[0] + rho[1] > rho_cut
    ra, rb = np.where(ok, rho[0], 0.5), np.where(ok, rho[1], 0.5)
    saa, sab, sbb = ((grad[0] * grad[0]).sum(0), (grad[0] * grad[1]).sum(0), (grad[1] * grad[1]).sum(0))
    _e, d = odft.eval_xc_spin(terms, ra, rb, saa, sab, sbb)
    vra, vaa, vab = (np.where(ok, x, 0.0) for x in (d[0], d[2], d[3]))
    aow = ao[0] * (0.5 * w * vra)[:, None]
    for k in range(3):
        aow += ao[1 + k] * (w * (2 * vaa * grad[0][k] + vab * grad[1][k]))[:, None]
    v = ao[0].T @ aow
    return v + v.T


def _triplet_ab(mf, eri, eri_lr, hyb, alpha, dvt):
    """Dense A_T, B_T: exchange -hyb (oovv | ovvo) - (alpha - hyb) (oovv | ovvo)_LR plus f_T = [dvt(2 D_s)]_ov per unit amplitude."""
    C, e = np.asarray(mf.mo_coeff), np.asarray(mf.mo_energy)
    no = int((np.asarray(mf.mo_occ) > 0).sum())
    Co, Cv = C[:, :no], C[:, no:]
    nv = Cv.shape[1]
    n = no * nv

    def exch(g):
        oovv = np.einsum("pqrs,pi,qj,ra,sb->ijab", g, Co, Co, Cv, Cv, optimize=True).transpose(0, 2, 1, 3).reshape(n, n)
        ovvo = np.einsum("pqrs,pi,qa,rj,sb->iajb", g, Co, Cv, Co, Cv, optimize=True).transpose(0, 3, 2, 1).reshape(n, n)
        return oovv, ovvo
    oovv, ovvo = exch(eri)
    A, B = -hyb * oovv, -hyb * ovvo
    if eri_lr is not None:
        oovv_lr, ovvo_lr = exch(eri_lr)
        A, B = A - (alpha - hyb) * oovv_lr, B - (alpha - hyb) * ovvo_lr
    fT = np.zeros((n, n))
    for j in range(no):
        for b in range(nv):
            Dt = np.outer(Co[:, j], Cv[:, b]) + np.outer(Cv[:, b], Co[:, j])
            fT[:, j * nv + b] = (Co.T @ dvt(Dt) @ Cv).reshape(-1)
    de = (e[no:][None, :] - e[:no, None]).reshape(-1)
    A, B = np.diag(de) + A + fT, B + fT
    assert np.abs(A - A.T).max() < 1e-6
    return 0.5 * (A + A.T), 0.5 * (B + B.T)


def _check_triplet_roots(mf, A, B, ns=5, tol=1e-6):
    from pyscf import tdscf
    td = tdscf.TDA(mf)
    td.singlet, td.nstates, td.conv_tol = False, ns, 1e-11
    e, _ = td.kernel()
    assert td.converged.all()
    assert np.abs(e - np.linalg.eigvalsh(A)[:ns]).max() < tol, (e, np.linalg.eigvalsh(A)[:ns])
    assert np.all(td.oscillator_strength() == 0.0)
    rp = tdscf.TDDFT(mf)
    rp.singlet, rp.nstates, rp.conv_tol = False, ns, 1e-11
    e2, xy = rp.kernel()
    ref = np.sort(np.sqrt(np.linalg.eigvals((A - B) @ (A + B)).real))[:ns]
    assert rp.converged.all()
    assert np.abs(e2 - ref).max() < tol, (e2, ref)
    for x, y in xy:
        assert abs((x * x).sum() - (y * y).sum() - 0.5) < 1e-9
    return e, e2


@pytest.mark.parametrize("xc", ["B3LYP", "PBE", "SVWN"])
def test_triplet_roots_match_dense_oracle(xc):
    from oracle import dft as odft, oracle as orc
    mol, mf = _rks(xc)
    hyb, terms = odft.parse_xc(xc)
    ao = odft.eval_ao(mol, mf.grids.coords.cpu().numpy(), 1)
    w = mf.grids.weights.cpu().numpy()
    D0 = np.asarray(mf.make_rdm1())

    def dvt(M, step=1e-4):
        s = step / np.abs(M).max()
        Dp, Dm = 0.5 * (D0 + s * M), 0.5 * (D0 - s * M)
        return (_oracle_vxc_alpha(ao, w, terms, Dp, Dm) - _oracle_vxc_alpha(ao, w, terms, Dm, Dp)) / (2 * s)
    A, B = _triplet_ab(mf, orc.Oracle(mol).eri_full(), None, hyb, hyb, dvt)
    _check_triplet_roots(mf, A, B)


def test_hf_limit_equals_rhf_triplets():
    """An RKS object with xc = "HF" (no semilocal terms: zero XC response) gives the RHF triplet roots."""
    from pyscf import gto, scf, dft, tdscf
    mol = gto.M(atom=MOLECULES["h2o"], basis="6-31g(d)", verbose=0)
    rks = dft.RKS(mol)
    rks.xc = "HF"
    out = []
    for mf in (scf.RHF(mol), rks):
        mf.conv_tol = 1e-12
        mf.kernel()
        assert mf.converged
        roots = []
        for cls in (tdscf.TDA, tdscf.TDHF):
            td = cls(mf)
            td.singlet, td.nstates, td.conv_tol = False, 5, 1e-12
            roots.append(td.kernel()[0])
            assert td.converged.all()
        out.append(roots)
    for a, b in zip(*out):
        assert np.abs(a - b).max() < 1e-8, (a, b)


def test_cam_b3lyp_triplets_match_dense_engine_operators():
    import torch
    from pyscf import tdscf
    from mi355scf.dft import lr_engine, rsh_coeff
    mol, mf = _rks("CAM-B3LYP")
    _omega, alpha, hyb = rsh_coeff("CAM-B3LYP")
    eri = mf.engine.eri_dense().cpu().numpy()
    eri_lr = lr_engine(mf).eri_dense().cpu().numpy()
    td = tdscf.TDA(mf)
    td._setup()

    def dvt(M):
        Mt = torch.as_tensor(M[None], device=td._de.device)
        return td._dvxc_fd(Mt, triplet=True)[0].cpu().numpy()
    A, B = _triplet_ab(mf, eri, eri_lr, hyb, alpha, dvt)
    _check_triplet_roots(mf, A, B)


def test_cam_b3lyp_h2co_lowest_triplet_below_singlet():
    from pyscf import tdscf
    _mol, mf = _rks("CAM-B3LYP", "h2co")
    e = {}
    for singlet in (True, False):
        td = tdscf.TDA(mf)
        td.singlet, td.nstates = singlet, 3
        e[singlet] = td.kernel()[0]
        assert td.converged.all()
    assert e[False][0] < e[True][0], e
