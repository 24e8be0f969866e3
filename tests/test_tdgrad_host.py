"""TDA/TDDFT excited-state gradients, the parts that need no GPU: the decomposition of the excited state's two-particle density
into the `(Q, s, R, t, sym)` of `Engine.grad_eri` (`tdscf_grad.two_particle_terms`, plain NumPy), the difference-density
identities, the argument checks of the Python wrapper, and the public surface with its refusals."""
import numpy as np
import pytest

from conftest import MOLECULES

N = 7


def _sym8(n, seed):
    """Random tensor with the 8-fold symmetry of real two-electron integrals."""
    x = np.random.default_rng(seed).standard_normal((n, n, n, n))
    x = x + x.transpose(1, 0, 2, 3)
    x = x + x.transpose(0, 1, 3, 2)
    return x + x.transpose(2, 3, 0, 1)


def _coul(eri, A, B):
    return float(np.einsum("ijkl,ij,kl->", eri, A, B))


def _ex(eri, A, B):
    """sum_ijkl (ik|jl) A_ij B_kl"""
    return float(np.einsum("ikjl,ij,kl->", eri, A, B))


def _e2_formula(eri, D, M, hyb, Q, s, R, t):
    """The functional whose gradient `mi_grad_eri_xpairs` evaluates (include/mi355scf.h)."""
    e = 0.5 * _coul(eri, D, D) - 0.25 * hyb * _ex(eri, D, D)
    if M is not None:
        e -= 0.25 * hyb * _ex(eri, M, M)
    e += 0.5 * sum(s[k] * _coul(eri, Q[k], Q[k]) for k in range(len(s)))
    return e + sum(t[m] * _ex(eri, R[m], R[m]) for m in range(len(t)))


def _state(n, nocc, tda, seed):
    """Random orthonormal orbitals, amplitudes normalised as `td.xy` (X.X - Y.Y = 1/2) and a random symmetric relaxation Z."""
    rng = np.random.default_rng(seed)
    C = np.linalg.qr(rng.standard_normal((n, n)))[0]
    Co, Cv = C[:, :nocc], C[:, nocc:]
    x = rng.standard_normal((nocc, n - nocc))
    y = np.zeros_like(x) if tda else 0.3 * rng.standard_normal(x.shape)
    nrm = np.sqrt(0.5 / (np.sum(x * x) - np.sum(y * y)))
    x, y = x * nrm, y * nrm
    z = rng.standard_normal(x.shape)
    return Co, Cv, x, y, z


@pytest.mark.parametrize("hyb", [0.0, 0.2, 1.0])
@pytest.mark.parametrize("tda", [True, False])
def test_decomposition_reproduces_the_two_particle_contraction(tda, hyb):
    """Direct contraction (Furche-Ahlrichs, AO basis): the ground state's Hartree-Fock form, the relaxed difference density P
    in the ground state's field, and the (A+B) / (A-B) two-electron parts of the excitation energy,
        1/2 (D0|D0) - c/4 ex(D0, D0) + (P|D0) - c/2 ex(P, D0) + sum_iajb [4 (ia|jb) - c (ij|ab) - c (ib|ja)] u_ia u_jb
                                                                    + sum_iajb c [(ib|ja) - (ij|ab)] v_ia v_jb."""
    from mi355scf import tdscf_grad as tg
    nocc = 3
    Co, Cv, x, y, z = _state(N, nocc, tda, 11 + int(tda))
    eri = _sym8(N, 21)
    u, v = x + y, x - y
    doo, dvv = tg.difference_density(x, y)
    Zao = Co @ z @ Cv.T
    P = Co @ doo @ Co.T + Cv @ dvv @ Cv.T + 0.5 * (Zao + Zao.T)
    D0 = 2.0 * Co @ Co.T
    Nu, Nv = Co @ u @ Cv.T, Co @ v @ Cv.T
    U, V = 0.5 * (Nu + Nu.T), 0.5 * (Nv - Nv.T)
    ovov = np.einsum("pqrs,pi,qa,rj,sb->iajb", eri, Co, Cv, Co, Cv, optimize=True)
    oovv = np.einsum("pqrs,pi,qj,ra,sb->ijab", eri, Co, Co, Cv, Cv, optimize=True)
    apb = 4.0 * ovov - hyb * (oovv.transpose(0, 2, 1, 3) + ovov.transpose(0, 3, 2, 1))
    amb = hyb * (ovov.transpose(0, 3, 2, 1) - oovv.transpose(0, 2, 1, 3))
    direct = (0.5 * _coul(eri, D0, D0) - 0.25 * hyb * _ex(eri, D0, D0) + _coul(eri, P, D0) - 0.5 * hyb * _ex(eri, P, D0)
              + float(np.einsum("iajb,ia,jb->", apb, u, u)) + float(np.einsum("iajb,ia,jb->", amb, v, v)))
    D, Q, s, R, t, sym = tg.two_particle_terms(D0, P, U, V, hyb)
    assert Q.shape == (len(s), N, N) and R.shape == (len(t), N, N) and len(sym) == len(t) <= 8
    for m in range(len(t)):
        assert np.abs(R[m] - sym[m] * R[m].T).max() < 1e-14 and sym[m] in (1, -1)
    assert np.abs(Q - Q.transpose(0, 2, 1)).max() < 1e-14
    if hyb == 0.0:
        assert len(t) == 0           # no exchange term without exact exchange
    else:
        assert -1 in list(sym) and np.abs(V).max() > 1e-3
    got = _e2_formula(eri, D, None, hyb, Q, s, R, t)
    err = abs(got - direct) / max(1.0, abs(direct))
    print(f"tda={tda} hyb={hyb}: direct {direct:+.10f}, through (Q, s, R, t, sym) {got:+.10f}, relative difference {err:.1e}")
    assert err < 1e-12


@pytest.mark.parametrize("tda", [True, False])
def test_difference_density_identities(tda):
    from mi355scf import tdscf_grad as tg
    _Co, _Cv, x, y, _z = _state(N, 3, tda, 31)
    assert abs(np.sum(x * x) - np.sum(y * y) - 0.5) < 1e-14            # the normalisation of td.xy
    doo, dvv = tg.difference_density(x, y)
    assert doo.shape == (3, 3) and dvv.shape == (N - 3, N - 3)
    assert np.abs(doo - doo.T).max() < 1e-15 and np.abs(dvv - dvv.T).max() < 1e-15
    assert abs(np.trace(doo) + np.trace(dvv)) < 1e-14                  # tr T = 0: no change of the electron count
    assert abs(np.trace(dvv) - 2.0 * (np.sum(x * x) + np.sum(y * y))) < 1e-14
    if tda:
        assert abs(np.trace(dvv) - 1.0) < 1e-14                        # one electron promoted
    assert np.linalg.eigvalsh(dvv).min() > -1e-14 and np.linalg.eigvalsh(doo).max() < 1e-14


def test_xpairs_arguments_are_checked_before_any_launch():
    import torch
    from mi355scf import engine
    n = 5
    R = torch.zeros(2, n, n, dtype=torch.float64)
    ok = engine.xpairs_args((R, [0.5, -2.0], [1, -1]), n, "cpu")
    assert ok[3] == 2 and ok[1].dtype == np.float64 and ok[2].dtype == np.intc and list(ok[2]) == [1, -1]
    assert engine.xpairs_args((None, [], []), n, "cpu")[3] == 0
    with pytest.raises(ValueError, match="at most 8"):
        engine.xpairs_args((torch.zeros(9, n, n, dtype=torch.float64), [1.0] * 9, [1] * 9), n, "cpu")
    with pytest.raises(ValueError, match="finite"):
        engine.xpairs_args((R, [0.5, float("inf")], [1, -1]), n, "cpu")
    with pytest.raises(ValueError, match="finite"):
        engine.xpairs_args((R, [float("nan"), 1.0], [1, -1]), n, "cpu")
    with pytest.raises(ValueError, match=r"\+1 \(symmetric\) or -1"):
        engine.xpairs_args((R, [0.5, 1.0], [1, 0]), n, "cpu")
    with pytest.raises(ValueError, match="symmetry flags"):
        engine.xpairs_args((R, [0.5, 1.0], [1]), n, "cpu")
    with pytest.raises(ValueError, match="contiguous"):
        engine.xpairs_args((torch.zeros(2, n, 2 * n, dtype=torch.float64)[:, :, ::2], [0.5, 1.0], [1, 1]), n, "cpu")
    with pytest.raises(ValueError, match="contiguous"):
        engine.xpairs_args((None, [0.5], [1]), n, "cpu")
    with pytest.raises(ValueError, match="contiguous"):
        engine.xpairs_args((R.float(), [0.5, 1.0], [1, 1]), n, "cpu")
    with pytest.raises(ValueError, match="contiguous"):
        engine.xpairs_args((torch.zeros(2, n, n + 1, dtype=torch.float64), [0.5, 1.0], [1, 1]), n, "cpu")
    with pytest.raises(ValueError, match=r"\(R, t, sym\)"):
        engine.xpairs_args((R, [0.5, 1.0]), n, "cpu")


def _objects(xc=None):
    from pyscf import dft, gto, scf
    mol = gto.M(atom=MOLECULES["h2o"], basis="sto-3g", verbose=0)
    mf = scf.RHF(mol) if xc is None else dft.RKS(mol)
    if xc is not None:
        mf.xc = xc
    mf.mo_coeff = np.eye(mol.nao)                   # never run: nothing here may touch the GPU
    return mol, mf


def test_surface_and_refusals(monkeypatch):
    import gpu4pyscf.tdscf
    import pyscf.tdscf
    from mi355scf import engine, tdscf_grad

    def no_gpu(*a, **k):
        raise AssertionError("constructing the gradient object opened the engine")
    monkeypatch.setattr(engine, "lib", no_gpu)
    monkeypatch.setattr(engine.Engine, "__init__", no_gpu)
    for mod in (pyscf.tdscf, gpu4pyscf.tdscf):
        for make in (mod.TDA, mod.TDHF, mod.TDDFT, mod.CIS, mod.RPA):
            mol, mf = _objects()
            td = make(mf)
            g = td.nuc_grad_method()
            assert isinstance(g, tdscf_grad.Gradients) and isinstance(td.Gradients(), tdscf_grad.Gradients)
            assert g.base is td and g.mol is mol and g.de is None and g.state == 1 and g.converged is False
            assert g.algorithm == "onepass" and g.timing == {}
            assert g.conv_tol > 0 and g.max_cycle > 0 and g.xc3_step > 0
            assert g.grad.__func__ is g.kernel.__func__
            sc = g.as_scanner(state=2)
            assert callable(sc) and sc.base is td and sc.mol is mol and sc.state == 2 and g.state == 2
            assert callable(td._log) and td.mol is mol      # what geomopt.optimize asks of its argument
    mol, mf = _objects()
    td = pyscf.tdscf.TDA(mf)
    g = td.nuc_grad_method()
    g.algorithm = "loop"
    with pytest.raises(ValueError, match="algorithm"):
        g.algorithm = "naive"
    with pytest.raises(ValueError, match="algorithm"):
        tdscf_grad.Gradients(td, algorithm="torch")
    td.singlet = False
    with pytest.raises(NotImplementedError, match="triplet"):
        td.nuc_grad_method()
    with pytest.raises(NotImplementedError, match="triplet"):
        g.kernel(state=1)
    _mol, mks = _objects("camb3lyp")
    with pytest.raises(NotImplementedError, match="range-separated"):
        pyscf.tdscf.TDDFT(mks).nuc_grad_method()
    # a state above nstates / an unconverged root, on a response object that holds (made-up) solutions
    _mol, mf = _objects()
    td = pyscf.tdscf.TDA(mf)
    nov = 5 * 2
    td.e = np.array([0.3, 0.4])
    td.xy = [(np.zeros((5, 2)), np.zeros((5, 2)))] * 2
    td.converged = np.array([True, False])
    g = td.nuc_grad_method()
    with pytest.raises(NotImplementedError, match="above nstates"):
        g.kernel(state=3)
    with pytest.raises(NotImplementedError, match="not converged"):
        g.kernel(state=2)
    assert nov == 10


def test_pcm_references_are_refused():
    import pyscf.tdscf
    from mi355scf import tdscf, tdscf_grad
    _mol, mf = _objects()
    mf._pcm = True
    with pytest.raises(NotImplementedError, match="PCM"):
        pyscf.tdscf.TDA(mf)                          # the response itself is not available with PCM ...
    td = tdscf.TDA(mf)
    with pytest.raises(NotImplementedError, match="PCM"):
        tdscf_grad.Gradients(td)                     # ... and the gradient refuses on its own
    with pytest.raises(NotImplementedError, match="PCM"):
        td.nuc_grad_method()


def test_scanner_guess_from_previous_vectors():
    """`kernel(x0=...)`: the previous (X, Y) become Davidson trial vectors (CPU tensors here; Y = 0 contributes none)."""
    import torch
    from mi355scf import tdscf
    _mol, mf = _objects()
    td = tdscf.TDA(mf)
    td._nocc, td._nvir = 2, 3
    td._de = torch.arange(1.0, 7.0, dtype=torch.float64)
    assert td._guess(None) is None
    x = np.arange(6.0).reshape(2, 3) + 1.0
    gs = td._guess([(x, np.zeros_like(x)), (2 * x, 0.1 * x)])
    assert gs.shape == (3, 6) and gs.dtype == torch.float64
    assert np.allclose(gs[0].numpy(), x.ravel()) and np.allclose(gs[2].numpy(), 0.1 * x.ravel())
    assert td._guess([(np.zeros((3, 3)), np.zeros((3, 3)))]) is None      # another orbital space: the default guess


def test_entry_point_is_exported_and_declared():
    import os
    import re
    from conftest import ROOT
    sub = os.path.join(ROOT, "computational-chemistry-ai_amd")
    hdr = open(os.path.join(ROOT, "include", "mi355scf.h")).read()
    src = open(os.path.join(sub, "csrc", "mi355scf.hip")).read()
    py = open(os.path.join(sub, "python", "mi355scf", "engine.py")).read()
    assert re.search(r"int mi_grad_eri_xpairs\(mi_ctx \*", hdr)
    assert 'extern "C" int mi_grad_eri_xpairs(' in src
    assert "L.mi_grad_eri_xpairs.argtypes" in py
