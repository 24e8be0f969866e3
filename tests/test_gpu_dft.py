"""GPU parity for the DFT rows (a7-a9): grids, AO values, XC functionals, nr_rks and RKS energies vs the
numpy oracle (oracle/dft.py).  Tolerances written per check; energies 1e-7 Ha (north_star: 1e-6)."""
import numpy as np
import pytest
import torch

from conftest import MOLECULES

pytestmark = pytest.mark.gpu


def _mol(name, basis):
    from mi355scf.mole import Mole
    return Mole(atom=MOLECULES[name], basis=basis, verbose=0).build()


@pytest.mark.parametrize("name", ["h2o", "h2co"])
def test_becke_grid_matches_oracle(name):
    from mi355scf.engine import Engine
    from mi355scf.grids import Grids
    from oracle import dft as odft
    mol = _mol(name, "6-31g")
    g = Grids(mol).build(engine=Engine(mol))
    c, w = odft.build_grids(mol, 3)
    assert g.size == len(w)
    assert np.abs(g.coords.cpu().numpy() - c).max() < 1e-12
    assert np.abs(g.weights.cpu().numpy() - w).max() < 1e-12 * max(1.0, np.abs(w).max())
    # a normalised Gaussian on each atom integrates to 1
    R = mol.atom_coords()
    for ia in range(mol.natm):
        val = (w * np.exp(-((c - R[ia]) ** 2).sum(1)) / np.pi ** 1.5).sum()
        assert abs(val - 1) < 1e-6


@pytest.mark.parametrize("basis", ["cc-pvdz", "cc-pvtz"])
def test_eval_ao_matches_oracle(basis):
    from mi355scf.engine import Engine
    from oracle import dft as odft
    mol = _mol("h2o", basis)
    eng = Engine(mol)
    rng = np.random.default_rng(0)
    pts = rng.normal(size=(500, 3)) * 1.5
    ao = eng.eval_ao(torch.as_tensor(pts, device=eng.device), deriv=1).cpu().numpy()  # [4][nao][ng]
    ref = odft.eval_ao(mol, pts, 1)  # [4][ng][nao]
    assert np.abs(ao.transpose(0, 2, 1) - ref).max() < 1e-11


@pytest.mark.parametrize("xc", ["LDA,VWN", "B3LYP", "PBE", "BLYP"])
def test_xc_functional_matches_oracle_complex_step(xc):
    from mi355scf.engine import Engine
    from mi355scf.dft import parse_xc
    from oracle import dft as odft
    eng = Engine(_mol("h2o", "sto-3g"))
    hyb, terms, gga = parse_xc(xc)
    ohyb, oterms = odft.parse_xc(xc)
    assert hyb == ohyb
    rng = np.random.default_rng(5)
    n = 4000
    rho = 10 ** rng.uniform(-6, 2, n)
    grad = rng.normal(size=(3, n)) * rho ** (4.0 / 3) * 10 ** rng.uniform(-2, 0.7, n)
    r4 = torch.as_tensor(np.vstack([rho[None], grad]), device=eng.device).contiguous()
    w = torch.ones(n, dtype=torch.float64, device=eng.device)
    e, wv, vr, vs = eng.xc_eval(terms, r4, w, True, want_raw=True)
    sigma = (grad ** 2).sum(0)
    eo, vro, vso = odft.eval_xc(oterms, rho, sigma)
    scale = np.maximum(np.abs(eo), 1e-12)
    assert (np.abs(e.cpu().numpy() - eo) / scale).max() < 1e-11
    # derivatives: error measured in energy units (dv * rho, dv * sigma) relative to |e| -- at extreme
    # reduced gradients the PBE-c derivative is a difference of large terms in BOTH implementations
    assert (np.abs(vr.cpu().numpy() - vro) * rho / scale).max() < 1e-9
    if gga:
        assert (np.abs(vs.cpu().numpy() - vso) * sigma / scale).max() < 1e-9


@pytest.mark.parametrize("xc", ["LDA,VWN", "B3LYP", "PBE"])
def test_nr_rks_matches_oracle(xc):
    from pyscf import gto, dft
    from oracle import dft as odft
    mol = _mol("h2o", "cc-pvdz")
    mf = dft.RKS(mol)
    mf.xc = xc
    mf.small_rho_cutoff = 0      # compare on the unpruned grid
    mf._setup_once()
    rng = np.random.default_rng(3)
    c = rng.normal(size=(mol.nao, 5)) * 0.3
    dm = 2 * c @ c.T
    n, exc, v, hyb = mf.nr_rks(torch.as_tensor(dm, device=mf.engine.device))
    co, wo = odft.build_grids(mol, 3)
    no, eo, vo, ho = odft.nr_rks(mol, co, wo, xc, dm)
    assert abs(float(n) - no) < 1e-9 and abs(float(exc) - eo) < 1e-9
    assert np.abs(v.cpu().numpy() - vo).max() < 1e-9


@pytest.mark.parametrize("xc,e_mem", [("LDA,VWN", None), ("B3LYP", None), ("PBE", None)])
def test_rks_energy_matches_oracle(xc, e_mem):
    import gpu4pyscf
    from pyscf import gto
    from oracle import dft as odft
    mol = gto.Mole()
    mol.atom = MOLECULES["h2o"]
    mol.basis = "cc-pVDZ"
    mol.verbose = 0
    mol.build()
    mf = gpu4pyscf.dft.RKS(mol).to_gpu()
    mf.xc = xc  # assigned after to_gpu(), as templates/optimize_geometry.py:72-73 does
    e = mf.kernel()
    assert mf.converged
    ref = odft.rks(mol, xc, dm0=mf.get_init_guess())
    assert abs(e - ref["e_tot"]) < 1e-7, (e, ref["e_tot"])
    assert abs(float(mf._nelec_grid) - 10.0) < 1e-5


@pytest.mark.parametrize("key,mol_name,xc", [("benzene_ccpvdz_b3lyp", "benzene", "B3LYP"), ("h2o_ccpvdz_pbe", "h2o", "PBE")])
def test_rks_energy_vs_committed_oracle_golden(key, mol_name, xc):
    """tests/golden/energies.json (made by tests/golden/make_golden.py with oracle/dft.py)."""
    import json, os
    from pyscf import gto, dft
    from mi355scf import fixtures
    g = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "energies.json")))[key]
    mol = gto.Mole()
    mol.atom = fixtures.BENZENE if mol_name == "benzene" else fixtures.H2O
    mol.basis = "cc-pVDZ"
    mol.verbose = 0
    mol.build()
    mf = dft.RKS(mol).to_gpu()
    mf.xc = xc
    e = mf.kernel()
    # pruned grid sizes differ slightly: the oracle prunes with its core-Hamiltonian guess, the product with the atomic guess
    assert mf.converged and abs(mf.grids.size - g["ngrids"]) < 0.06 * g["ngrids"]
    assert abs(e - g["e_tot"]) < 2e-7, (e, g["e_tot"])
    assert abs(float(mf._nelec_grid) - g["nelec_grid"]) < 1e-7


def test_vxc_product_with_weighted_aos_formed_in_kernel_matches_two_pass_path():
    """`mi_xc_vmat_fold` (round-3 experiment, default off: DESIGN.md 8.8) forms sum_c wv_c ao_c inside the MFMA kernel; it must give
    the V_xc matrix of the xc_aow + xc_vmat pair (LDA and GGA, N not a multiple of 64, several row blocks)."""
    from pyscf import gto, dft
    mol = gto.Mole()
    mol.atom, mol.basis, mol.verbose = "C 0 0 0; O 1.2 0 0; H -0.5 0.9 0; H -0.5 -0.9 0", "cc-pVDZ", 0
    mol.build()
    for xc in ("LDA,VWN", "PBE", "B3LYP"):
        ref = dft.RKS(mol); ref.xc = xc
        ref.kernel()
        dm = ref.make_rdm1()
        v0 = ref.get_veff(dm=dm)
        ref.xc_vmat_fold = True          # same object: same (pruned) grid, same AO cache
        for mt in (1, 3, 5):
            ref.engine.set_option("vmat_fold_mt", mt)
            v1 = ref.get_veff(dm=dm)
            assert np.abs(v1 - v0).max() < 1e-10, (xc, mt, np.abs(v1 - v0).max())
        assert np.abs(v0).max() > 0.1


# --- the per-point XC entry points at the edges of their launch (one kernel per grid point, 256 per workgroup) ---------------
B3LYP_TERMS = [(0.08, 1), (0.72, 2), (0.19, 3), (0.81, 5)]
TPSS_TERMS = [(1.0, 8), (1.0, 9)]
_XC_EDGE = {}


def _xc_points():
    """(engine, 512 fixed points): spin densities in [1e-3, 2] with their gradients, tau and weights; a few densities exactly 0
    and point 0 with rho_a + rho_b below the kernels' 1e-10 cut (it is in every prefix, ng = 1 included)."""
    if not _XC_EDGE:
        from mi355scf.engine import Engine
        eng = Engine(_mol("h2o", "sto-3g"))
        rng = np.random.default_rng(20240613)
        n = 512
        r = rng.uniform(1e-3, 2.0, (2, n))
        r[:, 0] = (3e-11, 2e-11)
        r[0, [5, 200, 256]] = 0.0
        r[1, [7, 200, 300]] = 0.0           # point 200: both spins empty
        g = rng.normal(size=(2, 3, n)) * r[:, None, :] ** (4.0 / 3)
        tau = rng.uniform(0.05, 3.0, (2, n)) * r ** (5.0 / 3) + (g ** 2).sum(1) / (8.0 * np.maximum(r, 1e-300))
        dev = eng.device
        _XC_EDGE.update(eng=eng, n=n, w=torch.as_tensor(rng.uniform(0.1, 2.0, n), device=dev),
                        rho=[torch.as_tensor(np.vstack([r[s][None], g[s]]), device=dev) for s in range(2)],
                        tau=[torch.as_tensor(tau[s], device=dev) for s in range(2)])
    return _XC_EDGE


def _xc_edge_call(case, ng):
    """Outputs (a tuple of tensors) of one wrapper on the first `ng` points, inputs sliced into contiguous [(1|4), ng]."""
    p = _xc_points()
    eng, w = p["eng"], p["w"][:ng].contiguous()
    ra, rb = (x[:, :ng].contiguous() for x in p["rho"])
    ta, tb = (x[:ng].contiguous() for x in p["tau"])
    tot, ttot = (ra + rb).contiguous(), (ta + tb).contiguous()
    kind, gga = case.split("-")[0], not case.endswith("lda")
    if kind == "eval":
        return eng.xc_eval(B3LYP_TERMS, tot if gga else tot[:1].contiguous(), w, gga, want_raw=True)
    if kind == "spin":
        return eng.xc_eval_spin(B3LYP_TERMS, ra if gga else ra[:1].contiguous(), rb if gga else rb[:1].contiguous(), w, gga)
    if kind == "mgga":
        return eng.xc_eval_mgga(TPSS_TERMS, tot, ttot, w)
    if kind == "mggaspin":
        return eng.xc_eval_mgga_spin(TPSS_TERMS, ra, rb, ta, tb, w)
    return (eng.xc_fxc_prep(B3LYP_TERMS, tot, w, True, triplet=case.endswith("triplet")),)


XC_EDGE_CASES = ["eval-lda", "eval-gga", "spin-lda", "spin-gga", "mgga", "mggaspin", "fxc-singlet", "fxc-triplet"]


@pytest.mark.parametrize("case", XC_EDGE_CASES)
def test_xc_entry_points_at_workgroup_edges(case, monkeypatch):
    """ng = 1, 255, 256, 257 (one thread, one short of / exactly / one past a 256-thread workgroup): every output equals bit for
    bit the first ng entries of each component of the 512-point evaluation (the arithmetic is per point), and the guard words
    behind each output buffer are untouched."""
    from test_gpu_dense_kernels import assert_guard, guarded
    p = _xc_points()
    eng = p["eng"]
    full = [o.cpu().numpy() for o in _xc_edge_call(case, p["n"])]
    flats = []

    def guarded_new(*shape):
        size = int(np.prod(shape))
        flats.append((guarded(size), size))
        return flats[-1][0][:size].view(*shape)

    monkeypatch.setattr(eng, "_new", guarded_new)
    for ng in (1, 255, 256, 257):
        del flats[:]
        outs = _xc_edge_call(case, ng)
        torch.cuda.synchronize()
        assert len(flats) == len(full)
        for o, ref in zip(outs, full):
            got = o.cpu().numpy()
            assert got.shape == ref[..., :ng].shape
            assert np.array_equal(got.view(np.int64), np.ascontiguousarray(ref[..., :ng]).view(np.int64)), (case, ng)
        for flat, size in flats:
            assert_guard(flat, size, f"{case} ng={ng}")
    if case.startswith(("spin", "mggaspin")):        # the cut point and the empty point give exactly zero
        assert all(not o[..., [0, 200]].any() for o in full)


def _xc_raw_calls(ng, out):
    """name -> the raw entry point called on `ng` points with every output pointing into `out`."""
    import ctypes
    from mi355scf.engine import lib
    p = _xc_points()
    L, w = lib(), p["w"].data_ptr()
    ra, rb, ta, tb = (x.data_ptr() for x in p["rho"] + p["tau"])
    kinds = (ctypes.c_int32 * 4)(*[k for _c, k in B3LYP_TERMS])
    coefs = (ctypes.c_double * 4)(*[c for c, _k in B3LYP_TERMS])
    mk = (ctypes.c_int32 * 2)(*[k for _c, k in TPSS_TERMS])
    mc = (ctypes.c_double * 2)(*[c for c, _k in TPSS_TERMS])
    o = [out.data_ptr() + 8 * 8 * max(ng, 1) * i for i in range(4)]
    return {
        "mi_xc_eval": lambda: L.mi_xc_eval(kinds, coefs, 4, ra, w, ng, 1, o[0], o[1], o[2], o[3], None),
        "mi_xc_eval_p": lambda: L.mi_xc_eval_p(kinds, coefs, None, 4, ra, w, ng, 1, o[0], o[1], o[2], o[3], None),
        "mi_xc_eval_spin": lambda: L.mi_xc_eval_spin(kinds, coefs, 4, ra, rb, w, ng, 1, o[0], o[1], o[2], None),
        "mi_xc_eval_spin_p": lambda: L.mi_xc_eval_spin_p(kinds, coefs, None, 4, ra, rb, w, ng, 1, o[0], o[1], o[2], None),
        "mi_xc_eval_mgga": lambda: L.mi_xc_eval_mgga(mk, mc, 2, ra, ta, w, ng, o[0], o[1], None),
        "mi_xc_eval_mgga_spin": lambda: L.mi_xc_eval_mgga_spin(mk, mc, 2, ra, rb, ta, tb, w, ng, o[0], o[1], o[2], None),
        "mi_xc_fxc_prep": lambda: L.mi_xc_fxc_prep(kinds, coefs, None, 4, ra, w, ng, 1, 0, o[0], None),
    }


def test_xc_entry_points_zero_and_negative_sizes():
    """ng == 0 returns 0 and launches nothing (a poisoned output buffer keeps its sentinel); ng == -1 is an error."""
    from mi355scf.engine import EngineError, _check
    from test_gpu_dense_kernels import assert_guard, guarded
    out = guarded(0)
    for name, call in _xc_raw_calls(0, out).items():
        assert call() == 0, name
    torch.cuda.synchronize()
    assert_guard(out, 0, "ng == 0")
    for name, call in _xc_raw_calls(-1, out).items():
        with pytest.raises(EngineError, match="negative"):
            _check(call())
    torch.cuda.synchronize()
    assert_guard(out, 0, "ng == -1")


def test_xc_entry_points_refuse_bad_functional_specs():
    """One validator for all: a short-range B88 term without its omega (always, where there is no `params`), a meta-GGA id
    where there is no tau, an unknown id, more than eight terms."""
    from mi355scf.engine import EngineError
    p = _xc_points()
    eng, w = p["eng"], p["w"]
    ra, rb = p["rho"]
    ta, tb = p["tau"]
    calls = {
        "xc_eval": lambda t: eng.xc_eval(t, ra, w, True),
        "xc_eval_spin": lambda t: eng.xc_eval_spin(t, ra, rb, w, True),
        "xc_fxc_prep": lambda t: eng.xc_fxc_prep(t, ra, w, True),
        "xc_eval_mgga": lambda t: eng.xc_eval_mgga(t, ra, ta, w),
        "xc_eval_mgga_spin": lambda t: eng.xc_eval_mgga_spin(t, ra, rb, ta, tb, w),
    }
    for name, call in calls.items():
        with pytest.raises(EngineError, match="omega"):
            call([(1.0, 12)])
        with pytest.raises(EngineError, match="unknown functional id"):
            call([(1.0, 13)])
        with pytest.raises(EngineError, match="at most 8"):
            call([(0.1, 1)] * 9)
        if "mgga" not in name:
            with pytest.raises(EngineError, match="meta-GGA"):
                call(TPSS_TERMS)
    assert len(calls["xc_eval_mgga"]([(0.1, 1)] * 8)) == 2      # eight terms are accepted
