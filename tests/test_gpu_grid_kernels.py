"""The DFT grid front end one kernel at a time -- `becke_weights_kernel`, `eval_ao_kernel<DERIV>`, `xc_rho_kernel`,
`xc_rho_mo_kernel`, `xc_rho_lowrank_kernel<IC,DERIV>`, `xc_fxc_apply_kernel`, `nystrom_factor_kernel` -- against the long-double
references of tests/grid_reference.py, at the edges where per-point kernels go wrong.

  * Every output lives in a flat buffer followed by guard words (`guarded` / `assert_guard` of test_gpu_dense_kernels).
  * Every case runs at ng = 1, 255, 256, 257 and 1025 on the same point list: the kernels are per point, so a shorter run must
    equal the prefix of the longest bit for bit.
  * Bounds come from the FP64 rounding of the same formula on the host (tests/test_grid_reference_host.py measures it on these
    very inputs and each docstring quotes it), never from what the kernels give.
  * Integer inputs make every sum exact: there the kernels must equal the reference bit for bit.
Each test prints its figures (pytest -rP shows them)."""
import numpy as np
import pytest
import torch

import grid_reference as gr
from test_gpu_dense_kernels import U, assert_guard, guarded, ints, record
from test_gpu_pcm_kernels import WATER, _mol, _synthetic, _synthetic_with_ghost

pytestmark = pytest.mark.gpu

FLOOR = 64 * 2.0 ** -1022                    # results that are subnormal in FP64 but normal in long double
NGS = gr.NG_EDGES + (gr.NG_FULL,)
_CACHE = {}


def _eng(key):
    """(mol, Engine), one per molecule: nao = 1 (He), 7 (H2O), 48 and 64 (the synthetic s..f molecules), 58 (water/cc-pVTZ)."""
    from mi355scf.engine import Engine
    make = {"he": lambda: _mol("He 0 0 0", "sto-3g"), "h2o": lambda: _mol(WATER, "sto-3g"), "synthetic3": _synthetic,
            "synthetic": _synthetic_with_ghost, "water": lambda: _mol(WATER, "cc-pvtz"),
            "h2": lambda: _mol("H 0 0 -0.7; H 0 0 0.7", "sto-3g", unit="Bohr")}
    if key not in _CACHE:
        mol = make[key]()
        _CACHE[key] = (mol, Engine(mol))
    return _CACHE[key]


NAO_ENGINES = {1: "he", 7: "h2o", 48: "synthetic3", 64: "synthetic"}


def _dev(x):
    return torch.as_tensor(np.ascontiguousarray(x), device="cuda")


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.int64)


def _same_bits(a, b):
    return np.array_equal(_bits(a), _bits(b))


class _GuardedNew:
    """Stands in for Engine._new: every buffer the wrapper allocates is a guarded one."""

    def __init__(self):
        self.flats = []

    def __call__(self, *shape):
        size = int(np.prod(shape))
        self.flats.append((guarded(size), size))
        return self.flats[-1][0][:size].view(*shape)

    def check(self, what):
        torch.cuda.synchronize()
        assert self.flats
        for flat, size in self.flats:
            assert_guard(flat, size, what)
        del self.flats[:]


@pytest.fixture
def gnew(monkeypatch):
    """A `_GuardedNew`; `gnew.attach(eng)` puts it in place of `eng._new` for the length of the test."""
    g = _GuardedNew()
    g.attach = lambda eng: monkeypatch.setattr(eng, "_new", g)
    return g


# ------------------------------------------------------------------------------------------------------------------------------
# eval_ao_kernel<0 | 1 | 2>
# ------------------------------------------------------------------------------------------------------------------------------
def _ao_ref(name):
    """(pts, ref, majorant) of the ten components, once per molecule; the lower orders are its leading components."""
    if ("aoref", name) not in _CACHE:
        mol, _ = _eng(name)
        pts = gr.ao_points(mol)
        _CACHE["aoref", name] = (pts,) + gr.ao_reference(mol, pts, 2)
    return _CACHE["aoref", name]


def _run_ao(eng, pts, deriv):
    ng, nc = len(pts), gr.NCOMP[deriv]
    size = nc * eng.nao * ng
    flat = guarded(size)
    eng.eval_ao(_dev(pts), deriv=deriv, out=flat[:size].view(nc, eng.nao, ng))
    torch.cuda.synchronize()
    assert_guard(flat, size, f"eval_ao deriv={deriv} ng={ng}")
    return flat[:size].view(nc, eng.nao, ng).cpu().numpy()


@pytest.mark.parametrize("deriv", [0, 1, 2])
@pytest.mark.parametrize("name", ["synthetic", "water"])
def test_eval_ao_within_rounding_of_long_double_every_class(name, deriv):
    """`mi_eval_ao` on the synthetic s..f molecule with a ghost (every l on every centre) and on water/cc-pVTZ (contractions of
    up to ten primitives with mixed signs) at 1025 points: normal ones (sigma 2.5 Bohr), one on every centre, one 1e-9 Bohr off a
    centre, one far down every AO's tail and one where every primitive underflows (exactly 0.0 there, in every component).
    Bound per element: |got - ref| <= 16 u majorant + 64 * 2^-1022.  Yardstick: the FP64 NumPy oracle is within 3.60 u majorant
    on the synthetic molecule and 3.89 on water on these points (test_grid_reference_host); 16 is four times the 3.6.
    The runs at ng = 1, 255, 256, 257 equal the prefix of the 1025-point run bit for bit.
    Observed on the MI355X: worst err / bound 0.224 (synthetic, every order) and 0.212 (water, every order)."""
    mol, eng = _eng(name)
    pts, ref, maj = _ao_ref(name)
    nc = gr.NCOMP[deriv]
    full = _run_ao(eng, pts, deriv)
    got = full.transpose(0, 2, 1)                                                   # [nc][ng][nao]
    assert np.isfinite(got).all()
    assert not got[:, gr.AO_FAR, :].any()                                           # every primitive has underflowed: exactly zero
    err = np.abs((got - ref[:nc]).astype(np.float64))
    ratio = err / (16.0 * U * maj[:nc].astype(np.float64) + FLOOR)
    loc = mol.ao_loc_nr()
    lof = np.concatenate([np.full(loc[i + 1] - loc[i], int(mol._bas[i, 1])) for i in range(mol.nbas)])
    for l in sorted(set(lof.tolist())):
        worst = ratio[:, :, lof == l].max(axis=(1, 2))
        print(f"[rounding] eval_ao {name} deriv={deriv} l={l}: worst err / bound per component = {np.round(worst, 3).tolist()}")
    record(f"eval_ao {name} deriv={deriv}", float(ratio.max()))
    for ng in gr.NG_EDGES:
        assert _same_bits(_run_ao(eng, pts[:ng], deriv), full[:, :, :ng]), (name, deriv, ng)


@pytest.mark.parametrize("name", ["synthetic", "water"])
def test_eval_ao_value_is_the_same_at_every_derivative_order(name):
    """The deriv = 0 output equals component 0 of deriv = 1 and of deriv = 2 bit for bit, and the gradient of deriv = 1 equals
    components 1..3 of deriv = 2."""
    _, eng = _eng(name)
    pts = _ao_ref(name)[0]
    a0, a1, a2 = (_run_ao(eng, pts, d) for d in (0, 1, 2))
    assert _same_bits(a0[0], a1[0]) and _same_bits(a0[0], a2[0]) and _same_bits(a1, a2[:4])


# ------------------------------------------------------------------------------------------------------------------------------
# becke_weights_kernel
# ------------------------------------------------------------------------------------------------------------------------------
def _run_becke(eng, coords, atom_of, vol, a):
    from mi355scf.engine import _check, lib
    ng = len(vol)
    c, o, v, ad = _dev(coords), _dev(atom_of.astype(np.int32)), _dev(vol), _dev(a)
    flat = guarded(ng)
    _check(lib().mi_grid_becke(eng._h, c.data_ptr(), o.data_ptr(), v.data_ptr(), ng, ad.data_ptr(), flat.data_ptr(), eng._stream()))
    torch.cuda.synchronize()
    assert_guard(flat, ng, f"becke ng={ng}")
    return flat[:ng].cpu().numpy()


def _becke_edges(eng, coords, atom_of, vol, a):
    """The full run (through Engine.becke_weights and through the raw entry point into a guarded buffer: same bits) and the
    prefix property at the workgroup edges."""
    full = _run_becke(eng, coords, atom_of, vol, a)
    w = eng.becke_weights(_dev(coords), _dev(atom_of.astype(np.int32)), _dev(vol), _dev(a)).cpu().numpy()
    assert _same_bits(w, full)
    for ng in gr.NG_EDGES:
        assert _same_bits(_run_becke(eng, coords[:ng], atom_of[:ng], vol[:ng], a), full[:ng]), ng
    return full


def test_becke_single_atom_returns_the_volume_element():
    """natm = 1: the empty product is 1, so w == vol bit for bit -- on the nucleus, near it and 40 Bohr away."""
    _, eng = _eng("he")
    rng = np.random.default_rng(1)
    coords = 3.0 * rng.standard_normal((gr.NG_FULL, 3))
    coords[0] = 0.0
    coords[1] = (1e-9, 0.0, 0.0)
    coords[2] = (24.0, -24.0, 22.0)
    vol = np.exp(rng.uniform(-6.0, 3.0, gr.NG_FULL))
    w = _becke_edges(eng, coords, np.zeros(gr.NG_FULL, dtype=np.int32), vol, np.zeros((1, 1)))
    assert _same_bits(w, vol)


def test_becke_homonuclear_pair_mirrored_points_share_the_volume():
    """natm = 2, a = 0: the mirror image p' of p in the bisecting plane swaps the two cells, so with both booked to atom 0
    w(p) + w(p') = vol.  In FP64 the two distances swap exactly and mu changes sign exactly, so the two cell functions are the same
    two numbers s0, s1 and their sum is the same fl(s0 + s1): each weight is vol s / fl(s0 + s1) within 2 u (product, quotient),
    the sum of the exact quotients is vol within u, the final addition adds u: |w + w' - vol| <= 4 u vol.  Each weight is also
    within the general bound 2e-14 vol of the long-double reference.
    Observed on the MI355X: worst |w + w' - vol| / (4 u vol) = 0.492, worst |w - ref| / (2e-14 vol) = 0.11."""
    mol, eng = _eng("h2")
    R = mol.atom_coords()
    assert np.array_equal(R, [[0, 0, -0.7], [0, 0, 0.7]])
    rng = np.random.default_rng(2)
    half = (gr.NG_FULL + 1) // 2
    p = np.exp(rng.uniform(np.log(0.05), np.log(6.0), (half, 1))) * rng.standard_normal((half, 3))
    p[0] = (0.0, 0.0, -0.7)                                                   # on atom 0; its image is on atom 1
    p[1] = (0.4, -0.3, 0.0)                                                   # on the bisecting plane: its own image
    coords = np.empty((2 * half, 3))
    coords[0::2], coords[1::2] = p, p * [1, 1, -1]                            # image pairs sit side by side in every prefix
    assert len(coords) == gr.NG_FULL + 1
    vol = np.repeat(np.exp(rng.uniform(-6.0, 3.0, half)), 2)
    own = np.zeros(len(vol), dtype=np.int32)
    a = np.zeros((2, 2))
    ref, _ = gr.becke_reference(coords, own, vol, R, a)
    w = _run_becke(eng, coords, own, vol, a)
    for ng in NGS:
        assert _same_bits(_run_becke(eng, coords[:ng], own[:ng], vol[:ng], a), w[:ng]), ng
    assert w[0] == vol[0] and w[1] == 0.0 and w[2] == 0.5 * vol[2] and w[3] == 0.5 * vol[3]
    record("becke H2 mirror sum", float(np.max(np.abs(w[0::2] + w[1::2] - vol[0::2]) / (4 * U * vol[0::2]))))
    record("becke H2 vs long double", float(np.max(np.abs((w - ref).astype(np.float64)) / (2e-14 * vol))))


def _lattice_engine(natm):
    """natm hydrogen atoms (STO-3G) on `gr.becke_lattice`: only the centres matter to the Becke kernel."""
    from mi355scf.engine import Engine
    if ("lattice", natm) not in _CACHE:
        R = gr.becke_lattice(natm)
        mol = _mol("; ".join(f"H {x!r} {y!r} {z!r}" for x, y, z in R.tolist()), "sto-3g", unit="Bohr", spin=natm % 2)
        assert np.array_equal(mol.atom_coords(), R)
        _CACHE["lattice", natm] = Engine(mol)
    return _CACHE["lattice", natm]


@pytest.mark.parametrize("natm", [85, 86, 100])
def test_becke_many_atoms_within_rounding_of_long_double(natm):
    """natm = 85 (the last size whose 3 natm coordinates one trip of the 256-thread cooperative load covers), 86 (the first
    that needs a second trip) and 100, on a jittered 5 x 5 x 4 lattice whose first three atoms are exactly collinear, with
    adjustments a_ij from mixed radii, one pair put at the clip +-0.5, and `atom_of` not the nearest atom.  Points: log-uniform
    0.05..6 Bohr from random parents, one on its parent nucleus (w == vol exactly), one on another nucleus and one on the
    collinear axis beyond the end atom (w == 0 exactly), one on a bisecting plane, one 48 Bohr out.
    Bound: |w - ref| <= 2e-14 vol.  Yardstick: the FP64 NumPy evaluation of the same formula is within 1.31e-15, 1.35e-15 and
    1.41e-15 vol of the reference on these inputs, whose smallest sum_i P_i is 1.1e-2 (test_grid_reference_host).  Wherever the
    reference is exactly vol or exactly 0 the kernel must be too.
    Observed on the MI355X: worst err / bound 0.0655, 0.0677, 0.049; 45, 48 and 31 weights exactly zero, one exactly vol."""
    eng = _lattice_engine(natm)
    coords, atom_of, vol, R, a = gr.becke_case(natm)
    ref, psum = gr.becke_reference(coords, atom_of, vol, R, a)
    assert float(psum.min()) > 1e-6
    w = _becke_edges(eng, coords, atom_of, vol, a)
    assert np.isfinite(w).all()
    record(f"becke natm={natm}", float(np.max(np.abs((w - ref).astype(np.float64)) / (2e-14 * vol))))
    is_vol, is_zero = np.asarray(ref == vol), np.asarray(ref == 0)
    assert is_vol[gr.BECKE_ON_PARENT] and is_zero[gr.BECKE_ON_OTHER] and is_zero[gr.BECKE_AXIS]
    assert _same_bits(w[is_vol], vol[is_vol]) and _same_bits(w[is_zero], np.zeros(int(is_zero.sum())))
    print(f"[exact] becke natm={natm}: {int(is_vol.sum())} weights exactly vol, {int(is_zero.sum())} exactly zero")


# ------------------------------------------------------------------------------------------------------------------------------
# xc_rho_kernel, xc_rho_mo_kernel, xc_rho_lowrank_kernel
# ------------------------------------------------------------------------------------------------------------------------------
def _f64(x):
    return None if x is None else np.asarray(x).astype(np.float64)


def _real(rng, shape):
    """Entries of both signs with a dynamic range of e^+-4."""
    return rng.standard_normal(shape) * np.exp(rng.uniform(-4.0, 4.0, shape))


def _rho_c(eng, gnew, ao, C, deriv, ng):
    nc = 4 if deriv else 1
    out = eng.xc_rho(_dev(ao[:nc, :, :ng]), _dev(C[:, :ng]), deriv=deriv, out=gnew(nc, ng))
    gnew.check(f"xc_rho nao={eng.nao} ng={ng}")
    return out.cpu().numpy()


@pytest.mark.parametrize("nao", [1, 7, 48, 64])
def test_xc_rho_exact_on_integers(nao, gnew):
    """`mi_xc_rho`, deriv 0 and 1: integer AO values and C make every sum exact, so rho and grad rho (with its factor 2) equal
    the reference bit for bit at every ng; the shorter runs are the prefix of the longest."""
    _, eng = _eng(NAO_ENGINES[nao])
    assert eng.nao == nao
    rng = np.random.default_rng(100 + nao)
    ao, C = ints(rng, (4, nao, gr.NG_FULL)), ints(rng, (nao, gr.NG_FULL))
    ref = _f64(gr.rho_c_reference(ao, C)[0])
    for deriv in (0, 1):
        for ng in NGS:
            assert _same_bits(_rho_c(eng, gnew, ao, C, deriv, ng), ref[:4 if deriv else 1, :ng]), (deriv, ng)


@pytest.mark.parametrize("nao", [7, 64])
def test_xc_rho_real_within_rounding_bound(nao, gnew):
    """Real entries over e^+-4: |rho - ref| <= u (nao + 2) majorant, majorant = sum_m |ao_m| |C_m| (times 2 for the gradient):
    nao fused multiply-adds, the rounding of the reference to FP64 and one to spare; the factor 2 is exact.
    Observed on the MI355X: worst err / bound 0.38 (nao 7), 0.133 (nao 64)."""
    _, eng = _eng(NAO_ENGINES[nao])
    rng = np.random.default_rng(200 + nao)
    ao, C = _real(rng, (4, nao, gr.NG_FULL)), _real(rng, (nao, gr.NG_FULL))
    ref, maj = gr.rho_c_reference(ao, C)
    got = _rho_c(eng, gnew, ao, C, 1, gr.NG_FULL)
    record(f"xc_rho nao={nao}", float(np.max(np.abs(_f64(got - ref)) / (U * (nao + 2) * _f64(maj)))))
    assert _same_bits(_rho_c(eng, gnew, ao, C, 0, 257)[0], got[0, :257])


def _rho_mo(eng, gnew, psi, deriv, tau, ng):
    nc = 4 if deriv else 1
    out = eng.xc_rho_mo(_dev(psi[:nc, :, :ng]), deriv=deriv, with_tau=tau)
    gnew.check(f"xc_rho_mo nocc={psi.shape[1]} ng={ng}")
    rho, t = out if tau else (out, None)
    return rho.cpu().numpy(), None if t is None else t.cpu().numpy()


@pytest.mark.parametrize("nocc", [1, 5, 24, 25, 64])
def test_xc_rho_mo_exact_on_integers(nocc, gnew):
    """`mi_xc_rho_mo` at deriv 0, deriv 1 and deriv 1 with tau: integer orbital values, every sum exact, tau's factor 1/2
    included; bit for bit at every ng."""
    _, eng = _eng("h2o")
    gnew.attach(eng)
    rng = np.random.default_rng(300 + nocc)
    psi = ints(rng, (4, nocc, gr.NG_FULL))
    val, _ = gr.rho_mo_reference(psi)
    rho_ref, tau_ref = _f64(val["rho"]), _f64(val["tau"])
    for deriv, tau in ((0, False), (1, False), (1, True)):
        for ng in NGS:
            rho, t = _rho_mo(eng, gnew, psi, deriv, tau, ng)
            assert _same_bits(rho, rho_ref[:4 if deriv else 1, :ng]), (deriv, tau, ng)
            assert t is None or _same_bits(t, tau_ref[:ng])


def test_xc_rho_mo_real_within_rounding_bound(gnew):
    """Real entries over e^+-4, nocc = 25: rho and grad rho within u (nocc + 2) majorant, tau (three multiply-adds per
    orbital) within u (3 nocc + 2) majorant.
    Observed on the MI355X: worst err / bound 0.209 (rho, grad rho), 0.113 (tau)."""
    _, eng = _eng("h2o")
    gnew.attach(eng)
    nocc = 25
    psi = _real(np.random.default_rng(41), (4, nocc, gr.NG_FULL))
    val, maj = gr.rho_mo_reference(psi)
    rho, tau = _rho_mo(eng, gnew, psi, 1, True, gr.NG_FULL)
    record("xc_rho_mo rho", float(np.max(np.abs(_f64(rho - val["rho"])) / (U * (nocc + 2) * _f64(maj["rho"])))))
    record("xc_rho_mo tau", float(np.max(np.abs(_f64(tau - val["tau"])) / (U * (3 * nocc + 2) * _f64(maj["tau"])))))


def _lowrank(eng, gnew, ao, Zp, deriv, tau, ng):
    nc = 4 if deriv else 1
    out = eng.xc_rho_lowrank(_dev(ao[:nc, :, :ng]), _dev(Zp), deriv=deriv, with_tau=tau)
    gnew.check(f"xc_rho_lowrank nao={eng.nao} ldz={Zp.shape[1]} ng={ng}")
    rho, t = out if tau else (out, None)
    return rho.cpu().numpy(), None if t is None else t.cpu().numpy()


@pytest.mark.parametrize("nao", [1, 7, 48, 64])
def test_xc_rho_lowrank_exact_on_integers(nao, gnew):
    """`mi_xc_rho_lowrank`: ldz 24, 48, 72 with derivatives (tau given and null) and 32, 64, 96 without, rank == ldz and
    rank < ldz with zero padding, at every ng (ng = 1 and 257 run the clamp of the idle lanes).  Integers: psi <= 64 * 64,
    rho <= 96 * 2^24, all exact, so the kernel equals the two-level reference bit for bit."""
    _, eng = _eng(NAO_ENGINES[nao])
    gnew.attach(eng)
    rng = np.random.default_rng(400 + nao)
    ao = ints(rng, (4, nao, gr.NG_FULL))
    for deriv, ldzs in ((1, (24, 48, 72)), (0, (32, 64, 96))):
        for ldz in ldzs:
            for rank in (ldz, ldz - 5):
                Zp = np.zeros((nao, ldz))
                Zp[:, :rank] = ints(rng, (nao, rank))
                val, _ = gr.rho_reference(ao, Zp[:, :rank])
                rho_ref, tau_ref = _f64(val["rho"]), _f64(val["tau"])
                for tau in ((True, False) if deriv else (False,)):
                    for ng in NGS:
                        rho, t = _lowrank(eng, gnew, ao, Zp, deriv, tau, ng)
                        assert _same_bits(rho, rho_ref[:4 if deriv else 1, :ng]), (deriv, ldz, rank, tau, ng)
                        assert t is None or _same_bits(t, tau_ref[:ng]), (ldz, rank, ng)


@pytest.mark.parametrize("nao,ldz", [(7, 24), (64, 72)])
def test_xc_rho_lowrank_real_within_rounding_bound(nao, ldz, gnew):
    """Real entries over e^+-4.  The kernel forms psi_i = sum_m z_mi ao_m (nao multiply-adds) and then rho = sum_i psi_i^2
    (ldz multiply-adds).  With A_i = sum_m |z_mi| |ao_m|: the computed psi_i is off by e_i, |e_i| <= nao u A_i; the sum of the
    computed squares is off from the exact one by sum_i (2 |psi_i| |e_i| + e_i^2) <= 2 nao u sum_i A_i^2, and its own rounding
    adds ldz u sum_i A_i^2.  So |rho - ref| <= u (2 nao + ldz + 2) majorant with majorant = sum_i A_i^2 (`rho_reference`), the
    + 2 for the rounding of the reference and the second-order terms; the same count holds for grad rho = 2 sum_i psi_i
    grad psi_i with majorant 2 sum_i A_i A'_i, and tau takes three multiply-adds per orbital: u (2 nao + 3 ldz + 2) majorant.
    Observed on the MI355X: worst err / bound 0.117 and 0.0161 (rho, grad rho), 0.103 and 0.0141 (tau), 0.0974 and 0.0144
    (rho without derivatives)."""
    _, eng = _eng(NAO_ENGINES[nao])
    gnew.attach(eng)
    rng = np.random.default_rng(500 + nao)
    ao = _real(rng, (4, nao, gr.NG_FULL))
    rank = ldz - 3
    Zp = np.zeros((nao, ldz))
    Zp[:, :rank] = _real(rng, (nao, rank))
    val, maj = gr.rho_reference(ao, Zp[:, :rank])
    rho, tau = _lowrank(eng, gnew, ao, Zp, 1, True, gr.NG_FULL)

    def worst(got, ref, n, majorant):
        return float(np.max(np.abs(_f64(got - ref)) / (U * (n + 2) * _f64(majorant))))
    record(f"xc_rho_lowrank rho nao={nao}", worst(rho, val["rho"], 2 * nao + ldz, maj["rho"]))
    record(f"xc_rho_lowrank tau nao={nao}", worst(tau, val["tau"], 2 * nao + 3 * ldz, maj["tau"]))
    ld0 = 32 * ((rank + 31) // 32)
    Z0 = np.zeros((nao, ld0))
    Z0[:, :rank] = Zp[:, :rank]
    rho0, _ = _lowrank(eng, gnew, ao, Z0, 0, False, gr.NG_FULL)
    record(f"xc_rho_lowrank rho deriv=0 nao={nao}", worst(rho0[0], val["rho"][0], 2 * nao + ld0, maj["rho"][0]))


def test_density_entry_points_refuse_bad_shapes():
    """ldz not a multiple of 24 with derivatives or of 32 without, tau with deriv 0, ng < 1 for `mi_xc_rho_lowrank` and
    `mi_xc_tail`, nocc < 1 for `mi_xc_rho_mo`: errors, and the guarded output keeps its sentinel."""
    from mi355scf.engine import EngineError, _check, lib
    _, eng = _eng("h2o")
    L, h, st = lib(), eng._h, eng._stream()
    out = guarded(0)
    o = out.data_ptr()
    ao = torch.zeros(4 * 7 * 8, dtype=torch.float64, device="cuda")
    z = torch.zeros(7 * 96, dtype=torch.float64, device="cuda")
    a, zp = ao.data_ptr(), z.data_ptr()
    cases = {
        "ldz 32 with derivatives": (lambda: L.mi_xc_rho_lowrank(h, a, zp, 32, 8, 1, o, None, st), "multiple of 24"),
        "ldz 40 with derivatives": (lambda: L.mi_xc_rho_lowrank(h, a, zp, 40, 8, 1, o, None, st), "multiple of 24"),
        "ldz 24 without": (lambda: L.mi_xc_rho_lowrank(h, a, zp, 24, 8, 0, o, None, st), "multiple of 32"),
        "ldz 0": (lambda: L.mi_xc_rho_lowrank(h, a, zp, 0, 8, 1, o, None, st), "bad argument"),
        "lowrank tau with deriv 0": (lambda: L.mi_xc_rho_lowrank(h, a, zp, 32, 8, 0, o, o + 64, st), "bad argument"),
        "lowrank ng 0": (lambda: L.mi_xc_rho_lowrank(h, a, zp, 24, 0, 1, o, None, st), "bad argument"),
        "lowrank ng -1": (lambda: L.mi_xc_rho_lowrank(h, a, zp, 24, -1, 1, o, None, st), "bad argument"),
        "tail ng 0": (lambda: L.mi_xc_tail(h, a, a, None, None, 0, o, st), "bad argument"),
        "rho_mo nocc 0": (lambda: L.mi_xc_rho_mo(h, a, 0, 8, 1, o, None, st), "bad argument"),
        "rho_mo nocc -1": (lambda: L.mi_xc_rho_mo(h, a, -1, 8, 1, o, None, st), "bad argument"),
        "rho_mo tau with deriv 0": (lambda: L.mi_xc_rho_mo(h, a, 5, 8, 0, o, o + 64, st), "bad argument"),
    }
    for name, (call, text) in cases.items():
        with pytest.raises(EngineError, match=text):
            _check(call())
    torch.cuda.synchronize()
    assert_guard(out, 0, "refusals")


# ------------------------------------------------------------------------------------------------------------------------------
# xc_fxc_apply_kernel
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gga", [False, True])
@pytest.mark.parametrize("m", [1, 3])
def test_xc_fxc_apply_exact_on_integers(m, gga, gnew):
    """Integer rho0 and rho1 and even integer coefficients (so the 1/2 is exact): bit for bit
        LDA: wv = c0 rho1 / 2
        GGA: s1 = 2 grad rho0 . grad rho1;  wv_0 = (c0 rho1 + c1 s1) / 2;  wv_k = 2 (c1 rho1 + c2 s1) d_k rho0 + 2 c3 d_k rho1
    for every trial density, at every ng."""
    _, eng = _eng("h2o")
    gnew.attach(eng)
    nc = 4 if gga else 1
    rng = np.random.default_rng(600 + 10 * m + gga)
    N = gr.NG_FULL
    rho0, coef, rho1 = ints(rng, (4, N)), 2.0 * ints(rng, (nc, N), -4, 4), ints(rng, (m, nc, N))
    if gga:
        r, g1 = rho1[:, 0], rho1[:, 1:]
        s1 = 2.0 * (rho0[None, 1:] * g1).sum(axis=1)
        t = 2.0 * (coef[1] * r + coef[2] * s1)
        ref = np.concatenate([(0.5 * (coef[0] * r + coef[1] * s1))[:, None],
                              t[:, None] * rho0[None, 1:] + 2.0 * coef[3] * g1], axis=1)
    else:
        ref = 0.5 * coef[0] * rho1
    assert ref.shape == (m, nc, N) and np.abs(ref).max() < 2.0 ** 40 and np.any(ref[:, 0] % 2 != 0)
    for ng in NGS:
        got = eng.xc_fxc_apply(_dev(rho0[:, :ng]), _dev(coef[:, :ng]), _dev(rho1[:, :, :ng]), gga=gga)
        gnew.check(f"xc_fxc_apply m={m} gga={gga} ng={ng}")
        assert _same_bits(got.cpu().numpy(), ref[:, :, :ng]), (m, gga, ng)


def test_xc_fxc_apply_zero_and_negative_sizes():
    """m == 0 and ng == 0 return 0 and leave a poisoned buffer untouched; negative sizes are refused."""
    from mi355scf.engine import EngineError, _check, lib
    L = lib()
    x = torch.ones(4 * 8 * 3, dtype=torch.float64, device="cuda").data_ptr()
    out = guarded(0)
    for m, ng in ((0, 8), (3, 0), (0, 0)):
        for gga in (0, 1):
            assert L.mi_xc_fxc_apply(x, x, x, m, ng, gga, out.data_ptr(), None) == 0
    for m, ng in ((-1, 8), (3, -1)):
        with pytest.raises(EngineError, match="negative"):
            _check(L.mi_xc_fxc_apply(x, x, x, m, ng, 1, out.data_ptr(), None))
    torch.cuda.synchronize()
    assert_guard(out, 0, "xc_fxc_apply sizes")


# ------------------------------------------------------------------------------------------------------------------------------
# nystrom_factor_kernel
# ------------------------------------------------------------------------------------------------------------------------------
def _run_nystrom(eng, M, W):
    n, nocc = W.shape
    flat = guarded(nocc * n)
    info = torch.full((), -7, dtype=torch.int32, device="cuda")
    eng.nystrom_factor(_dev(M), _dev(W), Zt=flat[:nocc * n].view(nocc, n), info=info)
    torch.cuda.synchronize()
    assert_guard(flat, nocc * n, f"nystrom_factor nocc={nocc} n={n}")
    return flat[:nocc * n].view(nocc, n).cpu().numpy(), int(info)


@pytest.mark.parametrize("nocc", [1, 2, 63, 64])
def test_nystrom_factor_matches_long_double_cholesky_solve(nocc):
    """`mi_nystrom_factor` at n = 1, 63, 64, 65 (each workgroup solves 64 columns) against a long-double Cholesky factorisation
    and forward substitution, at the bound of the existing test, 1e-11 (1 + max |ref|).  A failing first pivot, a failing last
    pivot and a NaN in M: info holds the LAPACK index of the reference and Zt is all NaN.
    Observed on the MI355X: worst err / bound 8.2e-6, 9.6e-6, 7.4e-5, 8.5e-5 (nocc = 1, 2, 63, 64)."""
    _, eng = _eng("h2o")
    rng = np.random.default_rng(700 + nocc)
    B = rng.standard_normal((nocc + 16, nocc))
    M = B.T @ B / (nocc + 16) + 0.25 * np.eye(nocc)
    worst = 0.0
    for n in (1, 63, 64, 65):
        W = rng.standard_normal((n, nocc))
        ref, info_ref = gr.cholesky_solve_reference(M, W)
        Zt, info = _run_nystrom(eng, M, W)
        assert info == 0 == info_ref
        worst = max(worst, float(np.max(np.abs(_f64(Zt - ref))) / (1e-11 * (1.0 + float(np.abs(ref).max())))))
    record(f"nystrom_factor nocc={nocc}", worst)
    bad = []
    for k, v in ((0, -1.0), (nocc - 1, -1e3), (nocc // 2, np.nan)):
        Mb = M.copy()
        Mb[k, k] = v
        bad.append(Mb)
    if nocc > 1:
        Mb = M.copy()
        Mb[nocc - 1, 0] = np.nan                                  # in the lower triangle: reaches the last pivot
        bad.append(Mb)
    for Mb in bad:
        _, info_ref = gr.cholesky_solve_reference(Mb, W)
        Zt, info = _run_nystrom(eng, Mb, W)
        assert info_ref > 0 and info == info_ref and np.isnan(Zt).all()


# ------------------------------------------------------------------------------------------------------------------------------
# Size conventions of the entry points
# ------------------------------------------------------------------------------------------------------------------------------
def _raw_grid_calls(eng, ng, out):
    """name -> the raw entry point called on `ng` points with its output pointing at `out`."""
    from mi355scf.engine import lib
    L, h, st, o = lib(), eng._h, eng._stream(), out.data_ptr()
    x = torch.zeros(4 * 8 * eng.nao, dtype=torch.float64, device="cuda")
    own = torch.zeros(8, dtype=torch.int32, device="cuda")
    _CACHE["raw keep"] = (x, own)
    p, q = x.data_ptr(), own.data_ptr()
    return {
        "mi_grid_becke": lambda: L.mi_grid_becke(h, p, q, p, ng, p, o, st),
        "mi_eval_ao 0": lambda: L.mi_eval_ao(h, p, ng, 0, o, st),
        "mi_eval_ao 2": lambda: L.mi_eval_ao(h, p, ng, 2, o, st),
        "mi_xc_rho": lambda: L.mi_xc_rho(h, p, p, ng, 1, o, st),
        "mi_xc_rho_mo": lambda: L.mi_xc_rho_mo(h, p, 5, ng, 1, o, o, st),
    }


def test_grid_entry_points_zero_and_negative_sizes():
    """The convention of `mi_xc_aow` for `mi_grid_becke`, `mi_eval_ao`, `mi_xc_rho` and `mi_xc_rho_mo`: ng == 0 returns 0 and
    launches nothing (a poisoned output keeps its sentinel), ng == -1 is an error that says "negative"; `mi_eval_ao` refuses a
    derivative order outside 0..2."""
    from mi355scf.engine import EngineError, _check, lib
    _, eng = _eng("h2o")
    out = guarded(0)
    for name, call in _raw_grid_calls(eng, 0, out).items():
        assert call() == 0, name
    torch.cuda.synchronize()
    assert_guard(out, 0, "ng == 0")
    for name, call in _raw_grid_calls(eng, -1, out).items():
        with pytest.raises(EngineError, match="negative"):
            _check(call())
    x = _CACHE["raw keep"][0].data_ptr()
    for deriv in (-1, 3):
        with pytest.raises(EngineError, match="deriv"):
            _check(lib().mi_eval_ao(eng._h, x, 8, deriv, out.data_ptr(), eng._stream()))
    for name, call in {"becke": lambda: lib().mi_grid_becke(None, x, x, x, 8, x, out.data_ptr(), None),
                       "eval_ao": lambda: lib().mi_eval_ao(None, x, 8, 1, out.data_ptr(), None),
                       "xc_rho": lambda: lib().mi_xc_rho(None, x, x, 8, 1, out.data_ptr(), None),
                       "xc_rho_mo": lambda: lib().mi_xc_rho_mo(None, x, 5, 8, 1, out.data_ptr(), None, None)}.items():
        with pytest.raises(EngineError, match="null context"):
            _check(call())
    torch.cuda.synchronize()
    assert_guard(out, 0, "refused sizes")
