"""GPU parity: HIP kernels (through the C ABI) vs the CPU oracle on the same inputs.
Tolerances: FP64 path; integrals and J/K agree to 1e-10 absolute (values are O(1)-O(10)); the
north_star's energy tolerance is 1e-6 Ha (tests/test_gpu_scf.py)."""
import numpy as np
import pytest

from conftest import MOLECULES

pytestmark = pytest.mark.gpu

CASES = [("h2o", "sto-3g"), ("h2o", "6-31g*"), ("h2co", "6-31g(d)"), ("h2o", "cc-pvdz"), ("ch4", "cc-pvdz"),
         ("h2o", "cc-pvtz")]


def _mol(name, basis):
    from mi355scf.mole import Mole
    return Mole(atom=MOLECULES[name], basis=basis).build()


def _sym_density(n, seed):
    rng = np.random.default_rng(seed)
    a = rng.normal(size=(n, n))
    return (a + a.T) * 0.5


@pytest.mark.parametrize("name,basis", CASES)
def test_int1e_matches_oracle(name, basis):
    from mi355scf.engine import Engine
    from oracle import oracle as orc
    mol = _mol(name, basis)
    eng = Engine(mol)
    S, T, V, dip = (x.cpu().numpy() for x in eng.int1e(with_dipole=True, origin=[0.1, -0.2, 0.3]))
    So, To, Vo, dipo = orc.Oracle(mol).int1e(origin=[0.1, -0.2, 0.3])
    assert np.abs(S - So).max() < 1e-12
    assert np.abs(T - To).max() < 1e-11
    assert np.abs(V - Vo).max() < 1e-10
    assert np.abs(dip - dipo).max() < 1e-11


def test_int1e_matches_oracle_every_class():
    """int1e_kernel<LA,LB> at each of its 10 angular classes on the synthetic s..f molecule with a ghost centre (16 shells, one
    of every l per centre): S, T, V and the dipole per shell-pair block against the oracle with test_int1e_matches_oracle's
    bounds.  Every class occurs on one centre and across two, with the higher l on the higher and on the lower shell index (the
    kernel always takes the higher l first, so the second case stores the transposed block and raises the dipole on the other
    centre), and next to the ghost centre.  Calls with null outputs (V alone; S and T alone) give the full call's S and T
    exactly and its V within 1e-13 max|V| (FP64 atomics in no fixed order).

    Observed on the MI355X, worst block per class: S 1e-16 .. 7e-16, T 2e-16 .. 2e-15, V 3e-15 .. 3e-14 (max|V| 13.9),
    dipole 2e-16 .. 9e-16; V alone against the full call 1.8e-15."""
    import ctypes
    import torch
    from mi355scf.engine import Engine, lib
    from oracle import oracle as orc
    from test_gpu_pcm_kernels import _synthetic_with_ghost
    mol = _synthetic_with_ghost()
    origin = np.array([0.1, -0.2, 0.3])
    eng = Engine(mol)
    got = [x.cpu().numpy() for x in eng.int1e(with_dipole=True, origin=origin)]
    ref = orc.Oracle(mol).int1e(origin=origin)
    bounds = {"S": 1e-12, "T": 1e-11, "V": 1e-10, "dipole": 1e-11}
    l, at, loc = mol._bas[:, 1], mol._bas[:, 0], mol.ao_loc_nr()
    nb = mol._bas.shape[0]
    seen, worst, bad = {}, {}, []
    for i in range(nb):
        for j in range(nb):
            cls = (int(max(l[i], l[j])), int(min(l[i], l[j])))
            si, sj = slice(loc[i], loc[i + 1]), slice(loc[j], loc[j + 1])
            if i >= j:
                kinds = seen.setdefault(cls, set())
                kinds.add("one-centre" if at[i] == at[j] else "two-centre")
                kinds.add("higher l first" if l[i] > l[j] else "lower l first" if l[i] < l[j] else "equal l")
                if 3 in (at[i], at[j]):
                    kinds.add("ghost")
            for (name, tol), g, r in zip(bounds.items(), got, ref):
                err = np.abs(g[..., si, sj] - r[..., si, sj]).max()
                worst[cls, name] = max(worst.get((cls, name), 0.0), err)
                if not err < tol:
                    bad.append(f"{name} block ({i},{j}) class {cls} atoms ({at[i]},{at[j]}): |err| = {err:.2e} (bound {tol:.0e})")
    assert sorted(seen) == [(a, b) for a in range(4) for b in range(a + 1)]
    for cls, kinds in seen.items():
        want = {"one-centre", "two-centre", "ghost"} | ({"equal l"} if cls[0] == cls[1] else {"higher l first", "lower l first"})
        assert kinds == want, (cls, kinds)
    for cls in sorted(seen):
        print(f"int1e<{cls[0]},{cls[1]}>: " + ", ".join(f"{name} {worst[cls, name]:.1e}" for name in bounds))
    assert not bad, "blocks over their bound:\n" + "\n".join(bad)

    n = mol.nao
    vp, org = ctypes.c_void_p, origin.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    V2, S2, T2 = (torch.full((n, n), float("nan"), dtype=torch.float64, device=eng.device) for _ in range(3))
    with torch.cuda.device(eng.device):
        assert lib().mi_int1e(eng._h, None, None, vp(V2.data_ptr()), None, org, eng._stream()) == 0
        assert lib().mi_int1e(eng._h, vp(S2.data_ptr()), vp(T2.data_ptr()), None, None, org, eng._stream()) == 0
    assert np.array_equal(S2.cpu().numpy(), got[0]) and np.array_equal(T2.cpu().numpy(), got[1])
    dv = np.abs(V2.cpu().numpy() - got[2]).max()
    print(f"V alone against the full call: {dv:.1e} of max|V| {np.abs(got[2]).max():.1f}")
    assert dv <= 1e-13 * np.abs(got[2]).max()


@pytest.mark.parametrize("name,basis", CASES)
def test_jk_matches_oracle(name, basis):
    from mi355scf.engine import Engine
    from oracle import oracle as orc
    mol = _mol(name, basis)
    eng = Engine(mol)
    st = eng.prepare_eri(1e-13)
    assert st["n_tiles"] > 0 and st["n_unique_eri"] > 0
    D = _sym_density(mol.nao, 7)
    J, K = eng.get_jk(D)
    Jo, Ko = orc.Oracle(mol).jk(D, tol=0.0)
    assert np.abs(J.cpu().numpy() - Jo).max() < 1e-10, np.abs(J.cpu().numpy() - Jo).max()
    assert np.abs(K.cpu().numpy() - Ko).max() < 1e-10, np.abs(K.cpu().numpy() - Ko).max()
    # J-only and K-only variants of the kernel
    J2, _ = eng.get_jk(D, with_k=False)
    _, K2 = eng.get_jk(D, with_j=False)
    assert np.abs((J2 - J).cpu().numpy()).max() < 1e-11
    assert np.abs((K2 - K).cpu().numpy()).max() < 1e-11


def test_jk_linearity_and_symmetry_benzene_sized():
    """Size-independent properties at the bench size (benzene/cc-pVDZ, N=114): J,K symmetric, linear in D."""
    from mi355scf.engine import Engine
    from mi355scf.fixtures import BENZENE
    from mi355scf.mole import Mole
    mol = Mole(atom=BENZENE, basis="cc-pvdz").build()
    assert mol.nao == 114
    eng = Engine(mol)
    eng.prepare_eri(1e-13)
    D1, D2 = _sym_density(114, 1), _sym_density(114, 2)
    J1, K1 = eng.get_jk(D1)
    J2, K2 = eng.get_jk(D2)
    J3, K3 = eng.get_jk(D1 + 2.0 * D2)
    assert (J1 - J1.T).abs().max() < 1e-10 and (K1 - K1.T).abs().max() < 1e-10
    assert (J3 - J1 - 2 * J2).abs().max() < 1e-9
    assert (K3 - K1 - 2 * K2).abs().max() < 1e-9
    # trace identities: tr(D1 J2) == tr(D2 J1), tr(D1 K2) == tr(D2 K1)
    import torch
    d1, d2 = torch.as_tensor(D1, device=J1.device), torch.as_tensor(D2, device=J1.device)
    assert abs(float((d1 * J2).sum() - (d2 * J1).sum())) < 1e-8
    assert abs(float((d1 * K2).sum() - (d2 * K1).sum())) < 1e-8


def test_against_committed_golden_vectors():
    """HIP path vs tests/golden/h2co_631gd_vectors.npz (made by tests/golden/make_golden_vectors.py)."""
    import os
    import torch
    from mi355scf.engine import Engine
    from mi355scf.dft import RKS
    from mi355scf.fixtures import H2CO
    from mi355scf.mole import Mole
    g = np.load(os.path.join(os.path.dirname(__file__), "golden", "h2co_631gd_vectors.npz"))
    mol = Mole(atom=H2CO, basis="6-31g(d)", verbose=0).build()
    eng = Engine(mol)
    S, T, V, dip = (x.cpu().numpy() for x in eng.int1e(with_dipole=True))
    assert np.abs(S - g["S"]).max() < 1e-12 and np.abs(T - g["T"]).max() < 1e-11
    assert np.abs(V - g["V"]).max() < 1e-10 and np.abs(dip - g["dip"]).max() < 1e-11
    J, K = eng.get_jk(g["D"])
    assert np.abs(J.cpu().numpy() - g["J"]).max() < 1e-10 and np.abs(K.cpu().numpy() - g["K"]).max() < 1e-10
    mf = RKS(mol, xc="B3LYP")
    mf.grids.level = 1
    mf._setup_once()
    assert mf.grids.size == int(g["ngrid"]) and abs(float(mf.grids.weights.sum()) - float(g["wsum"])) < 1e-8
    n, exc, vxc, hyb = mf.nr_rks(torch.as_tensor(g["Docc"], device=eng.device))
    assert abs(float(n) - float(g["nelec"])) < 1e-9 and abs(float(exc) - float(g["exc"])) < 1e-9
    assert np.abs(vxc.cpu().numpy() - g["vxc"]).max() < 1e-9 and hyb == float(g["hyb"])


@pytest.mark.parametrize("name,basis", [("h2o", "cc-pvtz"), ("ch4", "cc-pvdz")])
def test_pair_kernel_two_densities_in_one_pass_equals_two_passes(name, basis):
    """`mi_build_jk(n_dm = 2)` through `jk_tiles_pair_kernel` (two waves per work item, one per density; default for stores beyond
    16 GB, forced here with `jk_pair = 1`) against one pass per density, J+K, J-only and K-only: 1e-11 (ragged last blocks included:
    N = 58 and N = 34 are not multiples of 8)."""
    import torch
    from mi355scf.engine import Engine
    mol = _mol(name, basis)
    eng = Engine(mol)
    eng.prepare_eri(1e-13)
    n = mol.nao
    D2 = torch.as_tensor(np.stack([_sym_density(n, 1), _sym_density(n, 2)]), device="cuda")
    eng.set_option("jk_pair", 0)
    Jr, Kr = eng.get_jk(D2)
    eng.set_option("jk_pair", 1)
    J, K = eng.get_jk(D2)
    assert float((J - Jr).abs().max()) < 1e-11 and float((K - Kr).abs().max()) < 1e-11
    Jj, _ = eng.get_jk(D2, with_k=False)
    _, Kk = eng.get_jk(D2, with_j=False)
    assert float((Jj - Jr).abs().max()) < 1e-11 and float((Kk - Kr).abs().max()) < 1e-11
