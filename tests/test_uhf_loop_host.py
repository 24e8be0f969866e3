"""The plain open-shell SCF loop (UHF above `sp2_min_nao`, every ROHF / ROKS) without a GPU.  The loop is plain torch plus one Fock
build per cycle, so on CPU tensors it is deterministic: convergence flag, cycle count and number of Fock builds are pinned exactly,
energies and orbital energies to 1e-11 (the margin covers another BLAS only), <S^2> to 1e-10.

Only three things are replaced: `_setup_once` (no engine), `_fock_pair` (dense einsum J/K on the CPU oracle's integrals, counted)
and, for ROHF, `rohf.rohf_fock` (the numpy Roothaan coupling of `test_gpu_rohf_kernel.py`).  The pinned values in
`golden/uhf_loop_host.json` were recorded with `python tests/test_uhf_loop_host.py` on the commit BEFORE the loops were folded into
`SCF._iterate` / `UHF._ufinal`; they are what that commit computed and are not to be re-recorded from a later one."""
import json
import os
import types

import numpy as np
import pytest

from test_gpu_rohf_kernel import ref_rohf_fock
from test_rohf_host import CH2, OH, mol_of, numpy_rohf, oracle_integrals

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "uhf_loop_host.json")
PKG = os.path.join(os.path.dirname(HERE), "computational-chemistry-ai_amd", "python", "mi355scf")

# id: (method, geometry, basis, spin, settings)
CASES = {
    "uhf-oh-sto3g": ("UHF", OH, "sto-3g", 1, {}),
    "uhf-oh-631g": ("UHF", OH, "6-31g", 1, {}),
    "uhf-oh-sto3g-no-conv-check": ("UHF", OH, "sto-3g", 1, {"conv_check": False}),
    "uhf-oh-sto3g-max-cycle-3": ("UHF", OH, "sto-3g", 1, {"max_cycle": 3}),      # unconverged: orbitals of the last in-loop eigh
    "uhf-ch2-sto3g-shift": ("UHF", CH2, "sto-3g", 2, {"level_shift": 0.3}),
    "uhf-oh-sto3g-diis-start-3": ("UHF", OH, "sto-3g", 1, {"diis_start_cycle": 3}),
    "rohf-oh-sto3g": ("ROHF", OH, "sto-3g", 1, {}),
    "rohf-ch2-sto3g": ("ROHF", CH2, "sto-3g", 2, {}),
    "rohf-oh-sto3g-shift": ("ROHF", OH, "sto-3g", 1, {"level_shift": 0.3}),
}


def _host_rohf_fock(fa, fb, ncore, nopen, nmo=None):
    import torch
    f, g = ref_rohf_fock(fa.numpy(), fb.numpy(), ncore, nopen)
    return torch.as_tensor(f), torch.as_tensor(g), torch.as_tensor([float((g * g).sum()), float(np.abs(g).max())])


def run_case(name, monkeypatch=None):
    """The finished driver object of a case, with `.calls` (one entry per Fock build) and the integrals as `.ints`."""
    import torch
    from mi355scf import rohf, uhf
    method, atom, basis, spin, settings = CASES[name]
    mol = mol_of(atom, basis, spin)
    S, h, eri = oracle_integrals(mol)

    def t(a):
        return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64)

    E = t(eri)
    if method == "ROHF":
        if monkeypatch is not None:
            monkeypatch.setattr(rohf, "rohf_fock", _host_rohf_fock)
        else:
            rohf.rohf_fock = _host_rohf_fock

    class Host(rohf.ROHF if method == "ROHF" else uhf.UHF):
        def _setup_once(self):
            pass

        def get_ovlp(self, mol=None):
            return S

        def _fock_pair(self, dm):
            self.calls.append("fock")
            J = torch.einsum("ijkl,kl->ij", E, dm[0] + dm[1])
            K = torch.einsum("ikjl,skl->sij", E, dm)
            F = self._h1.unsqueeze(0) + J.unsqueeze(0) - K
            return F, 0.5 * torch.sum(dm * (self._h1.unsqueeze(0) + F))

    mf = Host(mol)
    mf.calls, mf.ints = [], (S, h, eri)
    mf._eng = types.SimpleNamespace(nao=S.shape[0], device="cpu", mol=mol)
    mf._S, mf._h1 = t(S), t(h)
    mf._L = torch.linalg.cholesky(mf._S)
    mf._Linv = torch.linalg.inv(mf._L)
    mf.fast_loop = False
    for k, v in settings.items():
        setattr(mf, k, v)
    Li = mf._Linv.numpy()
    c = Li.T @ np.linalg.eigh(Li @ h @ Li.T)[1]      # aufbau density of the core Hamiltonian
    na, nb = mol.nelec
    mf.kernel(dm0=np.stack([c[:, :na] @ c[:, :na].T, c[:, :nb] @ c[:, :nb].T]))
    return mf


def observed(mf):
    return {"converged": bool(mf.converged), "cycles": int(mf.cycles), "fock_builds": len(mf.calls), "e_tot": float(mf.e_tot),
            "s2": float(mf.spin_square()[0]), "mo_energy": np.asarray(mf.mo_energy).tolist()}


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.mark.parametrize("name", sorted(CASES))
def test_plain_loop_computes_what_it_computed_before_the_refactor(name, golden, monkeypatch):
    mf = run_case(name, monkeypatch)
    got, ref = observed(mf), golden[name]
    print(name, {k: got[k] for k in ("converged", "cycles", "fock_builds", "e_tot", "s2")})
    assert (got["converged"], got["cycles"], got["fock_builds"]) == (ref["converged"], ref["cycles"], ref["fock_builds"])
    assert abs(got["e_tot"] - ref["e_tot"]) <= 1e-11
    assert np.shape(got["mo_energy"]) == np.shape(ref["mo_energy"])
    assert np.abs(np.asarray(got["mo_energy"]) - np.asarray(ref["mo_energy"])).max() <= 1e-11
    assert abs(got["s2"] - ref["s2"]) <= 1e-10
    S, h, eri = mf.ints
    n, (na, nb) = S.shape[0], mf.mol.nelec
    C, dm, F = np.asarray(mf.mo_coeff), mf.make_rdm1(), mf._fock.numpy()
    if CASES[name][0] == "ROHF":
        assert abs(got["e_tot"] - numpy_rohf(mf.mol, S, h, eri)[0]) <= 1e-9
        # one orbital set, occupations 2 / 1 / 0, the per-spin diagonals of the returned Fock pair on mo_energy
        assert C.shape == (n, n) and mf.mo_occ.tolist() == [2.0] * nb + [1.0] * (na - nb) + [0.0] * (n - na)
        assert np.abs(mf.mo_energy.mo_ea - np.einsum("pi,pq,qi->i", C, F[0], C)).max() <= 1e-12
        assert np.abs(mf.mo_energy.mo_eb - np.einsum("pi,pq,qi->i", C, F[1], C)).max() <= 1e-12
        occ = (C[:, :na], C[:, :nb])
    else:
        assert C.shape == (2, n, n) and mf.mo_occ.sum(axis=1).tolist() == [na, nb]
        occ = (C[0][:, :na], C[1][:, :nb])
    if ref["converged"] and CASES[name][4].get("conv_check", True):
        # the extra cycle: the returned density is the one of the returned orbitals, the energy that of this density
        assert all(np.abs(dm[s_] - occ[s_] @ occ[s_].T).max() <= 1e-12 for s_ in range(2))
        D = dm[0] + dm[1]
        J = np.einsum("ijkl,kl->ij", eri, D)
        e_el = sum(0.5 * np.sum(dm[s_] * (2.0 * h + J - np.einsum("ikjl,kl->ij", eri, dm[s_]))) for s_ in range(2))
        assert abs(e_el + mf.mol.energy_nuc() - got["e_tot"]) <= 1e-11


def _source(name):
    with open(os.path.join(PKG, name)) as f:
        return f.read()


def test_the_projector_side_channel_is_gone():
    for name in sorted(os.listdir(PKG)):
        if name.endswith(".py"):
            assert "_plain_projectors" not in _source(name), name


def test_one_outer_loop_and_one_finish():
    """`SCF.kernel` and both open-shell loops run the one `SCF._iterate`; the open-shell loops end in the one `UHF._ufinal` and
    `UHF._uresult`, ROHF overriding `_set_orbitals` only; the two loop functions with outer loops of their own are gone."""
    from mi355scf import rohf, scf, uhf
    assert not hasattr(uhf.UHF, "_kernel_plain") and not hasattr(uhf.UHF, "_kernel_fast")
    for attr in ("_plain_start", "_plain_density", "_plain_step", "_ufinal", "_set_orbitals", "_uresult", "_iterate", "_start",
                 "_step"):
        assert callable(getattr(uhf.UHF, attr)), attr
    assert uhf.UHF._iterate is scf.SCF._iterate and rohf.ROHF._ufinal is uhf.UHF._ufinal
    assert rohf.ROHF._uresult is uhf.UHF._uresult and rohf.ROHF._set_orbitals is not uhf.UHF._set_orbitals
    assert "self._iterate(" in _source("scf.py") and "self._iterate(" in _source("uhf.py")


if __name__ == "__main__":      # record the pins (see the module docstring for when)
    import sys
    sys.path[:0] = [os.path.dirname(PKG), os.path.dirname(HERE)]
    out = {name: observed(run_case(name)) for name in CASES}
    with open(GOLDEN, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    for name, v in out.items():
        print(name, v["converged"], v["cycles"], v["fock_builds"], repr(v["e_tot"]), v["s2"])
