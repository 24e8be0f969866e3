"""The device CDIIS tail pinned to exact Pulay references: `mi_diis_solve` over its whole range (m = 1..16), its refusals,
`scf.DeviceDIIS` driven as the SCF drives it, SCFs at the subspace sizes no other test runs, and the convergence floor.
References and inputs: tests/diis_reference.py (checked on the host by tests/test_diis_reference_host.py).

The contract of the solve
  B1  row and column `slot` of B receive the 16 partials added left to right from 0.0, bit for bit; no other element of B,
      nothing of coef at index >= m and nothing of the partials changes.
  B2  the coefficients are exactly e_slot (the fallback: no extrapolation) or all finite.  `indep`, `geom`, `scales` and `floor`
      never fall back.
  B3  a solved case has backward error eta([lambda; c]) <= 8 x the worst eta of FP64 LAPACK on the same grid, lambda taken from
      row slot + 1 of the system in long double -- in the plain system and in the scaled one (diis_reference: B times the power
      of two that brings max|B| to [1, 2), the metric in which a small B still counts).
  B4  where kappa_inf x (B3 bound) < 1e-3: |c - c_exact|_inf <= 2 kappa eta_b / (1 - kappa eta_b) |c_exact|_inf, c_exact from
      mpmath at 50 digits, in whichever of the two systems qualifies.  Scaled, `indep` and `floor` qualify at every m.
  B5  all-zero partials, or a NaN or an Inf among them, give e_slot exactly; B still receives the sums.

LAPACK yardsticks (numpy.linalg.solve, worst eta over the 1044-case grid; plain / scaled):
  indep 4.88e-17 / 1.70e-16   geom 2.47e-17 / 1.44e-17   scales 4.84e-18 / 2.12e-17
  floor 6.94e-17 / 1.40e-16   dup  1.05e-16 / 3.35e-17   neardup 2.09e-16 / 2.50e-16
Every test prints its figures (pytest -rP)."""
import math

import numpy as np
import pytest

import diis_reference as dr

pytestmark = pytest.mark.gpu

LD = dr.LD
TINY = np.finfo(LD).tiny
WATER = "O 0 0 0; H 0 -0.757 0.587; H 0 0.757 0.587"
OH = "O 0 0 0; H 0 0 0.97"


@pytest.fixture(scope="module")
def eng():
    from mi355scf.engine import Engine
    from mi355scf.mole import Mole
    return Engine(Mole(atom=WATER, basis="sto-3g", verbose=0).build())


def _dev(a):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64), device="cuda").contiguous()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _run_solve(eng, part, m, slot, space, B0, coef0):
    import torch
    pd, Bd, cd = _dev(part), _dev(B0), _dev(coef0)
    eng.diis_solve(pd, m, slot, space, Bd, cd)
    torch.cuda.synchronize()
    return pd.cpu().numpy(), Bd.cpu().numpy(), cd.cpu().numpy()


def _e(slot, m):
    e = np.zeros(m)
    e[slot] = 1.0
    return e


def _check_b3_b4(family, B, m, slot, c):
    """(worst eta / bound over the two metrics, number of B4 comparisons made, worst B4 error / bound) of a solved case."""
    worst, n4, worst4 = 0.0, 0, 0.0
    for scaled, yard in ((False, dr.YARDSTICK[family]), (True, dr.YARDSTICK_SCALED[family])):
        bound = dr.BOUND_FACTOR * yard
        eta = dr.eta_of_coefficients(B, m, c, slot, scaled=scaled)
        worst = max(worst, eta / bound)
        assert eta <= bound, (family, m, slot, "scaled" if scaled else "plain", eta, bound)
        s = dr.pow2_scale(B, m) if scaled else 1.0
        if scaled and s == 1.0:
            continue
        A, b = dr.pulay_system(B[:m, :m] * s, m)
        if np.linalg.cond(A, np.inf) * bound >= dr.FORWARD_GATE:          # cheap FP64 look before the 50-digit inverse
            continue
        ref, kappa = dr.exact_solution(A, b)
        if not kappa * bound < dr.FORWARD_GATE:
            continue
        err = float(np.abs(np.asarray(c, dtype=LD) - ref[1:]).max())
        lim = dr.forward_bound(kappa, bound) * float(np.abs(ref[1:]).max())
        n4 += 1
        worst4 = max(worst4, err / lim)
        assert err <= lim, (family, m, slot, "scaled" if scaled else "plain", err, lim, kappa)
    return worst, n4, worst4


# --- a. the solve over its whole range ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", dr.FAMILIES)
def test_solve_contract_over_the_whole_range(eng, family):
    """B1 to B4 at m = 1..16 x space in {m, 16} x slot in {0, m // 2, m - 1} x 2 seeds of one family."""
    per_m = {m: 0.0 for m in range(1, dr.MAXM + 1)}
    fallbacks, solved, n4, worst4, cmax, solved_m1 = 0, 0, 0, 0.0, 0.0, 0
    for key in dr.solve_grid():
        if key[0] != family:
            continue
        _f, m, space, slot, seed = key
        case = dr.solve_case(*key)
        part, B, coef = _run_solve(eng, case["part"], m, slot, space, case["B0"], case["coef0"])
        # B1
        want = dr.expected_B(case, m, slot)
        assert np.array_equal(_bits(B[slot, :m]), _bits(dr.sequential_sum(case["part"].reshape(-1, dr.NS)[:m]))), key
        assert np.array_equal(_bits(B[:m, slot]), _bits(B[slot, :m])), key
        assert np.array_equal(_bits(B), _bits(want)), key
        assert np.array_equal(_bits(coef[m:]), _bits(case["coef0"][m:])) and np.array_equal(_bits(part), _bits(case["part"])), key
        # B2
        c = coef[:m]
        if m > 1 and np.array_equal(c, _e(slot, m)):
            fallbacks += 1
            assert family in ("dup", "neardup"), key        # a well-posed history is extrapolated, never dropped
            continue
        assert np.isfinite(c).all(), (key, c)
        solved += 1
        solved_m1 += m == 1
        cmax = max(cmax, float(np.abs(c).max()))
        # B3, B4
        w, k4, w4 = _check_b3_b4(family, B, m, slot, c)
        per_m[m] = max(per_m[m], w)
        n4 += k4
        worst4 = max(worst4, w4)
    print(f"[solve] {family}: solved {solved} ({solved_m1} of them m = 1), fallbacks {fallbacks}, largest |c| {cmax:.2e}; worst eta / bound per m "
          f"{ {m: round(v, 3) for m, v in per_m.items()} }; B4 comparisons {n4}, worst error / bound {worst4:.3f}")
    assert solved > 0
    if family in ("indep", "floor"):
        assert n4 >= solved                                  # (every case qualifies in the scaled system)


def test_solve_falls_back_on_zero_and_non_finite_partials(eng):
    """B5.  All-zero partials; one NaN, +Inf or -Inf at every row of the newest Gram row in turn."""
    n = 0
    for m, space, slot in ((1, 1, 0), (3, 8, 1), (9, 16, 8), (16, 16, 0), (16, 16, 7)):
        case = dr.solve_case("indep", m, space, slot, 0)
        zero = np.zeros_like(case["part"])
        _p, B, coef = _run_solve(eng, zero, m, slot, space, np.zeros((space, space)), case["coef0"])
        assert np.array_equal(coef[:m], _e(slot, m)) and np.array_equal(_bits(coef[m:]), _bits(case["coef0"][m:]))
        assert not B.any()
        for bad in (math.nan, math.inf, -math.inf):
            for row in range(m):
                part = case["part"].copy()
                part[row * dr.NS + (5 * row + 3) % dr.NS] = bad
                _p, B, coef = _run_solve(eng, part, m, slot, space, case["B0"], case["coef0"])
                assert np.array_equal(coef[:m], _e(slot, m)), (m, space, slot, bad, row, coef[:m])
                want = dr.expected_B(dict(case, part=part), m, slot)
                assert np.array_equal(B, want, equal_nan=True), (m, space, slot, bad, row)
                n += 1
    print(f"[solve] B5: {n} non-finite cases, all e_slot")


# --- b. refusals -----------------------------------------------------------------------------------------------------------------
def test_solve_refuses_what_it_cannot_hold(eng):
    import torch
    from mi355scf.engine import lib
    space = 16
    # B sits in the middle of a larger buffer and every operand outlives the calls: a call accepted by mistake stays inside
    guard = _dev(np.full(3 * space * space, dr.SENT_OUT))
    B = guard[space * space:2 * space * space]
    part, coef = _dev(np.full(space * dr.NS, 0.5)), _dev(np.full(space, dr.SENT_COEF))
    G0, c0 = guard.cpu().numpy(), coef.cpu().numpy()
    f = lib().mi_diis_solve
    stream = eng._stream()
    big, part17, coef17 = _dev(np.full((17, 17), dr.SENT_OUT)), _dev(np.zeros(17 * dr.NS)), _dev(np.full(17, dr.SENT_COEF))
    cases = {
        "m = 0": (eng._h, part.data_ptr(), 0, 0, space, B.data_ptr(), coef.data_ptr()),
        "m = 17": (eng._h, part17.data_ptr(), 17, 0, 17, big.data_ptr(), coef17.data_ptr()),
        "space < m": (eng._h, part.data_ptr(), 5, 0, 4, B.data_ptr(), coef.data_ptr()),
        "slot = -1": (eng._h, part.data_ptr(), 5, -1, space, B.data_ptr(), coef.data_ptr()),
        "slot = m": (eng._h, part.data_ptr(), 5, 5, space, B.data_ptr(), coef.data_ptr()),
        "null context": (None, part.data_ptr(), 5, 0, space, B.data_ptr(), coef.data_ptr()),
        "null partials": (eng._h, None, 5, 0, space, B.data_ptr(), coef.data_ptr()),
        "null B": (eng._h, part.data_ptr(), 5, 0, space, None, coef.data_ptr()),
        "null coef": (eng._h, part.data_ptr(), 5, 0, space, B.data_ptr(), None),
    }
    for name, a in cases.items():
        assert f(*a, stream) != 0, name
        torch.cuda.synchronize()
        assert np.array_equal(_bits(guard.cpu().numpy()), _bits(G0)) and np.array_equal(_bits(coef.cpu().numpy()), _bits(c0)), name
        assert np.all(big.cpu().numpy() == dr.SENT_OUT) and np.all(coef17.cpu().numpy() == dr.SENT_COEF), name
    assert f(eng._h, part.data_ptr(), 5, 0, space, B.data_ptr(), coef.data_ptr(), stream) == 0      # the same call, valid
    torch.cuda.synchronize()
    assert np.isfinite(coef.cpu().numpy()[:5]).all()


# --- c. DeviceDIIS as the SCF drives it ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def engines(eng):
    from mi355scf.engine import Engine
    from mi355scf.mole import Mole
    return {7: eng, 1: Engine(Mole(atom="He 0 0 0", basis="sto-3g", verbose=0).build())}


class _Mirror:
    """The ring of DeviceDIIS on the host."""

    def __init__(self, space, shape):
        self.space, self.count = space, 0
        self.E, self.F = np.zeros((space,) + shape), np.zeros((space,) + shape)

    def push(self, e, f):
        slot = self.count % self.space
        self.E[slot], self.F[slot] = e, f
        self.count += 1
        return slot, min(self.count, self.space)


def _push(diis, mir, e, f):
    slot = diis.next_slot()
    diis.F[slot].copy_(_dev(f))
    diis.E[slot].copy_(_dev(e))
    assert mir.push(e, f)[0] == slot
    m = diis.push_inplace()
    assert m == min(mir.count, mir.space) and diis.count == mir.count
    return slot, m


def _check_push(diis, mir, slot, m, length, stats):
    import torch
    torch.cuda.synchronize()
    B = diis.B_dev.cpu().numpy()
    c = diis.coef_dev.cpu().numpy()[:m].copy()
    V = mir.E[:m].reshape(m, -1).astype(LD)
    G, S = V @ V.T, np.abs(V) @ np.abs(V).T
    # Gram matrix: symmetric to the bit; every entry that of the CURRENT history (a wrong slot or a stale row is off by O(1))
    assert np.array_equal(_bits(B[:m, :m]), _bits(B[:m, :m].T)), (mir.count, slot)
    gerr = np.abs(B[:m, :m].astype(LD) - G)
    assert np.all(gerr <= dr.gamma(length) * S), (mir.count, slot, float((gerr / (dr.gamma(length) * S + TINY)).max()))
    # coefficients: B3 against the long-double Gram matrix of the history (recorded here, asserted by the caller after it has
    # printed every figure) and, as an extra, against the matrix the device holds
    if m > 1 and np.array_equal(c, _e(slot, m)):
        stats["fallback"] += 1
    else:
        assert np.isfinite(c).all(), (mir.count, c)
        for scaled, yard in ((False, dr.YARDSTICK["geom"]), (True, dr.YARDSTICK_SCALED["geom"])):
            bound = dr.BOUND_FACTOR * yard
            eta = dr.eta_of_coefficients(B, m, c, slot, scaled=scaled)
            s = LD(dr.pow2_scale(B, m)) if scaled else LD(1)
            Ag, bg = dr.pulay_system(G * s, m)
            lam = dr.lambda_from_row(Ag, bg, c, slot + 1)
            x = np.concatenate([[lam], c.astype(LD)])
            eta_g = dr.backward_error(Ag, bg, x)
            key = "scaled" if scaled else "plain"
            stats[key] = max(stats[key], eta / bound)
            if eta_g / bound > stats[key + "_gram"]:
                stats[key + "_gram"], stats[key + "_gram_at"] = eta_g / bound, (mir.count, m, slot)
            assert eta <= bound, (mir.count, m, slot, key, eta, bound)
    # combination: m fused multiply-adds with the device's own coefficients, one rounding each; a second call gives a new
    # tensor with the same bits (the captured SCF head relies on that)
    out = diis.extrapolate()
    out2 = diis.extrapolate()
    torch.cuda.synchronize()
    assert out2.data_ptr() != out.data_ptr() and out.shape == diis.F[0].shape
    o = out.cpu().numpy()
    assert np.array_equal(_bits(o), _bits(out2.cpu().numpy()))
    terms = c.astype(LD).reshape((m,) + (1,) * (mir.F.ndim - 1)) * mir.F[:m].astype(LD)
    cerr = np.abs(o.astype(LD) - terms.sum(axis=0))
    lim = dr.gamma(m) * np.abs(terms).sum(axis=0)
    assert np.all(cerr <= lim), (mir.count, slot, float((cerr / (lim + TINY)).max()))
    stats["comb"] = max(stats["comb"], float((cerr / (lim + TINY)).max()))
    return B, c, o


@pytest.mark.parametrize("nao", [1, 7])
@pytest.mark.parametrize("nmat", [1, 2])
@pytest.mark.parametrize("space", [1, 2, 8, 9, 16])
def test_device_diis_ring_as_the_scf_drives_it(engines, space, nmat, nao):
    """2 space + 3 pushes of a `geom` history through next_slot / push_inplace / extrapolate next to a host mirror of the ring:
    slot wrap, replacement of the stale row and column, the spin-stacked pair (nmat = 2), then a bitwise fixed point.
    B3 (eta <= 8 x the `geom` yardstick, plain and scaled) is asserted against the long-double Gram matrix of the history and,
    as an extra, against the matrix the device holds (what the kernel solved)."""
    import torch
    from mi355scf.scf import DeviceDIIS
    diis = DeviceDIIS(engines[nao], space, nmat=nmat)
    E, F = dr.chain_history(space, nmat, nao)
    mir = _Mirror(space, E.shape[1:])
    length = nmat * nao * nao
    stats = dict(fallback=0, plain=0.0, scaled=0.0, plain_gram=0.0, scaled_gram=0.0, comb=0.0, plain_gram_at=None, scaled_gram_at=None)
    for k in range(E.shape[0]):
        slot, m = _push(diis, mir, E[k], F[k])
        assert slot == k % space and m == min(k + 1, space)
        _check_push(diis, mir, slot, m, length, stats)
    # fixed point: the pair pushed now is, bit for bit, the oldest pair the ring still holds afterwards
    old = (mir.count - (space - 1)) % space if space > 1 else mir.count % space
    e_fix, f_fix = (mir.E[old].copy(), mir.F[old].copy()) if space > 1 else (E[-1], F[-1])
    slot, m = _push(diis, mir, e_fix, f_fix)
    torch.cuda.synchronize()
    B = diis.B_dev.cpu().numpy()
    c = diis.coef_dev.cpu().numpy()[:m].copy()
    o = diis.extrapolate().cpu().numpy()
    if np.array_equal(_bits(o), _bits(mir.F[slot])):
        how = "F[slot] to the bit"
    else:
        keep = [i for i in range(m) if i != old]                     # the history without the older copy
        Bk = B[np.ix_(keep, keep)]
        best = math.inf
        for s in (1.0, dr.pow2_scale(Bk, len(keep))):
            yard = dr.YARDSTICK["geom"] if s == 1.0 else dr.YARDSTICK_SCALED["geom"]
            A, b = dr.pulay_system(Bk * s, len(keep))
            ref, kappa = dr.exact_solution(A, b)
            if ref is not None and 2 * kappa * dr.BOUND_FACTOR * yard < best:
                best, c_ref = 2 * kappa * dr.BOUND_FACTOR * yard, ref[1:]
        assert math.isfinite(best), (space, nmat, nao, c)
        terms = c_ref.reshape((len(keep),) + (1,) * (mir.F.ndim - 1)) * mir.F[keep].astype(LD)
        lim = dr.gamma(m) * np.abs(terms).sum(axis=0) + np.abs(mir.F[:m]).max() * best
        err = np.abs(o.astype(LD) - terms.sum(axis=0))
        how = f"within {float((err / lim).max()):.2e} of the bound around the de-duplicated history, max|c| {np.abs(c).max():.2e}"
        assert np.all(err <= lim), (space, nmat, nao, how)
    print(f"[ring] space {space} nmat {nmat} nao {nao}: {mir.count} pushes, fallbacks {stats['fallback']}, worst eta / bound "
          f"against the long-double Gram matrix plain {stats['plain_gram']:.3f} scaled {stats['scaled_gram']:.3f} (against the device's "
          f"own B: {stats['plain']:.3f}, {stats['scaled']:.3f}), combination error / bound {stats['comb']:.3f}; fixed point: {how}")
    assert stats["plain_gram"] <= 1.0, ("push, m, slot", stats["plain_gram_at"], stats["plain_gram"])
    assert stats["scaled_gram"] <= 1.0, ("push, m, slot", stats["scaled_gram_at"], stats["scaled_gram"])


# --- d. SCFs at diis_space 1, 9 and 16 -------------------------------------------------------------------------------------------
def _mol(atom, basis, spin=0):
    from pyscf import gto
    m = gto.Mole()
    m.atom, m.basis, m.spin, m.verbose = atom, basis, spin, 0
    m.build()
    return m


@pytest.fixture(scope="module")
def water():
    from oracle import oracle as orc
    mol = _mol(WATER, "6-31G(d)")
    ref = orc.rhf(mol)
    assert ref["converged"]
    return mol, ref["e_tot"]


@pytest.mark.parametrize("space", [1, 9, 16])
def test_rhf_converges_at_unusual_diis_spaces(water, space):
    from pyscf import scf
    mol, e_ref = water
    mf = scf.RHF(mol)
    mf.diis_space = space
    mf.max_cycle = 100          # (space 1 is no extrapolation at all: plain Roothaan steps)
    e = mf.kernel()
    print(f"[scf] RHF H2O/6-31G(d) diis_space {space}: {mf.cycles} cycles, E - oracle {e - e_ref:.2e}")
    assert mf.converged and abs(e - e_ref) < 1e-8


@pytest.fixture(scope="module")
def hydroxyl():
    from pyscf import scf
    from oracle import oracle as orc
    mol = _mol(OH, "6-31G*", 1)
    dm0 = scf.UHF(mol).to_gpu().get_init_guess()
    return mol, dm0, orc.uhf(mol, dm0=dm0, conv_tol=1e-11)[0]


@pytest.mark.parametrize("space", [1, 16])
def test_uhf_converges_at_unusual_diis_spaces(hydroxyl, space):
    """As tests/test_gpu_uhf.py::test_uhf_matches_oracle: same initial density as the oracle, conv_tol 1e-10, 1e-7."""
    from pyscf import scf
    mol, dm0, e_ref = hydroxyl
    mf = scf.UHF(mol).to_gpu()
    mf.conv_tol, mf.diis_space, mf.max_cycle = 1e-10, space, 200
    e = mf.kernel(dm0=dm0)
    print(f"[scf] UHF OH/6-31G* diis_space {space}: {mf.cycles} cycles, E - oracle {e - e_ref:.2e}")
    assert mf.converged and abs(e - e_ref) < 1e-7
    dm = mf.make_rdm1()
    S = mf.get_ovlp()
    na, nb = mol.nelec
    assert abs(np.trace(dm[0] @ S) - na) < 1e-8 and abs(np.trace(dm[1] @ S) - nb) < 1e-8


def test_scf_refuses_diis_space_17(water):
    from pyscf import scf
    mf = scf.RHF(water[0])
    mf.diis_space = 17
    with pytest.raises(ValueError):
        mf.kernel()


# --- e. the convergence floor ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def water_df_energy(water):
    from pyscf import scf
    mf = scf.RHF(water[0]).density_fit()
    e = mf.kernel()
    assert mf.converged
    return e


FLOOR_RUNS = [(space, eig, fitted, graph) for fitted in (False, True) for eig in ("sp2", "eigh") for space in (2, 8, 16)
              for graph in ((False, True) if space != 16 else (False,))]


@pytest.mark.parametrize("space,eig,fitted,graph", FLOOR_RUNS)
def test_scf_holds_its_energy_at_the_convergence_floor(water, water_df_energy, space, eig, fitted, graph):
    """40 cycles with conv_tol = 0: the error vectors end as rounding noise plus a systematic part, the fitted path (free of
    atomics) can reach a bitwise fixed point.  From some cycle k0 <= 20 on, every energy stays within 1e-8 of the reference.
    Measured: k0 = 9 (space 2) or 6 (spaces 8, 16) in all 20 variants; from cycle 20 on |E - E_ref| <= 3.6e-13 on the resident
    tiles and <= 2.0e-12 fitted; no redone cycle, no fallback cycle; largest |c| 971 (space 16, SP2), otherwise below 12."""
    import torch
    from pyscf import scf
    mol, e_ref = water
    mf = scf.RHF(mol)
    if fitted:
        mf = mf.density_fit()
        e_ref = water_df_energy
    mf.conv_tol, mf.max_cycle, mf.diis_space, mf.eig_method, mf.graph_front = 0.0, 40, space, eig, graph
    energies, coefs = [], []
    step = mf._step

    def recorded(st, *a, **kw):
        out = step(st, *a, **kw)
        energies.append(float(st["e_tot"]))
        diis = st["diis"]
        if hasattr(diis, "coef_dev"):
            coefs.append((diis._pending, diis.coef_dev.clone()))        # device copy in stream order: read after the run
        return out

    mf._step = recorded
    e = mf.kernel()
    torch.cuda.synchronize()
    fallback = sum(1 for (slot, m), c in coefs if m > 1 and np.array_equal(c.cpu().numpy()[:m], _e(slot, m)))
    big = max((float(c[:m].abs().max()) for (slot, m), c in coefs), default=0.0)
    err = np.abs(np.array(energies) - e_ref)
    inside = err < 1e-8
    k0 = next((k for k in range(len(err)) if inside[k:].all()), None)
    heads = len((mf.__dict__.get("_fgraph") or {}).get("heads", []))
    print(f"[floor] space {space} {eig} {'fitted' if fitted else 'plain'} graph_front {graph}: cycles {len(energies)}, k0 "
          f"{None if k0 is None else k0 + 1}, worst |E - E_ref| from cycle 20 on {err[19:].max():.2e}, last {err[-1]:.2e}, n_redo "
          f"{getattr(mf, 'n_redo', 0)}, fallback cycles {fallback}, largest |c| {big:.2e}, captured heads {heads}, paths {getattr(mf, 'path_counts', {})}")
    assert len(energies) == 40 and np.isfinite(energies).all() and np.isfinite(e)
    assert mf.converged is False
    assert mf.graph_front is graph               # (a head that could not be captured would have switched it off)
    assert k0 is not None and k0 + 1 <= 20, (k0, err.tolist())
