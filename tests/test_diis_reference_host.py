"""Host checks of tests/diis_reference.py, the references and inputs of tests/test_gpu_diis_chain.py: the references agree
with each other, the inputs reach the branches of the solve they are meant to reach, and FP64 LAPACK's backward error on the
very same systems is measured -- the yardstick the GPU bound is 8 x of.  No GPU.  Each test prints its figures (pytest -rP)."""
import types

import numpy as np
import pytest

import diis_reference as dr


@pytest.fixture(scope="module")
def grid():
    """[(key, case, B = the matrix the kernel solves with, model)] over the GPU test's grid, built once."""
    out = []
    for key in dr.solve_grid():
        family, m, space, slot, seed = key
        case = dr.solve_case(*key)
        out.append((key, case, dr.expected_B(case, m, slot), dr.kernel_model(case["part"], m, slot, space, case["B0"])))
    return out


@pytest.mark.parametrize("family", ["indep", "floor"])
def test_lapack_and_mpmath_agree_within_the_forward_bound(family):
    """numpy.linalg.solve against the 50-digit solution within 2 kappa eta / (1 - kappa eta), eta its own measured backward
    error.  In the scaled system `indep` and `floor` are well conditioned at every m (kappa_inf of a few units), so B4 of the
    GPU test applies to them everywhere; in the plain system kappa_inf ~ 1 / max|B| (1e24 at the floor) and the bound says
    nothing -- the comparison is made there only where kappa eta < 1/2."""
    worst_k, worst_ratio, n_plain = 0.0, 0.0, 0
    for m in range(1, dr.MAXM + 1):
        for seed in dr.SEEDS:
            B = dr.gram(dr.history(family, m, seed))
            s = dr.pow2_scale(B, m)
            for scale in (s, 1.0):
                A, b = dr.pulay_system(B * scale, m)
                x = np.linalg.solve(A, b)
                eta = dr.backward_error(A, b, x)
                ref, kappa = dr.exact_solution(A, b)
                if scale == 1.0 and s != 1.0:
                    if kappa * eta >= 0.5:
                        continue
                    n_plain += 1
                else:
                    worst_k = max(worst_k, kappa)
                    # the GPU test's gate for B4, with its bound 8 x yardstick in place of this eta
                    assert kappa * dr.BOUND_FACTOR * dr.YARDSTICK_SCALED[family] < dr.FORWARD_GATE, (m, seed, kappa)
                err = float(np.abs(x.astype(dr.LD) - ref).max() / np.abs(ref).max())
                bound = dr.forward_bound(kappa, max(eta, 2.0 ** -64))
                worst_ratio = max(worst_ratio, err / bound)
                assert err <= bound, (m, seed, scale, err, bound, kappa, eta)
    print(f"[references] {family}: scaled kappa_inf <= {worst_k:.1f}, worst error / bound {worst_ratio:.2f}, "
          f"{n_plain} plain systems with kappa eta < 1/2")


def test_the_grid_reaches_every_branch_of_the_solve(grid):
    """`kernel_model` over the GPU grid: a row interchange at a step k >= 1 for every m >= 2, the fallback, and the solved
    branch for every m."""
    inter = {m: 0 for m in range(1, dr.MAXM + 1)}
    solved = dict(inter)
    fallback = 0
    for (family, m, space, slot, seed), case, B, model in grid:
        inter[m] += any(k >= 1 for k in model["swaps"])
        solved[m] += not model["fallback"]
        fallback += model["fallback"]
        assert np.array_equal(model["B"], B)
    print(f"[coverage] {len(grid)} cases; interchanges at k >= 1 per m {inter}; solved per m {solved}; fallbacks {fallback}")
    assert all(inter[m] > 0 for m in range(2, dr.MAXM + 1))
    assert all(solved[m] > 0 for m in range(1, dr.MAXM + 1))
    assert fallback > 0


def test_inputs_have_the_properties_the_gpu_test_relies_on():
    """Unequal partials whose sum is the Gram entry to within a few ulps, sentinels where the kernel must not write, `dup`
    duplicated to the bit, and a model that falls back on it and on all-zero partials."""
    case = dr.solve_case("dup", 5, 16, 2, 0)
    part = case["part"].reshape(-1, dr.NS)[:5]
    assert np.abs(part - part.mean(axis=1, keepdims=True)).min() > 0.0
    assert np.allclose(dr.sequential_sum(part), case["Bfull"][:, 2], rtol=8 * dr.U, atol=0)
    assert np.all(case["B0"][5:] == dr.SENT_OUT) and np.all(case["B0"][:, 5:] == dr.SENT_OUT) and np.all(case["B0"][2, :5] == dr.SENT_ROW)
    V = dr.history("dup", 5, 0)
    assert np.array_equal(V[-1], V[0]) and np.array_equal(case["Bfull"][0], case["Bfull"][-1])
    assert dr.kernel_model(case["part"], 5, 2, 16, case["B0"])["fallback"]
    zero = dr.kernel_model(np.zeros(16 * dr.NS), 3, 1, 16, np.zeros((16, 16)))
    assert zero["fallback"] and np.array_equal(zero["coef"], [0.0, 1.0, 0.0])
    E, F = dr.chain_history(2, 2, 7)
    assert E.shape == (7, 2, 7, 7) and np.array_equal(F, np.swapaxes(F, -1, -2))


def test_lapack_yardstick(grid):
    """Worst backward error of numpy.linalg.solve per family over the grid (systems it reports singular, or solves with a
    non-finite value, skipped), in the plain and in the scaled metric, against the figures diis_reference records.  The recorded
    figures are the contract of the GPU test; a sample maximum moves with the BLAS build (kernel selection by CPU), so the
    re-measurement has to land within a factor 4 below and 2 above them, not on them."""
    plain = {f: 0.0 for f in dr.FAMILIES}
    scaled = dict(plain)
    for (family, m, space, slot, seed), case, B, model in grid:
        A, b = dr.pulay_system(B, m)
        try:
            x = np.linalg.solve(A, b)
        except np.linalg.LinAlgError:
            continue
        if not np.isfinite(x).all():
            continue
        plain[family] = max(plain[family], dr.backward_error(A, b, x))
        s = dr.pow2_scale(B, m)
        As, bs = dr.pulay_system(B[:m, :m] * s, m)
        x[0] *= s
        scaled[family] = max(scaled[family], dr.backward_error(As, bs, x))
    for f in dr.FAMILIES:
        print(f"[yardstick] {f:8s} LAPACK worst eta: plain {plain[f]:.3e} (recorded {dr.YARDSTICK[f]:.3e})  "
              f"scaled {scaled[f]:.3e} (recorded {dr.YARDSTICK_SCALED[f]:.3e})")
    for f in dr.FAMILIES:
        assert 0.25 * dr.YARDSTICK[f] <= plain[f] <= 2.0 * dr.YARDSTICK[f], (f, plain[f])
        assert 0.25 * dr.YARDSTICK_SCALED[f] <= scaled[f] <= 2.0 * dr.YARDSTICK_SCALED[f], (f, scaled[f])


@pytest.mark.parametrize("space", [0, 17])
def test_device_diis_refuses_a_space_the_kernel_cannot_hold(space):
    from mi355scf.scf import DeviceDIIS
    with pytest.raises(ValueError):
        DeviceDIIS(types.SimpleNamespace(nao=7), space)
