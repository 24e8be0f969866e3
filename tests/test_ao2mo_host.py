"""Host-side checks of `mi355scf.ao2mo` (no GPU): the symmetrisation, the work-space figure and the batch rule of the
transformation, and the `frozen` mask."""
import numpy as np
import pytest


def test_symmetrize8_is_the_mean_of_the_eight_permutations_and_exactly_symmetric():
    import torch
    from mi355scf.ao2mo import symmetrize8
    x = np.random.default_rng(8).standard_normal((5, 5, 5, 5))
    perms = {k + b if pairs else b + k for pairs in (False, True) for b in ((0, 1), (1, 0)) for k in ((2, 3), (3, 2))}
    assert len(perms) == 8
    mean = sum(x.transpose(p) for p in sorted(perms)) / 8.0
    y = symmetrize8(torch.from_numpy(x.copy())).numpy()
    err = np.abs(y - mean).max() / np.abs(mean).max()
    print(f"symmetrize8: max |y - mean of 8| / max |mean| = {err:.2e}")
    assert err <= 1e-15
    for name, p in (("(rs|pq)", (2, 3, 0, 1)), ("(qp|rs)", (1, 0, 2, 3)), ("(pq|sr)", (0, 1, 3, 2))):
        assert np.array_equal(y, y.transpose(p)), name                      # bitwise
    assert np.array_equal(symmetrize8(torch.from_numpy(y.copy())).numpy(), y)


def test_qtrans_work_bytes_counts_the_tensors_of_a_transformation():
    """Per column of C1: Y [N, N, N] beside the kernel's padded accumulator, then beside the first GEMM's output [n, N, N]."""
    from mi355scf.ao2mo import qtrans_work_bytes
    for N in (13, 264):
        ldp = 8 * ((N + 7) // 8) + 8
        assert ldp % 8 == 0 and N + 8 <= ldp < N + 16
        for n in (1, 5, N, 2 * N):
            need = qtrans_work_bytes(N, n)
            assert need >= 8 * (N ** 3 + max(ldp ** 3, n * N * N))
            assert need >= 8 * (N ** 3 + ldp ** 3) and need >= 8 * (N ** 3 + n * N * N)
            assert need <= 8 * (N ** 3 + ldp ** 3 + n * N * N)
    assert abs(qtrans_work_bytes(264, 243) * 1e-9 - 0.308) < 0.001            # benzene / cc-pVTZ: 264^3 + 272^3 doubles


class _StubEngine:
    nao, device = 13, "cpu"

    @staticmethod
    def qtrans_batch():
        return 8


def test_batch_rule(monkeypatch):
    import torch
    from mi355scf import mp2
    from mi355scf.ao2mo import plan_qtrans_batch
    per = 1000
    free = [0.0]
    monkeypatch.setattr(torch.cuda, "empty_cache", lambda: None)
    monkeypatch.setattr(torch.cuda, "mem_get_info", lambda *a, **k: (free[0], 10 ** 12))
    eng = _StubEngine()

    def room(orbitals, reserve=0):           # free HBM of which 80 %, less the reserve, hold this many orbitals
        free[0] = (orbitals * per + reserve) / 0.8
        return plan_qtrans_batch(eng, 100, per, reserve_bytes=reserve)

    assert room(19.5) == (16, free[0])                                        # whole passes of 8
    assert room(5.5) == (5, free[0])                                          # below one pass: as many as fit
    assert room(8.5)[0] == 8 and room(16.5)[0] == 16 and room(7.5)[0] == 7
    assert room(19.5, reserve=10 ** 6)[0] == 16 and room(0.5, reserve=10 ** 6)[0] == 0
    assert room(1000.5)[0] == 100                                             # at most n_first
    assert room(0.9) == (0, free[0])                                          # fewer than one: the caller refuses

    class _StubSCF:
        mol, verbose, engine = None, 0, eng

        def _log(self, level, msg):
            pass

    pt = mp2.MP2(_StubSCF())
    with pytest.raises(MemoryError, match="one occupied orbital needs"):
        pt._plan_batch(5, 8)
    free[0] = 1e12
    assert pt._plan_batch(5, 8) == 5 and pt._plan_batch(40, 8) == 40
    free[0] = 0.0                                                             # forced: nothing is looked up
    assert plan_qtrans_batch(eng, 100, per, forced=3) == (3, None)
    assert plan_qtrans_batch(eng, 2, per, forced=3) == (2, None)
    pt.occ_batch = 3
    assert pt._plan_batch(5, 8) == 3 and pt._plan_batch(2, 8) == 2


def test_frozen_selects_orbitals():
    from mi355scf import mp2
    from mi355scf.ao2mo import active_mask
    assert mp2._active is active_mask
    assert active_mask(None, 5).all() and active_mask(0, 5).all()
    assert active_mask(2, 5).tolist() == [False, False, True, True, True]
    assert active_mask([0, 4], 5).tolist() == [False, True, True, True, False]
    assert active_mask(np.int64(1), 3).tolist() == [False, True, True]
    for bad in (-1, 6, [5], [-1]):
        with pytest.raises(ValueError):
            active_mask(bad, 5)
