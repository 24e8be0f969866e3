"""Host-side checks of the streaming MP2 (no GPU): the C-ABI entry points are exported, the `frozen` conventions select the
orbitals PySCF's do [MEM], and the `mp` namespaces of both drop-in packages resolve the names the templates use."""
import ctypes
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_qtrans_entry_points_are_exported_and_declared():
    from mi355scf import engine
    L = ctypes.CDLL(engine.LIB_PATH)
    assert L.mi_eri_qtrans is not None
    assert 1 <= int(L.mi_eri_qtrans_batch()) <= 16
    assert int(L.mi_abi_version()) == 2                       # an added entry point does not bump the ABI version
    hdr = open(os.path.join(ROOT, "include", "mi355scf.h")).read()
    assert "int mi_eri_qtrans(mi_ctx *ctx, const double *d_C, int nb, int ldc, double *d_Y, void *stream);" in hdr
    assert engine.Engine.qtrans_batch() == int(L.mi_eri_qtrans_batch())


def test_frozen_selects_orbitals():
    from mi355scf.mp2 import _active
    assert _active(None, 5).all() and _active(0, 5).all()
    assert _active(2, 5).tolist() == [False, False, True, True, True]
    assert _active([0, 4], 5).tolist() == [False, True, True, True, False]
    assert _active(np.int64(1), 3).tolist() == [False, True, True]
    for bad in (-1, 6, [5], [-1]):
        with pytest.raises(ValueError):
            _active(bad, 5)


def test_mp_namespaces_resolve():
    import gpu4pyscf.mp
    import pyscf.mp
    from mi355scf import mp2
    for m in (pyscf.mp, gpu4pyscf.mp):
        assert m.MP2 is mp2.MP2 and m.RMP2 is mp2.MP2 and m.UMP2 is mp2.MP2 and m.mp2.MP2 is mp2.MP2
    assert mp2.MP2.algorithm == "stream" and mp2.MP2.occ_batch is None
    assert mp2.T2_MAX_BYTES >= 8 * 110 ** 4                   # every N <= 220 molecule keeps its amplitudes
