"""CPU test of the XC quadrature's launch sequence: one pass of the RKS quadrature, of the UKS quadrature and of the TDDFT
spin potential `_vxc_alpha` over a recording stub engine must issue the recorded engine calls, in order, with the recorded
shapes.  The padded low-rank factor of UKS is not an engine call; its reuse between cycles is asserted on its own."""
import types

import pytest
import torch

NAO, NPTS = 10, 1600          # grid_block = 1024 and no byte budget: both block rules cut 1600 points into 1024 + 576
XC = {"lda": "LDA,VWN", "gga": "B3LYP", "mgga": "TPSS"}


def _shapes(args):
    out = []
    for a in args:
        if isinstance(a, torch.Tensor):
            out.append("x".join(map(str, a.shape)) or "s")
        elif isinstance(a, (tuple, list)):
            out += _shapes(a)
    return out


class RecordingEngine:
    """Engine stand-in: CPU tensors of the right shapes, and a log of `method shape shape ...` of the tensor arguments."""
    mol, device, NYSTROM_MAX_OCC = None, "cpu", 64

    def __init__(self):
        self.nao, self.log, self.zps = NAO, [], []

    def _rec(self, name, *args):
        self.log.append(" ".join([name] + _shapes(args)))

    @staticmethod
    def _z(*shape):
        return torch.zeros(*shape, dtype=torch.float64)

    def eval_ao(self, coords, deriv=1, out=None):
        self._rec("eval_ao", coords)
        return self._z({0: 1, 1: 4, 2: 10}[int(deriv)], NAO, coords.shape[0])

    def xc_rho(self, ao, C, deriv=1, out=None):
        self._rec("xc_rho", ao, C)
        return self._z(4 if deriv else 1, ao.shape[-1])

    def xc_rho_lowrank(self, ao, Zp, deriv=1, with_tau=False):
        self._rec("xc_rho_lowrank", ao, Zp)
        self.zps.append(Zp)
        rho = self._z(4 if deriv else 1, ao.shape[-1])
        return (rho, self._z(ao.shape[-1])) if with_tau else rho

    def xc_tau(self, ao, dm):
        self._rec("xc_tau", ao, dm)
        return self._z(ao.shape[-1])

    def xc_eval(self, terms, rho, weights, gga=True, want_raw=False, params=None):
        self._rec("xc_eval", rho, weights)
        return self._z(rho.shape[-1]), self._z(4 if gga else 1, rho.shape[-1])

    def xc_eval_spin(self, terms, rhoa, rhob, weights, gga=True, params=None):
        self._rec("xc_eval_spin", rhoa, rhob, weights)
        ng = rhoa.shape[-1]
        return self._z(ng), self._z(4 if gga else 1, ng), self._z(4 if gga else 1, ng)

    def xc_eval_mgga(self, terms, rho, tau, weights):
        self._rec("xc_eval_mgga", rho, tau, weights)
        return self._z(rho.shape[-1]), self._z(5, rho.shape[-1])

    def xc_eval_mgga_spin(self, terms, rhoa, rhob, taua, taub, weights):
        self._rec("xc_eval_mgga_spin", rhoa, rhob, taua, taub, weights)
        ng = rhoa.shape[-1]
        return self._z(ng), self._z(5, ng), self._z(5, ng)

    def xc_tail(self, w, vals, tail):
        self._rec("xc_tail", w, vals, tail)

    def xc_aow(self, ao, wv, gga=True):
        self._rec("xc_aow", ao, wv)
        return self._z(NAO, ao.shape[-1])

    def xc_vmat(self, ao0, aow, vmat):
        self._rec("xc_vmat", ao0, aow, vmat)

    def xc_vmat_fold(self, ao, wv, gga, vmat):
        self._rec("xc_vmat_fold", ao, wv, vmat)

    def nystrom_factor(self, M, W, Zt=None, info=None):
        self._rec("nystrom_factor", M, W)
        return torch.ones(W.shape[1], W.shape[0], dtype=torch.float64), torch.zeros((), dtype=torch.int32)

    def nystrom_warm(self, Zt, info, G0, G):
        self._rec("nystrom_warm", Zt, info, G0, G)
        return G


def _driver(cls, level, monkeypatch):
    for k in ("MI355_XC_BLOCK_GB", "MI355_VMAT_MT", "MI355_XC_FOLD"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setattr(torch.cuda, "mem_get_info", lambda device=None: (64e9, 288e9))
    mf = object.__new__(cls)
    mf.mol, mf._eng, mf._rank, mf._nranks = None, RecordingEngine(), 0, 1
    mf.xc, mf.grid_block, mf.xc_block_gb, mf.xc_lowrank_min_nao = XC[level], 1024, 0.0, 0
    mf.grids = types.SimpleNamespace(coords=torch.zeros(NPTS, 3, dtype=torch.float64),
                                     weights=torch.ones(NPTS, dtype=torch.float64), generation=1)
    mf._Linv = torch.eye(NAO, dtype=torch.float64)
    return mf


def _projector(nocc):
    x = torch.zeros(NAO, NAO, dtype=torch.float64)
    x[:nocc, :nocc] = torch.eye(nocc, dtype=torch.float64)
    return x


def _rks_pass(level, projector, fold, monkeypatch):
    from mi355scf.dft import RKS
    mf = _driver(RKS, level, monkeypatch)
    mf.xc_vmat_fold = fold
    dm = 2.0 * _projector(3)
    if projector:
        mf._xc_projector = (dm, dm, 3)
    mf.nr_rks(dm)
    return mf._eng.log


def _uks_driver(level, projector, monkeypatch, nocc=(3, 2)):
    from mi355scf.uks import UKS
    mf = _driver(UKS, level, monkeypatch)
    dm = torch.stack([_projector(nocc[0]), _projector(nocc[1])])
    if projector:
        mf._xc_projector_pair = (dm, [dm[0], dm[1]], nocc)
    return mf, dm


def _uks_pass(level, projector, monkeypatch):
    mf, dm = _uks_driver(level, projector, monkeypatch)
    mf.nr_uks(dm)
    return mf._eng.log


def _vxc_alpha_pass(level, monkeypatch):
    from mi355scf.dft import RKS
    from mi355scf.tdscf import _TDBase
    td = object.__new__(_TDBase)
    td._scf = _driver(RKS, level, monkeypatch)
    td._vxc_alpha(_projector(3), _projector(2))
    return td._scf._eng.log


_CASES = ([("rks", level, proj, fold) for level in XC for proj in (False, True) for fold in (False, True)]
          + [("uks", level, proj) for level in XC for proj in (False, True)]
          + [("vxc_alpha", level) for level in ("lda", "gga")])


def _run(case, monkeypatch):
    return {"rks": _rks_pass, "uks": _uks_pass, "vxc_alpha": _vxc_alpha_pass}[case[0]](*case[1:], monkeypatch)


# The engine calls of one pass over two blocks of 1024 and 576 points, as `method shape shape ...`.  Recorded by running the
# stub above against the commit before the block body, the XC-gradient loop and `_vxc_alpha` were moved onto the `KSMixin`
# helpers (as `_GRID_BLOCKS` of test_host_logic.py was recorded before the grid loops were merged), not derived from the
# code under test.  Keys: (driver, functional level, projector density declared[, xc_vmat_fold]).  `_vxc_alpha` belongs to
# TDDFT, which refuses meta-GGAs and never sees a projector density, so its passes are LDA and GGA over full densities.
_EXPECTED = {
    ("rks", "lda", False, False): [
        "eval_ao 1024x3", "xc_rho 1x10x1024 10x1024", "xc_eval 1x1024 1024", "xc_tail 1024 1024 1024 2",
        "xc_aow 1x10x1024 1x1024", "xc_vmat 10x1024 10x1024 10x10", "eval_ao 576x3", "xc_rho 1x10x576 10x576",
        "xc_eval 1x576 576", "xc_tail 576 576 576 2", "xc_aow 1x10x576 1x576", "xc_vmat 10x576 10x576 10x10",
    ],
    ("rks", "lda", False, True): [
        "eval_ao 1024x3", "xc_rho 1x10x1024 10x1024", "xc_eval 1x1024 1024", "xc_tail 1024 1024 1024 2",
        "xc_vmat_fold 1x10x1024 1x1024 10x10", "eval_ao 576x3", "xc_rho 1x10x576 10x576", "xc_eval 1x576 576",
        "xc_tail 576 576 576 2", "xc_vmat_fold 1x10x576 1x576 10x10",
    ],
    ("rks", "lda", True, False): [
        "nystrom_factor 3x3 10x3", "nystrom_warm 3x10 s 10x3 10x3", "eval_ao 1024x3", "xc_rho_lowrank 1x10x1024 10x32",
        "xc_eval 1x1024 1024", "xc_tail 1024 1024 1024 2", "xc_aow 1x10x1024 1x1024", "xc_vmat 10x1024 10x1024 10x10",
        "eval_ao 576x3", "xc_rho_lowrank 1x10x576 10x32", "xc_eval 1x576 576", "xc_tail 576 576 576 2", "xc_aow 1x10x576 1x576",
        "xc_vmat 10x576 10x576 10x10",
    ],
    ("rks", "lda", True, True): [
        "nystrom_factor 3x3 10x3", "nystrom_warm 3x10 s 10x3 10x3", "eval_ao 1024x3", "xc_rho_lowrank 1x10x1024 10x32",
        "xc_eval 1x1024 1024", "xc_tail 1024 1024 1024 2", "xc_vmat_fold 1x10x1024 1x1024 10x10", "eval_ao 576x3",
        "xc_rho_lowrank 1x10x576 10x32", "xc_eval 1x576 576", "xc_tail 576 576 576 2", "xc_vmat_fold 1x10x576 1x576 10x10",
    ],
    ("rks", "gga", False, False): [
        "eval_ao 1024x3", "xc_rho 4x10x1024 10x1024", "xc_eval 4x1024 1024", "xc_tail 1024 1024 1024 2",
        "xc_aow 4x10x1024 4x1024", "xc_vmat 10x1024 10x1024 10x10", "eval_ao 576x3", "xc_rho 4x10x576 10x576",
        "xc_eval 4x576 576", "xc_tail 576 576 576 2", "xc_aow 4x10x576 4x576", "xc_vmat 10x576 10x576 10x10",
    ],
    ("rks", "gga", False, True): [
        "eval_ao 1024x3", "xc_rho 4x10x1024 10x1024", "xc_eval 4x1024 1024", "xc_tail 1024 1024 1024 2",
        "xc_vmat_fold 4x10x1024 4x1024 10x10", "eval_ao 576x3", "xc_rho 4x10x576 10x576", "xc_eval 4x576 576",
        "xc_tail 576 576 576 2", "xc_vmat_fold 4x10x576 4x576 10x10",
    ],
    ("rks", "gga", True, False): [
        "nystrom_factor 3x3 10x3", "nystrom_warm 3x10 s 10x3 10x3", "eval_ao 1024x3", "xc_rho_lowrank 4x10x1024 10x24",
        "xc_eval 4x1024 1024", "xc_tail 1024 1024 1024 2", "xc_aow 4x10x1024 4x1024", "xc_vmat 10x1024 10x1024 10x10",
        "eval_ao 576x3", "xc_rho_lowrank 4x10x576 10x24", "xc_eval 4x576 576", "xc_tail 576 576 576 2", "xc_aow 4x10x576 4x576",
        "xc_vmat 10x576 10x576 10x10",
    ],
    ("rks", "gga", True, True): [
        "nystrom_factor 3x3 10x3", "nystrom_warm 3x10 s 10x3 10x3", "eval_ao 1024x3", "xc_rho_lowrank 4x10x1024 10x24",
        "xc_eval 4x1024 1024", "xc_tail 1024 1024 1024 2", "xc_vmat_fold 4x10x1024 4x1024 10x10", "eval_ao 576x3",
        "xc_rho_lowrank 4x10x576 10x24", "xc_eval 4x576 576", "xc_tail 576 576 576 2", "xc_vmat_fold 4x10x576 4x576 10x10",
    ],
    ("rks", "mgga", False, False): [
        "eval_ao 1024x3", "xc_rho 4x10x1024 10x1024", "xc_tau 4x10x1024 10x10", "xc_eval_mgga 4x1024 1024 1024",
        "xc_tail 1024 1024 1024 2", "xc_aow 4x10x1024 5x1024", "xc_vmat 10x1024 10x1024 10x10", "xc_vmat 10x1024 10x1024 10x10",
        "xc_vmat 10x1024 10x1024 10x10", "xc_vmat 10x1024 10x1024 10x10", "eval_ao 576x3", "xc_rho 4x10x576 10x576",
        "xc_tau 4x10x576 10x10", "xc_eval_mgga 4x576 576 576", "xc_tail 576 576 576 2", "xc_aow 4x10x576 5x576",
        "xc_vmat 10x576 10x576 10x10", "xc_vmat 10x576 10x576 10x10", "xc_vmat 10x576 10x576 10x10",
        "xc_vmat 10x576 10x576 10x10",
    ],
    ("rks", "mgga", False, True): [
        "eval_ao 1024x3", "xc_rho 4x10x1024 10x1024", "xc_tau 4x10x1024 10x10", "xc_eval_mgga 4x1024 1024 1024",
        "xc_tail 1024 1024 1024 2", "xc_vmat_fold 4x10x1024 5x1024 10x10", "xc_vmat 10x1024 10x1024 10x10",
        "xc_vmat 10x1024 10x1024 10x10", "xc_vmat 10x1024 10x1024 10x10", "eval_ao 576x3", "xc_rho 4x10x576 10x576",
        "xc_tau 4x10x576 10x10", "xc_eval_mgga 4x576 576 576", "xc_tail 576 576 576 2", "xc_vmat_fold 4x10x576 5x576 10x10",
        "xc_vmat 10x576 10x576 10x10", "xc_vmat 10x576 10x576 10x10", "xc_vmat 10x576 10x576 10x10",
    ],
    ("rks", "mgga", True, False): [
        "nystrom_factor 3x3 10x3", "nystrom_warm 3x10 s 10x3 10x3", "eval_ao 1024x3", "xc_rho_lowrank 4x10x1024 10x24",
        "xc_eval_mgga 4x1024 1024 1024", "xc_tail 1024 1024 1024 2", "xc_aow 4x10x1024 5x1024", "xc_vmat 10x1024 10x1024 10x10",
        "xc_vmat 10x1024 10x1024 10x10", "xc_vmat 10x1024 10x1024 10x10", "xc_vmat 10x1024 10x1024 10x10", "eval_ao 576x3",
        "xc_rho_lowrank 4x10x576 10x24", "xc_eval_mgga 4x576 576 576", "xc_tail 576 576 576 2", "xc_aow 4x10x576 5x576",
        "xc_vmat 10x576 10x576 10x10", "xc_vmat 10x576 10x576 10x10", "xc_vmat 10x576 10x576 10x10",
        "xc_vmat 10x576 10x576 10x10",
    ],
    ("rks", "mgga", True, True): [
        "nystrom_factor 3x3 10x3", "nystrom_warm 3x10 s 10x3 10x3", "eval_ao 1024x3", "xc_rho_lowrank 4x10x1024 10x24",
        "xc_eval_mgga 4x1024 1024 1024", "xc_tail 1024 1024 1024 2", "xc_vmat_fold 4x10x1024 5x1024 10x10",
        "xc_vmat 10x1024 10x1024 10x10", "xc_vmat 10x1024 10x1024 10x10", "xc_vmat 10x1024 10x1024 10x10", "eval_ao 576x3",
        "xc_rho_lowrank 4x10x576 10x24", "xc_eval_mgga 4x576 576 576", "xc_tail 576 576 576 2",
        "xc_vmat_fold 4x10x576 5x576 10x10", "xc_vmat 10x576 10x576 10x10", "xc_vmat 10x576 10x576 10x10",
        "xc_vmat 10x576 10x576 10x10",
    ],
    ("uks", "lda", False): [
        "eval_ao 1024x3", "xc_rho 1x10x1024 10x1024", "xc_rho 1x10x1024 10x1024", "xc_eval_spin 1x1024 1x1024 1024",
        "xc_tail 1024 1024 1024 1024 3", "xc_aow 1x10x1024 1x1024", "xc_vmat 10x1024 10x1024 10x10", "xc_aow 1x10x1024 1x1024",
        "xc_vmat 10x1024 10x1024 10x10", "eval_ao 576x3", "xc_rho 1x10x576 10x576", "xc_rho 1x10x576 10x576",
        "xc_eval_spin 1x576 1x576 576", "xc_tail 576 576 576 576 3", "xc_aow 1x10x576 1x576", "xc_vmat 10x576 10x576 10x10",
        "xc_aow 1x10x576 1x576", "xc_vmat 10x576 10x576 10x10",
    ],
    ("uks", "lda", True): [
        "nystrom_factor 3x3 10x3", "nystrom_warm 3x10 s 10x3 10x3", "nystrom_factor 2x2 10x2", "nystrom_warm 2x10 s 10x2 10x2",
        "eval_ao 1024x3", "xc_rho_lowrank 1x10x1024 10x32", "xc_rho_lowrank 1x10x1024 10x32", "xc_eval_spin 1x1024 1x1024 1024",
        "xc_tail 1024 1024 1024 1024 3", "xc_aow 1x10x1024 1x1024", "xc_vmat 10x1024 10x1024 10x10", "xc_aow 1x10x1024 1x1024",
        "xc_vmat 10x1024 10x1024 10x10", "eval_ao 576x3", "xc_rho_lowrank 1x10x576 10x32", "xc_rho_lowrank 1x10x576 10x32",
        "xc_eval_spin 1x576 1x576 576", "xc_tail 576 576 576 576 3", "xc_aow 1x10x576 1x576", "xc_vmat 10x576 10x576 10x10",
        "xc_aow 1x10x576 1x576", "xc_vmat 10x576 10x576 10x10",
    ],
    ("uks", "gga", False): [
        "eval_ao 1024x3", "xc_rho 4x10x1024 10x1024", "xc_rho 4x10x1024 10x1024", "xc_eval_spin 4x1024 4x1024 1024",
        "xc_tail 1024 1024 1024 1024 3", "xc_aow 4x10x1024 4x1024", "xc_vmat 10x1024 10x1024 10x10", "xc_aow 4x10x1024 4x1024",
        "xc_vmat 10x1024 10x1024 10x10", "eval_ao 576x3", "xc_rho 4x10x576 10x576", "xc_rho 4x10x576 10x576",
        "xc_eval_spin 4x576 4x576 576", "xc_tail 576 576 576 576 3", "xc_aow 4x10x576 4x576", "xc_vmat 10x576 10x576 10x10",
        "xc_aow 4x10x576 4x576", "xc_vmat 10x576 10x576 10x10",
    ],
    ("uks", "gga", True): [
        "nystrom_factor 3x3 10x3", "nystrom_warm 3x10 s 10x3 10x3", "nystrom_factor 2x2 10x2", "nystrom_warm 2x10 s 10x2 10x2",
        "eval_ao 1024x3", "xc_rho_lowrank 4x10x1024 10x24", "xc_rho_lowrank 4x10x1024 10x24", "xc_eval_spin 4x1024 4x1024 1024",
        "xc_tail 1024 1024 1024 1024 3", "xc_aow 4x10x1024 4x1024", "xc_vmat 10x1024 10x1024 10x10", "xc_aow 4x10x1024 4x1024",
        "xc_vmat 10x1024 10x1024 10x10", "eval_ao 576x3", "xc_rho_lowrank 4x10x576 10x24", "xc_rho_lowrank 4x10x576 10x24",
        "xc_eval_spin 4x576 4x576 576", "xc_tail 576 576 576 576 3", "xc_aow 4x10x576 4x576", "xc_vmat 10x576 10x576 10x10",
        "xc_aow 4x10x576 4x576", "xc_vmat 10x576 10x576 10x10",
    ],
    ("uks", "mgga", False): [
        "eval_ao 1024x3", "xc_rho 4x10x1024 10x1024", "xc_tau 4x10x1024 10x10", "xc_rho 4x10x1024 10x1024",
        "xc_tau 4x10x1024 10x10", "xc_eval_mgga_spin 4x1024 4x1024 1024 1024 1024", "xc_tail 1024 1024 1024 1024 3",
        "xc_aow 4x10x1024 5x1024", "xc_vmat 10x1024 10x1024 10x10", "xc_vmat 10x1024 10x1024 10x10",
        "xc_vmat 10x1024 10x1024 10x10", "xc_vmat 10x1024 10x1024 10x10", "xc_aow 4x10x1024 5x1024",
        "xc_vmat 10x1024 10x1024 10x10", "xc_vmat 10x1024 10x1024 10x10", "xc_vmat 10x1024 10x1024 10x10",
        "xc_vmat 10x1024 10x1024 10x10", "eval_ao 576x3", "xc_rho 4x10x576 10x576", "xc_tau 4x10x576 10x10",
        "xc_rho 4x10x576 10x576", "xc_tau 4x10x576 10x10", "xc_eval_mgga_spin 4x576 4x576 576 576 576",
        "xc_tail 576 576 576 576 3", "xc_aow 4x10x576 5x576", "xc_vmat 10x576 10x576 10x10", "xc_vmat 10x576 10x576 10x10",
        "xc_vmat 10x576 10x576 10x10", "xc_vmat 10x576 10x576 10x10", "xc_aow 4x10x576 5x576", "xc_vmat 10x576 10x576 10x10",
        "xc_vmat 10x576 10x576 10x10", "xc_vmat 10x576 10x576 10x10", "xc_vmat 10x576 10x576 10x10",
    ],
    ("uks", "mgga", True): [
        "nystrom_factor 3x3 10x3", "nystrom_warm 3x10 s 10x3 10x3", "nystrom_factor 2x2 10x2", "nystrom_warm 2x10 s 10x2 10x2",
        "eval_ao 1024x3", "xc_rho_lowrank 4x10x1024 10x24", "xc_rho_lowrank 4x10x1024 10x24",
        "xc_eval_mgga_spin 4x1024 4x1024 1024 1024 1024", "xc_tail 1024 1024 1024 1024 3", "xc_aow 4x10x1024 5x1024",
        "xc_vmat 10x1024 10x1024 10x10", "xc_vmat 10x1024 10x1024 10x10", "xc_vmat 10x1024 10x1024 10x10",
        "xc_vmat 10x1024 10x1024 10x10", "xc_aow 4x10x1024 5x1024", "xc_vmat 10x1024 10x1024 10x10",
        "xc_vmat 10x1024 10x1024 10x10", "xc_vmat 10x1024 10x1024 10x10", "xc_vmat 10x1024 10x1024 10x10", "eval_ao 576x3",
        "xc_rho_lowrank 4x10x576 10x24", "xc_rho_lowrank 4x10x576 10x24", "xc_eval_mgga_spin 4x576 4x576 576 576 576",
        "xc_tail 576 576 576 576 3", "xc_aow 4x10x576 5x576", "xc_vmat 10x576 10x576 10x10", "xc_vmat 10x576 10x576 10x10",
        "xc_vmat 10x576 10x576 10x10", "xc_vmat 10x576 10x576 10x10", "xc_aow 4x10x576 5x576", "xc_vmat 10x576 10x576 10x10",
        "xc_vmat 10x576 10x576 10x10", "xc_vmat 10x576 10x576 10x10", "xc_vmat 10x576 10x576 10x10",
    ],
    ("vxc_alpha", "lda"): [
        "eval_ao 1024x3", "xc_rho 1x10x1024 10x1024", "xc_rho 1x10x1024 10x1024", "xc_eval_spin 1x1024 1x1024 1024",
        "xc_aow 1x10x1024 1x1024", "xc_vmat 10x1024 10x1024 10x10", "eval_ao 576x3", "xc_rho 1x10x576 10x576",
        "xc_rho 1x10x576 10x576", "xc_eval_spin 1x576 1x576 576", "xc_aow 1x10x576 1x576", "xc_vmat 10x576 10x576 10x10",
    ],
    ("vxc_alpha", "gga"): [
        "eval_ao 1024x3", "xc_rho 4x10x1024 10x1024", "xc_rho 4x10x1024 10x1024", "xc_eval_spin 4x1024 4x1024 1024",
        "xc_aow 4x10x1024 4x1024", "xc_vmat 10x1024 10x1024 10x10", "eval_ao 576x3", "xc_rho 4x10x576 10x576",
        "xc_rho 4x10x576 10x576", "xc_eval_spin 4x576 4x576 576", "xc_aow 4x10x576 4x576", "xc_vmat 10x576 10x576 10x10",
    ],
}


@pytest.mark.parametrize("case", _CASES, ids=lambda c: "-".join(map(str, c)))
def test_xc_quadrature_issues_the_recorded_engine_calls(case, monkeypatch):
    assert _run(case, monkeypatch) == _EXPECTED[case]


@pytest.mark.parametrize("level", list(XC))
def test_uks_padded_factor_is_kept_between_cycles(level, monkeypatch):
    """The zero-padded factor of each spin is one buffer per spin that a second pass with the same occupied counts fills
    again; a changed count makes new buffers (the columns behind the old count would keep stale orbitals)."""
    mf, dm = _uks_driver(level, True, monkeypatch)
    mf.nr_uks(dm)
    first = list(mf._eng.zps[:2])
    assert first[0] is not first[1] and mf._eng.zps[2] is first[0] and mf._eng.zps[3] is first[1]   # both blocks, one buffer
    del mf._eng.zps[:]
    mf.nr_uks(dm)
    assert mf._eng.zps[0] is first[0] and mf._eng.zps[1] is first[1]
    dm2 = torch.stack([_projector(4), _projector(1)])
    mf._xc_projector_pair = (dm2, [dm2[0], dm2[1]], (4, 1))
    del mf._eng.zps[:]
    mf.nr_uks(dm2)
    assert mf._eng.zps[0] is not first[0] and mf._eng.zps[1] is not first[1]
    assert mf._eng.zps[0].shape == first[0].shape           # same padded shape: only the count tells them apart
