"""Closed-shell CCSD and CCSD(T) behind `pyscf.cc.CCSD(mf)` / `gpu4pyscf.cc.CCSD(mf)` (the reference README's "adding a new
method": `mycc = cc.CCSD(mf); mycc.kernel(); et = mycc.ccsd_t(); return mycc.e_tot + et`) for a converged canonical RHF on one
GPU with the resident, unsharded ERI tile store.

Integrals.  The active MO space is transformed once per `kernel()`: `ao2mo.transform` in batches sized from free HBM
(`ao2mo.plan_qtrans_batch`) gives (pq|rs) over the active orbitals, `ao2mo.symmetrize8` restores the exact 8-fold symmetry (the
store is screened), and the blocks oooo, ovoo, oovv, ovov, ovvo, ovvv, vvvv stay on the device.  Everything is held in core: there is NO AO-direct
particle-particle ladder and NO vvvv-free algorithm here; a case whose integrals and work space exceed 80 % of the free HBM
beside the store is refused with NotImplementedError.

CCSD.  Spin-adapted closed-shell equations with one-particle (F, L) and two-particle (W_oooo, W_vvvv, W_voov, W_vovo)
intermediates, chemists' integrals, t1[i, a], t2[i, j, a, b] (DESIGN.md section 13 lists them).  The Fock matrix is taken as
diagonal: the reference's `mo_energy` on the diagonal, f_ov = 0 (canonical, converged RHF).  Contractions are torch FP64
einsum/matmul on the device; the amplitudes stay there as one stacked vector [t1 | t2]; DIIS extrapolates that vector on the
device.  `mi_cc_amp_update` does the whole elementwise tail of a cycle in one pass: division by the orbital-energy
denominators, new amplitudes, DIIS error vector, |dt|^2 and the correlation energy of the new amplitudes (fixed-order sums).

(T).  For batches of occupied triples i >= j >= k (weights 6 / 3 / 1 by the number of distinct orderings) twelve batched GEMMs
leave six raw cubes per triple, R_p = X(pi_p(i, j, k)) in its own index order,
    X(i, j, k)[a, b, c] = sum_d (ia|bd) t2[k, j, c, d] - sum_l (ia|lj) t2[l, k, b, c],
and `mi_cc_t_energy` does the rest (permutation sum W through LDS tiles, V = W + t1 (x) (jb|kc) terms, energy expression,
per-workgroup then fixed-order reduction into one number per triple); no v^3 permuted copy exists on that path.
`ccsd_t(algorithm="torch")` evaluates the same step with permute / add / elementwise torch ops as the cross-check.
`t_batch`: triples per launch (None: from free HBM).

Settings keep PySCF's names; the defaults (conv_tol 1e-7, conv_tol_normt 1e-5, max_cycle 50, diis_space 6, diis_start_cycle 0)
and the `frozen` convention (`ao2mo.active_mask`) are written from memory, not pinned against PySCF.

Not implemented (refused with NotImplementedError, never approximated): the references of row "CCSD" of `reference.SUPPORT`,
direct-mode references, frozen natural orbitals, gradients, lambda equations.
"""
import ctypes
import sys
import time

import numpy as np
import torch

from . import engine
from .ao2mo import (active_mask, free_hbm, plan_qtrans_batch, qtrans_work_bytes, resident_engine, symmetrize8,
                    transform)
from .reference import require

PERMS = ((0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0))     # lexicographic, as in csrc/cc_kernels.h
_Z_COEFF = (4.0, -2.0, -2.0, 1.0, 1.0, -2.0)                                   # identity, transpositions, 3-cycles


# ---- the CCSD equations (device-agnostic torch) ---------------------------------------------------------------------------------
def _numerators(t1, t2, E):
    """Right-hand sides (r1, r2) of t1 = r1 / D1, t2 = r2 / D2 for a diagonal Fock matrix with f_ov = 0."""
    ein = torch.einsum
    oooo, ovoo, oovv, ovov, ovvo, ovvv, vvvv = (E[k] for k in ("oooo", "ovoo", "oovv", "ovov", "ovvo", "ovvv", "vvvv"))
    tau = t2 + ein("ia,jb->ijab", t1, t1)
    L = 2.0 * ovov - ovov.transpose(1, 3)                        # 2 (kc|ld) - (kd|lc)
    Foo = ein("kcld,ilcd->ki", L, tau)
    Fvv = -ein("kcld,klad->ac", L, tau)
    Fov = ein("kcld,ld->kc", L, t1)
    Loo = Foo + 2.0 * ein("lcki,lc->ki", ovoo, t1) - ein("kcli,lc->ki", ovoo, t1)
    Lvv = Fvv + 2.0 * ein("kdac,kd->ac", ovvv, t1) - ein("kcad,kd->ac", ovvv, t1)

    r1 = ein("ac,ic->ia", Fvv, t1) - ein("ki,ka->ia", Foo, t1)
    r1 += 2.0 * ein("kc,kica->ia", Fov, t2) - ein("kc,ikca->ia", Fov, t2) + ein("kc,ic,ka->ia", Fov, t1, t1)
    r1 += 2.0 * ein("kcai,kc->ia", ovvo, t1) - ein("kiac,kc->ia", oovv, t1)
    r1 += 2.0 * ein("kdac,ikcd->ia", ovvv, tau) - ein("kcad,ikcd->ia", ovvv, tau)
    r1 += -2.0 * ein("lcki,klac->ia", ovoo, tau) + ein("kcli,klac->ia", ovoo, tau)

    Woooo = ein("lcki,jc->klij", ovoo, t1) + ein("kclj,ic->klij", ovoo, t1) + ein("kcld,ijcd->klij", ovov, tau) + oooo.transpose(1, 2)
    Wvvvv = vvvv.transpose(1, 2) - ein("kdac,kb->abcd", ovvv, t1) - ein("kcbd,ka->abcd", ovvv, t1)
    Wvoov = ein("kcad,id->akic", ovvv, t1) - ein("kcli,la->akic", ovoo, t1) + ovvo.permute(2, 0, 3, 1)
    Wvoov += -0.5 * ein("ldkc,ilda->akic", ovov, t2) - 0.5 * ein("lckd,ilad->akic", ovov, t2) - ein("ldkc,id,la->akic", ovov, t1, t1) \
        + ein("ldkc,ilad->akic", ovov, t2)
    Wvovo = ein("kdac,id->akci", ovvv, t1) - ein("lcki,la->akci", ovoo, t1) + oovv.permute(2, 0, 3, 1)
    Wvovo += -0.5 * ein("lckd,ilda->akci", ovov, t2) - ein("lckd,id,la->akci", ovov, t1, t1)

    def sym(x):                                                  # x[i,j,a,b] + x[j,i,b,a]
        return x + x.permute(1, 0, 3, 2)

    r2 = ovov.permute(0, 2, 1, 3).clone()
    r2 += sym(ein("abic,jc->ijab", ovvv.permute(1, 3, 0, 2) - ein("kibc,ka->abic", oovv, t1), t1))
    r2 -= sym(ein("akij,kb->ijab", ovoo.permute(1, 3, 0, 2) + ein("kcai,jc->akij", ovvo, t1), t1))
    r2 += ein("klij,klab->ijab", Woooo, tau) + ein("abcd,ijcd->ijab", Wvvvv, tau)
    r2 += sym(ein("ac,ijcb->ijab", Lvv, t2)) - sym(ein("ki,kjab->ijab", Loo, t2))
    r2 += sym(2.0 * ein("akic,kjcb->ijab", Wvoov, t2) - ein("akci,kjcb->ijab", Wvovo, t2))
    r2 -= sym(ein("akic,kjbc->ijab", Wvoov, t2)) + sym(ein("bkci,kjac->ijab", Wvovo, t2))
    return r1, r2


def _energy(t1, t2, ovov):
    tau = t2 + torch.einsum("ia,jb->ijab", t1, t1)
    return float(torch.sum(tau * (2.0 * ovov.permute(0, 2, 1, 3) - ovov.permute(0, 2, 3, 1))))


# ---- (T): the GEMM stage and the plain-torch tail -------------------------------------------------------------------------------
def _triples(no):
    """(ijk [n, 3] int32, weights [n]) of all i >= j >= k; the weight is the number of distinct orderings."""
    ijk = np.array([(i, j, k) for i in range(no) for j in range(i + 1) for k in range(j + 1)], dtype=np.int32).reshape(-1, 3)
    nd = (ijk[:, 0] != ijk[:, 1]).astype(int) + (ijk[:, 1] != ijk[:, 2]).astype(int)
    return ijk, np.array([1.0, 3.0, 6.0])[nd]


def _t_operands(t2, E):
    """Operands of the (T) GEMMs in the layouts that need no per-triple transposition: (ia|bd) as [i][a b][d], (ia|lj) as
    [i][j][a][l], t2[l, k, b, c] as [k][l][b c]."""
    return dict(ovvv=E["ovvv"], oo=E["ovoo"].permute(0, 3, 1, 2).contiguous(), t2=t2, t2T=t2.transpose(0, 1).contiguous())


def _raw_cubes(ops, ijk, raw, gather):
    """raw[p, t] = X(pi_p(ijk[t])) for the triples `ijk` (a device int64 [T, 3]); `gather`: [T, v^3] work space."""
    T = ijk.shape[0]
    v = ops["t2"].shape[2]
    for p, perm in enumerate(PERMS):
        x, y, z = ijk[:, perm[0]], ijk[:, perm[1]], ijk[:, perm[2]]
        torch.index_select(ops["ovvv"].view(-1, v * v * v), 0, x, out=gather)
        out = raw[p]
        torch.bmm(gather.view(T, v * v, v), ops["t2"][z, y].transpose(1, 2), out=out.view(T, v * v, v))
        out.view(T, v, v * v).baddbmm_(ops["oo"][x, y], ops["t2T"][z].reshape(T, -1, v * v), alpha=-1.0)
    return raw


def _t_energy_torch(raw, ijk, wt, t1, ovov, eo, ev):
    """Per-triple (T) energies from the raw cubes with permute / add / elementwise torch ops (the cross-check of mi_cc_t_energy)."""
    inv = lambda p: tuple(int(q) for q in np.argsort(p))
    W = sum(raw[p].permute(0, *(1 + d for d in inv(perm))) for p, perm in enumerate(PERMS))
    i, j, k = ijk[:, 0], ijk[:, 1], ijk[:, 2]
    V = W + t1[i][:, :, None, None] * ovov[j, :, k, :][:, None, :, :] + t1[j][:, None, :, None] * ovov[i, :, k, :][:, :, None, :] \
        + t1[k][:, None, None, :] * ovov[i, :, j, :][:, :, :, None]
    Z = sum(c * W.permute(0, *(1 + d for d in perm)) for c, perm in zip(_Z_COEFF, PERMS))
    D = (eo[i] + eo[j] + eo[k])[:, None, None, None] - ev[None, :, None, None] - ev[None, None, :, None] - ev[None, None, None, :]
    return wt * torch.sum(Z * V / (3.0 * D), dim=(1, 2, 3))


def t_energy_native(raw, ijk32, wt, t1, ovov, eo, ev, check=True):
    """Per-triple (T) energies [T] from raw cubes [6, T, v, v, v] through `mi_cc_t_energy` (all device tensors, FP64 / int32).
    `check`: verify the occupied indices on the host first (a synchronisation; the driver's own triples skip it)."""
    _, T, v = raw.shape[:3]
    no = t1.shape[0]
    for x in (raw, ijk32, wt, t1, ovov, eo, ev):
        if not (x.is_cuda and x.is_contiguous()):
            raise ValueError("mi_cc_t_energy: contiguous device tensors are required")
    if raw.shape != (6, T, v, v, v) or ijk32.shape != (T, 3) or ijk32.dtype != torch.int32 or wt.shape != (T,) or t1.shape != (no, v) \
            or ovov.shape != (no, v, no, v) or eo.shape != (no,) or ev.shape != (v,):
        raise ValueError("mi_cc_t_energy: inconsistent shapes")
    if check and T and (int(ijk32.min()) < 0 or int(ijk32.max()) >= no):
        raise ValueError("mi_cc_t_energy: occupied index out of range")
    L = engine.lib()
    nblk = int(L.mi_cc_t_blocks(int(v)))
    part = torch.empty(T * nblk, dtype=torch.float64, device=raw.device)
    et = torch.empty(T, dtype=torch.float64, device=raw.device)
    if T:
        with torch.cuda.device(raw.device):
            stream = ctypes.c_void_p(torch.cuda.current_stream(raw.device).cuda_stream)
            engine._check(L.mi_cc_t_energy(raw.data_ptr(), T, v, no, ijk32.data_ptr(), wt.data_ptr(), t1.data_ptr(), ovov.data_ptr(),
                                           eo.data_ptr(), ev.data_ptr(), part.data_ptr(), et.data_ptr(), stream))
    return et


def amp_update_native(num, told, ovov, eo, ev):
    """(new amplitudes, error vector, |dt|^2, E_corr of the new amplitudes) from the stacked numerators through `mi_cc_amp_update`."""
    no, nv = eo.numel(), ev.numel()
    n = no * nv + (no * nv) ** 2
    for x in (num, told, ovov, eo, ev):
        if not (x.is_cuda and x.is_contiguous() and x.dtype == torch.float64):
            raise ValueError("mi_cc_amp_update: contiguous float64 device tensors are required")
    if num.numel() != n or told.numel() != n or ovov.shape != (no, nv, no, nv):
        raise ValueError("mi_cc_amp_update: inconsistent shapes")
    L = engine.lib()
    tnew, err = torch.empty_like(num), torch.empty_like(num)
    part = torch.empty(2 * int(L.mi_cc_amp_blocks()), dtype=torch.float64, device=num.device)
    out = torch.empty(2, dtype=torch.float64, device=num.device)
    with torch.cuda.device(num.device):
        stream = ctypes.c_void_p(torch.cuda.current_stream(num.device).cuda_stream)
        engine._check(L.mi_cc_amp_update(num.data_ptr(), told.data_ptr(), tnew.data_ptr(), err.data_ptr(), ovov.data_ptr(), eo.data_ptr(),
                                         ev.data_ptr(), no, nv, part.data_ptr(), out.data_ptr(), stream))
    dt2, e = out.cpu().tolist()
    return tnew, err, dt2, e


class _DIIS:
    """Pulay extrapolation of the stacked amplitude vector; vectors and error vectors stay on the device."""

    def __init__(self, space):
        self.space, self.x, self.e = int(space), [], []

    def update(self, x, err):
        self.x, self.e = (self.x + [x])[-self.space:], (self.e + [err])[-self.space:]
        m = len(self.x)
        if m < 2:
            return x
        Em = torch.stack(self.e)
        B = np.zeros((m + 1, m + 1))
        B[:m, :m] = (Em @ Em.T).cpu().numpy()
        B[m, :m] = B[:m, m] = 1.0
        rhs = np.zeros(m + 1)
        rhs[m] = 1.0
        c = np.linalg.lstsq(B, rhs, rcond=None)[0][:m]
        return torch.as_tensor(c, dtype=x.dtype, device=x.device) @ torch.stack(self.x)


class CCSD:
    conv_tol = 1e-7
    conv_tol_normt = 1e-5
    max_cycle = 50
    diis_space = 6
    diis_start_cycle = 0
    t_batch = None          # (T): occupied triples per launch (None: from free HBM)

    def __init__(self, mf, frozen=None):
        require(mf, "CCSD")
        self._scf = mf
        self.mol = mf.mol
        self.verbose = mf.verbose
        self.stdout = getattr(mf, "stdout", None)
        self.frozen = frozen
        self.e_hf = self.e_corr = self.emp2 = self.e_t = None
        self.t1 = self.t2 = None
        self.converged = False
        self.cycles = 0
        self.timing = {}
        self._eris = None

    def density_fit(self, *a, **kw):
        raise NotImplementedError("CCSD: density-fitted coupled cluster is not implemented")

    @property
    def e_tot(self):
        return None if self.e_corr is None else self.e_hf + self.e_corr

    def _log(self, level, msg):
        if self.verbose >= level:
            (self.stdout or sys.stdout).write(msg + "\n")

    # ---- integrals ------------------------------------------------------------------------------------------------------------
    def _spaces(self):
        mf = self._scf
        mo_c, mo_e, occ = np.asarray(mf.mo_coeff), np.asarray(mf.mo_energy), np.asarray(mf.mo_occ)
        if mo_c.ndim != 2:
            raise NotImplementedError("CCSD: UCCSD is not implemented (closed-shell RHF only)")
        act = active_mask(self.frozen, mo_c.shape[1])
        o, v = (occ > 0) & act, (occ == 0) & act
        if not o.any() or not v.any():
            raise ValueError(f"CCSD: {int(o.sum())} occupied and {int(v.sum())} virtual orbitals are correlated")
        return np.concatenate([mo_c[:, o], mo_c[:, v]], axis=1), mo_e[o], mo_e[v]

    @staticmethod
    def _need_bytes(no, nv, diis_space):
        """Peak device bytes of a CCSD run beside the store, the largest of three phases: the full active (pq|rs) with the two
        temporaries of its symmetrisation (3 n^4); (pq|rs) while the blocks are cut out of it; a cycle, i.e. the blocks, two
        vvvv-sized and six oovv-sized temporaries, the DIIS history and four more stacked vectors."""
        n, amp = no + nv, no * nv + (no * nv) ** 2
        blocks = no ** 4 + no ** 3 * nv + 3 * no ** 2 * nv ** 2 + no * nv ** 3 + nv ** 4
        return 8 * max(3 * n ** 4, n ** 4 + blocks, blocks + 2 * nv ** 4 + 6 * amp + (2 * diis_space + 4) * amp)

    def ao2mo(self):
        """The integral blocks of the active space on the device (a dict), the orbital energies and the work-space check."""
        mf = self._scf
        if mf.mo_coeff is None:
            mf.kernel()
        if not getattr(mf, "converged", True):
            self._log(2, "CCSD: the reference SCF is not converged (a canonical, converged RHF is assumed: f_ov = 0)")
        eng = resident_engine(mf, "CCSD")
        dev, N = eng.device, eng.nao
        C, eo, ev = self._spaces()
        no, nv = len(eo), len(ev)
        n = no + nv
        per_orb = qtrans_work_bytes(N, n)
        need = self._need_bytes(no, nv, self.diis_space)
        nb, free = plan_qtrans_batch(eng, n, per_orb, reserve_bytes=8 * n ** 4)
        if need + per_orb > 0.8 * free:      # `need` exceeds the reserve, so below this line at least one orbital fits
            raise NotImplementedError(f"CCSD: o = {no}, v = {nv} needs {(need + per_orb) * 1e-9:.1f} GB for the MO integrals and the work "
                                      f"space; {0.8 * free * 1e-9:.1f} GB (80 % of the free HBM beside the ERI store) are available")
        self._log(4, f"CCSD: o = {no}, v = {nv}; {need * 1e-9:.2f} GB of integrals and work space, qtrans batches of {nb} orbitals")
        t0 = time.perf_counter()
        Cd = torch.as_tensor(np.ascontiguousarray(C), dtype=torch.float64, device=dev)
        eri = torch.empty((n, n, n, n), dtype=torch.float64, device=dev)
        for p0 in range(0, n, nb):
            p1 = min(p0 + nb, n)
            eri[p0:p1] = transform(eng, Cd[:, p0:p1], Cd, [(Cd, Cd)])[0]
        eri = symmetrize8(eri)
        o, v = slice(0, no), slice(no, n)
        E = {k: eri[tuple(o if ch == "o" else v for ch in k)].contiguous() for k in ("oooo", "ovoo", "oovv", "ovov", "ovvo", "ovvv", "vvvv")}
        del eri
        E["eo"] = torch.as_tensor(eo, dtype=torch.float64, device=dev)
        E["ev"] = torch.as_tensor(ev, dtype=torch.float64, device=dev)
        torch.cuda.synchronize(dev)
        self.timing["ao2mo_seconds"] = time.perf_counter() - t0
        self._eris = E
        return E

    # ---- amplitudes -----------------------------------------------------------------------------------------------------------
    def _split(self, x, no, nv):
        return x[:no * nv].view(no, nv), x[no * nv:].view(no, no, nv, nv)

    def _stack(self, t1, t2, E):
        dev = E["eo"].device
        T = lambda a: torch.as_tensor(np.asarray(a), dtype=torch.float64, device=dev).reshape(-1)
        return torch.cat([T(t1), T(t2)]).contiguous()

    def _init_amps(self, E):
        no, nv = E["eo"].numel(), E["ev"].numel()
        num = torch.cat([torch.zeros(no * nv, dtype=torch.float64, device=E["eo"].device), E["ovov"].permute(0, 2, 1, 3).reshape(-1)])
        x, _err, _dt2, emp2 = amp_update_native(num.contiguous(), torch.zeros_like(num), E["ovov"], E["eo"], E["ev"])
        return emp2, x

    def init_amps(self, eris=None):
        """(E_MP2, t1, t2): the first-order amplitudes (t1 = 0 for a canonical reference)."""
        E = eris or self._eris or self.ao2mo()
        emp2, x = self._init_amps(E)
        t1, t2 = self._split(x, E["eo"].numel(), E["ev"].numel())
        self.emp2 = emp2
        return emp2, t1.cpu().numpy(), t2.cpu().numpy()

    def energy(self, t1=None, t2=None, eris=None):
        """Correlation energy of the amplitudes (default: the stored ones)."""
        E = eris or self._eris or self.ao2mo()
        x = self._stack(self.t1 if t1 is None else t1, self.t2 if t2 is None else t2, E)
        return _energy(*self._split(x, E["eo"].numel(), E["ev"].numel()), E["ovov"])

    def kernel(self, t1=None, t2=None, eris=None):
        mf = self._scf
        if mf.mo_coeff is None:
            mf.kernel()
        E = eris or self.ao2mo()
        no, nv = E["eo"].numel(), E["ev"].numel()
        self.e_hf = float(mf.e_tot)
        self.emp2, x = self._init_amps(E)
        if t1 is not None or t2 is not None:
            if t1 is None or t2 is None or np.shape(t1) != (no, nv) or np.shape(t2) != (no, no, nv, nv):
                raise ValueError(f"CCSD.kernel: t1 [{no}, {nv}] and t2 [{no}, {no}, {nv}, {nv}] are needed together")
            x = self._stack(t1, t2, E)
        e = self.emp2 if t1 is None else _energy(*self._split(x, no, nv), E["ovov"])
        self._log(4, f"CCSD: E(MP2) = {self.emp2:.12f}, initial E_corr = {e:.12f}")
        diis = _DIIS(self.diis_space)
        self.converged = False
        t0 = time.perf_counter()
        for cycle in range(1, self.max_cycle + 1):
            r1, r2 = _numerators(*self._split(x, no, nv), E)
            num = torch.cat([r1.reshape(-1), r2.reshape(-1)])
            del r1, r2
            xn, err, dt2, e_new = amp_update_native(num, x, E["ovov"], E["eo"], E["ev"])
            del num
            normt, de = float(np.sqrt(dt2)), e_new - e
            done = abs(de) < self.conv_tol and normt < self.conv_tol_normt
            if not done and cycle > self.diis_start_cycle and self.diis_space > 1:
                xn = diis.update(xn, err)
                e_new = _energy(*self._split(xn, no, nv), E["ovov"])
            x, e = xn.contiguous(), e_new
            self.cycles = cycle
            self._log(4, f"CCSD cycle {cycle:3d}: E_corr = {e:.12f}  dE = {de: .3e}  |dt| = {normt:.3e}")
            if done:
                self.converged = True
                break
        torch.cuda.synchronize(E["eo"].device)
        self.timing["cycle_seconds"] = (time.perf_counter() - t0) / max(self.cycles, 1)
        if not self.converged:
            self._log(2, f"CCSD: not converged in {self.max_cycle} cycles")
        t1d, t2d = self._split(x, no, nv)
        self.e_corr = e
        self.t1, self.t2 = t1d.cpu().numpy(), t2d.cpu().numpy()
        self._log(3, f"E(CCSD) = {self.e_tot:.12f}  E_corr = {e:.12f}")
        return self.e_corr, self.t1, self.t2

    ccsd = kernel

    # ---- (T) ------------------------------------------------------------------------------------------------------------------
    def _plan_triples(self, nv, ntrip, dev):
        if self.t_batch:
            return max(1, min(int(self.t_batch), ntrip))
        free = free_hbm(dev)
        per = 8.0 * (7 * nv ** 3 + nv * nv * 8)                  # six raw cubes, the gathered (ia|bd), small operands
        nb = int(0.5 * free // per)
        if nb < 1:
            raise NotImplementedError(f"CCSD(T): one occupied triple needs {per * 1e-9:.1f} GB of work space, {free * 1e-9:.1f} GB are free")
        return min(nb, ntrip, 65535)

    def ccsd_t(self, t1=None, t2=None, eris=None, algorithm="native"):
        """The perturbative triples correction E(T) (stored as `e_t`; `e_tot` is left alone)."""
        if algorithm not in ("native", "torch"):
            raise ValueError(f"ccsd_t: algorithm = {algorithm!r}: 'native' or 'torch'")
        if t1 is None and self.t1 is None:
            self.kernel()
        E = eris or self._eris or self.ao2mo()
        dev = E["eo"].device
        no, nv = E["eo"].numel(), E["ev"].numel()
        x = self._stack(self.t1 if t1 is None else t1, self.t2 if t2 is None else t2, E)
        t1d, t2d = (a.contiguous() for a in self._split(x, no, nv))
        ops = _t_operands(t2d, E)
        ijk, wt = _triples(no)
        nb = self._plan_triples(nv, len(ijk), dev)
        raw = torch.empty((6, nb, nv, nv, nv), dtype=torch.float64, device=dev)
        gather = torch.empty((nb, nv ** 3), dtype=torch.float64, device=dev)
        et = torch.empty(len(ijk), dtype=torch.float64, device=dev)
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        marks = []                                               # device events around the tail: no host wait inside the loop
        for b0 in range(0, len(ijk), nb):
            b1 = min(b0 + nb, len(ijk))
            T = b1 - b0
            idx = torch.as_tensor(ijk[b0:b1], device=dev)
            w = torch.as_tensor(wt[b0:b1], dtype=torch.float64, device=dev)
            r = raw[:, :T] if T == nb else torch.empty((6, T, nv, nv, nv), dtype=torch.float64, device=dev)
            _raw_cubes(ops, idx.long(), r, gather[:T])
            marks.append((torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)))
            marks[-1][0].record()
            if algorithm == "native":
                et[b0:b1] = t_energy_native(r, idx.contiguous(), w, t1d, E["ovov"], E["eo"], E["ev"], check=False)
            else:
                et[b0:b1] = _t_energy_torch(r, idx.long(), w, t1d, E["ovov"], E["eo"], E["ev"])
            marks[-1][1].record()
        et_host = et.cpu().numpy()                               # the one synchronisation
        self.timing["t_seconds"] = time.perf_counter() - t0
        tail = 1e-3 * sum(a.elapsed_time(b) for a, b in marks)
        self.timing["t_tail_seconds"] = tail
        self.timing["t_triples"], self.timing["t_batch"] = len(ijk), nb
        self.e_t = float(np.sum(et_host))                        # host sum in triple order: independent of the batching
        self._log(3, f"E(T) = {self.e_t:.12f}  ({len(ijk)} triples in batches of {nb}, tail {tail:.3f} s of {self.timing['t_seconds']:.3f} s)")
        return self.e_t


RCCSD = CCSD
