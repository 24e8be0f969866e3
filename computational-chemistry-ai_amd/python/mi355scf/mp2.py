"""Second-order Moller-Plesset correlation energy behind `pyscf.mp.MP2(mf).kernel()` / `gpu4pyscf.mp.MP2(mf).kernel()`
(`templates/calculate_energy.py:117-141`, `templates/calculate_interaction.py:19,116-120`; `mp.MP2` dispatches on the
reference: RHF -> RMP2, UHF -> UMP2).

`algorithm = "stream"` (default): conventional (not density-fitted) MP2 for any molecule whose ERI tile store is resident
and unsharded.  For each batch O of active occupied orbitals

    (oa|jb) for ALL active occupied j       `ao2mo.transform`: one pass over the resident tiles per 8 orbitals, three FP64 GEMMs
    E += sum_ajb (oa|jb) [2 (oa|jb) - (ob|ja)] / (e_o + e_j - e_a - e_b)

needs only integrals of the batch's own o, so batches are independent and nothing of size N^4 exists.  Memory per orbital
of a batch: the transformation's work space (`ao2mo.qtrans_work_bytes`) plus the amplitude-sized temporaries of the energy
step; the batch size is the largest that fits in 80 % of the free HBM beside the store (`ao2mo.plan_qtrans_batch`;
`occ_batch` overrides it).  UMP2 runs alpha batches (alpha-alpha and alpha-beta energies from one Y) and beta batches (beta-beta).

`algorithm = "dense"`: the earlier path, kept as the cross-check -- the tiles are unpacked to a dense (ij|kl) tensor
(`mi_eri_unpack`, 8 N^4 bytes, N <= 220) and transformed with torch contractions.

`frozen` [PySCF's convention, written from memory]: None / 0 = all orbitals correlated; an int n = the n lowest orbitals
are frozen; a list of MO indices = those orbitals (occupied or virtual) are left out.  UMP2 takes an int or a pair of lists
(alpha, beta).  `e_corr_os` / `e_corr_ss` are the opposite- and same-spin parts (`e_corr` is their sum; no scaling applied).
`t2` (RMP2 only, layout [i, a, j, b] = (ia|jb) / D_iajb) is kept while it is below `T2_MAX_BYTES`, else None.  No density
fitting: a density-fitted reference is correlated with the exact four-centre integrals.
"""
import time

import numpy as np
import torch

from .ao2mo import active_mask as _active, plan_qtrans_batch, qtrans_work_bytes, resident_engine, transform
from .reference import require

MAX_NAO = 220   # dense path: 8 * 220^4 = 18.7 GB tensor
T2_MAX_BYTES = 8 * (MAX_NAO // 2) ** 4   # 1.17 GB: the largest n_occ^2 n_vir^2 amplitude tensor of any N <= MAX_NAO basis


class MP2:
    algorithm = "stream"    # "stream" | "dense"
    occ_batch = None        # occupied orbitals per batch of the streaming path (None: from free HBM)

    def __init__(self, mf, frozen=None):
        require(mf, "MP2")
        self._scf = mf
        self.mol = mf.mol
        self.verbose = mf.verbose
        self.frozen = frozen
        self.e_corr = None
        self.e_corr_os = None
        self.e_corr_ss = None
        self.t2 = None
        self.timing = {}

    @property
    def e_tot(self):
        return self._scf.e_tot + self.e_corr

    # ---- orbital spaces -------------------------------------------------------------------------------------------------------
    def _spaces(self, mo_c, mo_e, occ):
        """[(C_occ, C_vir, e_occ, e_vir)] per spin (one entry: restricted) of the active orbitals, as device tensors."""
        dev = self._scf.engine.device
        T = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64, device=dev)
        if mo_c.ndim == 2:
            if self.frozen is not None and not isinstance(self.frozen, (int, np.integer)) and len(self.frozen) == 2 \
                    and all(hasattr(f, "__len__") for f in self.frozen):
                raise ValueError("frozen: a pair of lists belongs to an unrestricted reference")
            act = [_active(self.frozen, mo_c.shape[1])]
            mo_c, mo_e, occ = mo_c[None], mo_e[None], occ[None]
        else:
            fz = self.frozen
            if fz is None or isinstance(fz, (int, np.integer)):
                fz = (fz, fz)
            elif not (len(fz) == 2 and all(hasattr(f, "__len__") for f in fz)):
                raise ValueError("frozen (UMP2): an int or a pair of index lists (alpha, beta)")
            act = [_active(fz[s_], mo_c.shape[2]) for s_ in range(2)]
        out = []
        for s_ in range(len(act)):
            o, v = (occ[s_] > 0) & act[s_], (occ[s_] == 0) & act[s_]
            out.append((T(mo_c[s_][:, o]), T(mo_c[s_][:, v]), T(mo_e[s_][o]), T(mo_e[s_][v])))
        return out

    # ---- dense path (N <= MAX_NAO) --------------------------------------------------------------------------------------------
    def _ovov(self, eri, co, cv):
        # (ia|jb) = sum_pqrs C_pi C_qa (pq|rs) C_rj C_sb, one index at a time
        t = torch.einsum("pqrs,pi->iqrs", eri, co)
        t = torch.einsum("iqrs,qa->iars", t, cv)
        return t

    def _kernel_dense(self, spaces):
        eng = self._scf.engine
        if eng.nao > MAX_NAO:
            raise NotImplementedError(f"dense MP2 needs the dense ERI tensor: N_ao = {eng.nao} > {MAX_NAO}")
        eri = eng.eri_dense()
        t2 = None
        if len(spaces) == 1:      # restricted
            co, cv, eo, ev = spaces[0]
            iars = self._ovov(eri, co, cv)
            ovov = torch.einsum("iars,rj,sb->iajb", iars, co, cv)
            d = eo[:, None, None, None] - ev[None, :, None, None] + eo[None, None, :, None] - ev[None, None, None, :]
            t2 = ovov / d
            e = float(torch.sum(t2 * (2.0 * ovov - ovov.transpose(1, 3))))
            e_os = float(torch.sum(t2 * ovov))
            e_ss = e - e_os
        else:                     # unrestricted: aa, bb (antisymmetrised) and ab
            e_ss = 0.0
            for s_ in range(2):
                co, cv, eo, ev = spaces[s_]
                if co.shape[1] == 0:
                    continue
                ovov = torch.einsum("iars,rj,sb->iajb", self._ovov(eri, co, cv), co, cv)
                d = eo[:, None, None, None] - ev[None, :, None, None] + eo[None, None, :, None] - ev[None, None, None, :]
                anti = ovov - ovov.transpose(1, 3)
                e_ss += 0.25 * float(torch.sum(anti * anti / d))
            (coa, cva, eoa, eva), (cob, cvb, eob, evb) = spaces
            e_os = 0.0
            if cob.shape[1] > 0:
                ovov = torch.einsum("iars,rj,sb->iajb", self._ovov(eri, coa, cva), cob, cvb)
                d = eoa[:, None, None, None] - eva[None, :, None, None] + eob[None, None, :, None] - evb[None, None, None, :]
                e_os = float(torch.sum(ovov * ovov / d))
            e = e_ss + e_os
        del eri
        return e, e_os, e_ss, t2

    # ---- streaming path -------------------------------------------------------------------------------------------------------
    def _plan_batch(self, nocc, nvir):
        """Occupied orbitals per batch: what fits in 80 % of the free HBM (see the module docstring), at most `nocc`."""
        eng = self._scf.engine
        n = eng.nao
        per_orb = qtrans_work_bytes(n, nvir) + 8.0 * 6 * nvir * max(nocc, 1) * max(nvir, n)
        nb, free = plan_qtrans_batch(eng, nocc, per_orb, forced=self.occ_batch)
        if nb < 1:
            raise MemoryError(f"MP2: one occupied orbital needs {per_orb * 1e-9:.1f} GB of work space (Y[N^3], accumulator, "
                              f"first GEMM), {free * 1e-9:.1f} GB of HBM are free beside the ERI store")
        self._scf._log(4, f"MP2: occupied batch {nb} of {nocc}: {per_orb * nb * 1e-9:.2f} GB of work space, " +
                          ("set by occ_batch" if free is None else f"{free * 1e-9:.1f} GB of HBM free"))
        return nb

    def _kernel_stream(self, spaces):
        mf = self._scf
        eng = mf.engine
        dev = eng.device
        self.timing.update(qtrans_seconds=0.0, gemm_seconds=0.0, energy_seconds=0.0, passes=0)
        zero = lambda: torch.zeros((), dtype=torch.float64, device=dev)

        def denom(eo_b, ev, eo2, ev2):
            return eo_b[:, None, None, None] - ev[None, :, None, None] + eo2[None, None, :, None] - ev2[None, None, None, :]

        t2 = None
        if len(spaces) == 1:      # restricted
            co, cv, eo, ev = spaces[0]
            no, nv = co.shape[1], cv.shape[1]
            e_os, e_ss = zero(), zero()
            if no and nv:
                keep = 8 * no * no * nv * nv <= T2_MAX_BYTES
                if keep:
                    t2 = torch.empty((no, nv, no, nv), dtype=torch.float64, device=dev)
                else:
                    mf._log(3, f"MP2: t2 ({8e-9 * no * no * nv * nv:.1f} GB) exceeds {T2_MAX_BYTES * 1e-9:.2f} GB and is not kept")
                nb = self._plan_batch(no, nv)
                for o0 in range(0, no, nb):
                    sl = slice(o0, min(o0 + nb, no))
                    ovov, = transform(eng, co[:, sl], cv, [(co, cv)], self.timing)
                    t0 = time.perf_counter()
                    t = ovov / denom(eo[sl], ev, eo, ev)
                    e_os += torch.sum(t * ovov)
                    e_ss += torch.sum(t * (ovov - ovov.transpose(1, 3)))
                    if keep:
                        t2[sl] = t
                    del t, ovov
                    torch.cuda.synchronize(dev)
                    self.timing["energy_seconds"] += time.perf_counter() - t0
            else:
                t2 = torch.empty((no, nv, no, nv), dtype=torch.float64, device=dev)
        else:                     # unrestricted: alpha batches give aa and ab, beta batches give bb
            e_os, e_ss = zero(), zero()
            for s_ in range(2):
                co, cv, eo, ev = spaces[s_]
                no, nv = co.shape[1], cv.shape[1]
                if no == 0 or nv == 0:
                    continue
                targets = [(co, cv)]
                cob, cvb, eob, evb = spaces[1]
                mixed = s_ == 0 and cob.shape[1] > 0 and cvb.shape[1] > 0
                if mixed:
                    targets.append((cob, cvb))
                nb = self._plan_batch(no, max(nv, cvb.shape[1]))
                for o0 in range(0, no, nb):
                    sl = slice(o0, min(o0 + nb, no))
                    res = transform(eng, co[:, sl], cv, targets, self.timing)
                    t0 = time.perf_counter()
                    ovov = res[0]
                    anti = ovov - ovov.transpose(1, 3)
                    e_ss += 0.5 * torch.sum(ovov * anti / denom(eo[sl], ev, eo, ev))
                    if mixed:
                        e_os += torch.sum(res[1] * res[1] / denom(eo[sl], ev, eob, evb))
                    del res, ovov, anti
                    torch.cuda.synchronize(dev)
                    self.timing["energy_seconds"] += time.perf_counter() - t0
        e_os, e_ss = float(e_os), float(e_ss)
        mf._log(4, "MP2 (stream): {passes} passes over the store {qtrans_seconds:.3f} s, GEMMs {gemm_seconds:.3f} s, "
                   "energy {energy_seconds:.3f} s".format(**self.timing))
        return e_os + e_ss, e_os, e_ss, t2

    def kernel(self, mo_energy=None, mo_coeff=None, **kw):
        mf = self._scf
        if mf.mo_coeff is None:
            mf.kernel()
        if self.algorithm not in ("stream", "dense"):
            raise ValueError(f"MP2.algorithm = {self.algorithm!r}: 'stream' or 'dense'")
        resident_engine(mf, "MP2")
        mo_c = np.asarray(mf.mo_coeff if mo_coeff is None else mo_coeff)
        mo_e = np.asarray(mf.mo_energy if mo_energy is None else mo_energy)
        occ = np.asarray(mf.mo_occ)
        spaces = self._spaces(mo_c, mo_e, occ)
        t0 = time.perf_counter()
        if self.algorithm == "dense":
            e, e_os, e_ss, t2 = self._kernel_dense(spaces)
        else:
            e, e_os, e_ss, t2 = self._kernel_stream(spaces)
        self.timing["kernel_seconds"] = time.perf_counter() - t0
        self.e_corr, self.e_corr_os, self.e_corr_ss = e, e_os, e_ss
        self.t2 = t2
        mf._log(3, f"E(MP2) = {mf.e_tot + e:.12g}  E_corr = {e:.12g}")
        return self.e_corr, self.t2


RMP2 = UMP2 = MP2
