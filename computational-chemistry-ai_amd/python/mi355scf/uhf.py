"""Spin-unrestricted SCF behind `pyscf.scf.UHF` / `gpu4pyscf.scf.UHF` and `dft.UKS` (SURVEY.md section 8f
rank 4; call sites `templates/calculate_bde.py:126-128,138-140,189-215`: radicals with `mol.spin = 1`).

Same engine as RHF: both spin densities go through the resident-tile J/K kernel in one call
(`mi_build_jk(n_dm = 2)`; J = J[Da] + J[Db], K_s = K[D_s]), sharded runs all-reduce the [J|K] buffer once.
F_s = h + J - c_x K_s (+ V_xc,s for UKS), E = 1/2 sum_s tr D_s (h + F_s^HF) (+ E_xc).  CDIIS acts on the pair
(F_a, F_b) with the concatenated error vectors F_s D_s S - S D_s F_s; the orbitals of each spin come from one
`eigh` of the Cholesky-orthogonalised Fock matrix per cycle (aufbau occupation, n_alpha >= n_beta).
"""
import time

import numpy as np
import torch

from .purify import Purifier
from .scf import SCF, DeviceDIIS


def pulay_coefficients(B, m):
    """Coefficients c[:m] (sum 1) that minimise |sum_i c_i e_i| for the Gram matrix B[:m, :m] of the error vectors: the
    bordered Pulay system, by least squares when it is singular."""
    A = np.zeros((m + 1, m + 1))
    A[0, 1:] = A[1:, 0] = 1.0
    A[1:, 1:] = B[:m, :m]
    rhs = np.zeros(m + 1)
    rhs[0] = 1.0
    try:
        c = np.linalg.solve(A, rhs)
    except np.linalg.LinAlgError:
        c = np.linalg.lstsq(A, rhs, rcond=None)[0]
    return c[1:]


class PairDIIS:
    """Pulay CDIIS on stacked [2, N, N] Fock/error matrices: ring-buffer history on the device, only the new Gram row
    (one fused multiply-reduce; a K = 2 N^2 GEMM with 8x8 output is the shape rocBLAS runs at < 1 TFLOP/s) and the
    (m+1)x(m+1) solve touch the host."""

    def __init__(self, space=8, sync=None):
        self.space, self.count = space, 0
        self.F = self.E = None
        self.B = np.zeros((space, space))
        # sharded runs: rank 0's Gram row is used on every rank.  Replicated FP64 work (eigh, reductions) differs in the last
        # bits between ranks; extrapolation coefficients computed per rank would feed that difference back and amplify it
        # (measured: x8 per cycle) until the ranks' densities disagree at 1e-7.
        self.sync = sync

    def update(self, f, e):
        if self.F is None:
            self.F = torch.empty((self.space,) + tuple(f.shape), dtype=f.dtype, device=f.device)
            self.E = torch.empty_like(self.F)
        slot = self.count % self.space
        self.F[slot].copy_(f)
        self.E[slot].copy_(e)
        self.count += 1
        m = min(self.count, self.space)
        dots = (self.E[:m].reshape(m, -1) * e.reshape(1, -1)).sum(dim=1)
        if self.sync is not None:
            self.sync(dots)
        dots = dots.cpu().numpy()
        self.B[slot, :m] = dots
        self.B[:m, slot] = dots
        c = pulay_coefficients(self.B, m)
        cw = torch.as_tensor(c, dtype=f.dtype, device=f.device).reshape(m, 1, 1, 1)
        return (cw * self.F[:m]).sum(dim=0)


class UHF(SCF):
    _spin_restricted = False
    sp2_min_nao = 200   # below this a per-cycle `eigh` of each spin is cheaper than the purification
    _purify_spins = True   # the plain loop may purify each spin's Fock matrix instead of diagonalising it (ROHF: never)

    def __init__(self, mol):
        SCF.__init__(self, mol)
        self.nelec = mol.nelec

    # --- densities ------------------------------------------------------------------------------
    def make_rdm1(self, mo_coeff=None, mo_occ=None):
        if mo_coeff is None:
            if self._dm is not None:
                return self._dm.cpu().numpy()
            mo_coeff, mo_occ = self.mo_coeff, self.mo_occ
        out = []
        for c, o in zip(np.asarray(mo_coeff), np.asarray(mo_occ)):
            co = c[:, o > 0]
            out.append((co * o[o > 0]) @ co.T)
        return np.stack(out)

    def get_init_guess(self, mol=None, key=None):
        """Spin-restricted guess density split by electron count: D_s = D n_s / N (the first diagonalisation
        with n_alpha != n_beta occupations separates the spins)."""
        key = key if key is not None else self.init_guess
        if isinstance(key, np.ndarray) and key.ndim == 3:
            return key
        d = np.asarray(SCF.get_init_guess(self, mol, key))
        if d.ndim == 3:
            return d
        na, nb = self.nelec
        ne = max(na + nb, 1)
        return np.stack([d * (na / ne), d * (nb / ne)])

    # --- Fock pieces ----------------------------------------------------------------------------
    def _fock_pair(self, dm):
        """(F[2,N,N], E_elec) on device for the spin densities dm[2,N,N].  Overridden by UKS."""
        self.n_fock_builds = getattr(self, "n_fock_builds", 0) + 1
        J, K = self._jk(dm)
        Jt = J[0] + J[1]
        F = self._h1.unsqueeze(0) + Jt.unsqueeze(0) - K
        e = 0.5 * torch.sum(dm * (self._h1.unsqueeze(0) + F))
        return F, e

    def get_veff(self, mol=None, dm=None, **kw):
        if dm is None:
            dm = self.make_rdm1()
        self._setup_once()
        d = torch.as_tensor(np.asarray(dm), dtype=torch.float64, device=self.engine.device)
        F, _ = self._fock_pair(d)
        return (F - self._h1.unsqueeze(0)).cpu().numpy()

    def energy_tot(self, dm=None, h1e=None, vhf=None):
        if dm is None:
            return self.e_tot
        self._setup_once()
        d = torch.as_tensor(np.asarray(dm), dtype=torch.float64, device=self.engine.device)
        return float(self._fock_pair(d)[1]) + self.energy_nuc()

    def spin_square(self, mo_coeff=None, s=None):
        """<S^2> and 2S+1 of the UHF determinant: S_z(S_z+1) + n_beta - sum_ij |<i_a|j_b>|^2."""
        mo = np.asarray(self.mo_coeff if mo_coeff is None else mo_coeff)
        occ = np.asarray(self.mo_occ)
        S = self.get_ovlp() if s is None else s
        ca, cb = mo[0][:, occ[0] > 0], mo[1][:, occ[1] > 0]
        na, nb = ca.shape[1], cb.shape[1]
        sab = ca.T @ S @ cb
        sz = 0.5 * (na - nb)
        ss = sz * (sz + 1.0) + nb - float(np.sum(sab * sab))
        return ss, float(np.sqrt(4.0 * ss + 1.0))

    # --- SCF loop -------------------------------------------------------------------------------
    fast_loop = True   # orthonormal-basis loop with device-side pair DIIS, planned purification per spin, pipelined step

    def kernel(self, dm0=None, **kw):
        """Two loops.  The fast one (orthonormal basis, device-side pair DIIS, pipelined step, planned purification per spin
        when plans exist) is the default below `sp2_min_nao` basis functions, where both loops diagonalise per cycle and it is
        5-13 % faster (CH3/cc-pVTZ UHF 2.92 -> 2.54 ms per cycle, UKS B3LYP 2.99 -> 2.83).  Above that size it did not pay in
        the measurements of round 2 (`tools/uhf_bench.py`, `tools/uhf_warm.py`, benzene cation / cc-pVTZ): from a cold object it
        needs diagonalisations for its purification plans (7 ms each), and restarted from a nearby density it ran 2.15 against
        3.1 ms per cycle but took 19 instead of 14 cycles (UKS: 8.6 against 7.2 ms per cycle), so the plain loop stays the default
        there; `fast_loop = "always"` selects the fast loop whenever plans exist (the plain loop's final orbitals seed them)."""
        self._setup_once()
        n = self.engine.nao
        na, nb = self.mol.nelec
        self.nelec = (na, nb)
        small = n < self.sp2_min_nao or self.eig_method != "sp2"
        warm = all(no == 0 or sp.plan is not None for sp, no in zip(self._spin_states(n), (na, nb)))
        use_fast = self.fast_loop and (small or (self.fast_loop == "always" and warm))
        return self._run(dm0, use_fast)

    def _run(self, dm0, fast):
        """One SCF on the fast or the plain loop: the loop's start state, the outer loop of every driver, the common finish."""
        t_start = time.time()
        self._setup_once()
        na, nb = self.mol.nelec
        self.nelec = (na, nb)
        st = self._fast_start(dm0) if fast else self._plain_start(dm0)
        self._iterate(st, self._ustep if fast else self._plain_step)
        return self._ufinal(st, t_start)

    # Plain loop (round 3): once a spin's checked, trace-correcting purification has run with |g| below `sp2_trace_plan_gnorm`, its
    # trace history gives the bounds of a purification PLAN for that spin (sp2plan.bounds_from_traces, as in the closed-shell
    # cold path) and the following cycles run the ~21 planned passes instead of the 40-60 of the recursion; the result is checked
    # on the host like the recursion's (this loop synchronises per spin anyway) and a failed check drops the plan.
    def _planned_spin_density(self, fo, no, pur):
        n = fo.shape[0]
        if pur.plan is None or not (self.sp2_planned and self.sp2_trace_plan and n <= self.sp2_fused_max):
            return None
        res, tr_dev, layout = pur.planned(fo, no, scale=2.0)
        if not pur.accept(tr_dev.cpu().numpy(), layout, no):
            pur.plan = None                 # the spectrum left the planned window: checked recursion, new plan from its traces
            return None
        self.path_counts = getattr(self, "path_counts", {})
        self.path_counts["planned_spin"] = self.path_counts.get("planned_spin", 0) + 1
        return res.clone()                  # (a view of the spin's ping-pong buffers, which its next purification reuses)

    def _seed_plans(self, mo_e):
        """Purification plans of both spins from the orbital energies of a finished SCF (for the next kernel() of this object)."""
        n = self.engine.nao
        if self.eig_method != "sp2" or n < self.sp2_min_nao or not self.sp2_planned or self.level_shift:
            return
        for s_, sp in enumerate(self._spin_states(n)):
            if 0 < self.nelec[s_] < n:
                sp.replan(mo_e[s_], self.nelec[s_])

    scf = kernel

    def _spin_states(self, n):
        """The purifiers of the fast loop's two spin channels live on the object: a geometry optimisation (same `mf`,
        `kernel(dm0=...)` per step) reuses the plans of the previous geometry and diagonalises nothing after its first SCF."""
        key = (n, tuple(self.nelec))
        if getattr(self, "_spin_key", None) != key:
            self._spin_key, self._spin_pair = key, [Purifier(self), Purifier(self)]
        return self._spin_pair

    def _projector(self, st, s_, fo, nocc_s, allow_plan=True):
        """(X_s, traces or None, their purify.Layout) for one spin: planned purification when a plan exists, else `eigh`
        (which also yields the bounds for a plan).  X_s is the occupied projector (occupation 1) in the orthonormal basis."""
        n = fo.shape[0]
        sp = st["spin"][s_]
        if nocc_s == 0:
            return torch.zeros_like(fo), None, None
        can_plan = (self.eig_method == "sp2" and self.sp2_planned and n >= self.sp2_min_nao and 0 < nocc_s < n
                    and not self.level_shift)
        settled = st.get("gnorm") is not None and st["gnorm"] <= self.sp2_plan_gnorm
        if can_plan and allow_plan and sp.plan is not None and not settled:
            # plans exist but this SCF is still far from its solution (see SCF._route): checked purification, no redo cycles
            # (pass count shared by both spins: the object's own purifier)
            d2 = self._purifier.checked(fo, nocc_s)
            if d2 is not None:
                return 0.5 * d2, None, None
        if can_plan and allow_plan and sp.plan is not None and settled:
            return sp.planned(fo, nocc_s, 1.0)
        self.n_eigh = getattr(self, "n_eigh", 0) + 1
        e, c = torch.linalg.eigh(fo)
        co = c[:, :nocc_s]
        if can_plan:
            sp.replan(e, nocc_s)
        return co @ co.T, None, None

    def _ulaunch(self, st, dm, dmo, next_cycle, trs):
        """Device part of a cycle after the densities: Fock pair, F'_s = L^-1 F_s L^-T into the DIIS slot, error vectors
        [F'_s, X_s] (orthonormal-basis CDIIS error of PySCF >= 2.1, spin-stacked) and their norms, Pulay solve, asynchronous
        read-back of the scalars."""
        eng, Li = self.engine, self._Linv
        dm = dm.contiguous()
        # from cycle 1 on the spin densities are projectors X_s of rank n_s: lets UKS take rho_s from a low-rank factor
        self._xc_projector_pair = (dm, dmo, st["nocc"]) if next_cycle > 0 else None
        F, e_el = self._fock_pair(dm)
        diis = st["diis"]
        keep = next_cycle >= self.diis_start_cycle
        slot = diis.next_slot()
        nb = eng.reduce_blocks
        part = torch.empty(2 * nb, dtype=torch.float64, device=dm.device)
        fo = diis.F[slot] if keep else torch.empty_like(diis.F[0])
        eo = diis.E[slot] if keep else torch.empty_like(diis.E[0])
        for s_ in range(2):
            torch.matmul(Li @ F[s_], Li.T, out=fo[s_])
            eng.commutator_norm(fo[s_] @ dmo[s_], eo[s_], part[s_ * nb:(s_ + 1) * nb])
        if keep:
            diis.push_inplace()
        parts = [e_el.reshape(1), part] + [t for t in trs if t is not None]
        return dict(dm=dm, dmo=dmo, F=F, fo=fo, nb=nb, tr_sizes=[0 if t is None else t.numel() for t in trs],
                    scalars=self._scalars_launch(torch.cat(parts)))

    def _ufinish(self, st, ctx, layouts, e_last):
        """Host part: wait for the scalars, validate the purifications, update the state.  False: a purification was not
        converged (nothing in `st` touched)."""
        vals = self._scalars_wait(ctx["scalars"])
        nb = ctx["nb"]
        e_el = float(vals[0])
        c2 = float(vals[1:1 + 2 * nb].sum())
        pos = 1 + 2 * nb
        for s_ in range(2):
            k = ctx["tr_sizes"][s_]
            if not k:
                continue
            hist = vals[pos:pos + k]
            pos += k
            if not st["spin"][s_].accept(hist, layouts[s_], st["nocc"][s_]):
                return False
        e_tot = e_el + st["enuc"]
        gnorm = float(np.sqrt(max(c2, 0.0) / 2.0)) / np.sqrt(st["nvo"])
        st.update(dm=ctx["dm"], dmo=ctx["dmo"], F=ctx["F"], fo=ctx["fo"], e_tot=e_tot, gnorm=gnorm,
                  de=(e_tot - e_last) if e_last is not None else 0.0)
        return True

    def _ufront(self, st):
        """Device-only head of the next cycle (pair-extrapolated F', planned purification of both spins, AO densities), queued
        before the host waits for the current cycle's scalars.  None when either spin has no plan."""
        if not (self.pipeline and st["cycle"] + 1 >= self.diis_start_cycle and st["diis"].count > 0 and not self.level_shift):
            return None
        if st.get("gnorm") is None or st["gnorm"] > self.sp2_plan_gnorm:
            return None
        for s_ in range(2):
            if st["nocc"][s_] > 0 and st["spin"][s_].plan is None:
                return None
        n = self._Linv.shape[0]
        if not (self.eig_method == "sp2" and self.sp2_planned and n >= self.sp2_min_nao):
            return None
        fo = st["diis"].extrapolate()
        return self._udensities(st, fo)

    def _udensities(self, st, fo, allow_plan=True):
        Li = self._Linv
        xs, trs, layouts = zip(*(self._projector(st, s_, fo[s_], st["nocc"][s_], allow_plan) for s_ in range(2)))
        dmo = torch.stack(xs)
        dm = torch.stack([Li.T @ xs[0] @ Li, Li.T @ xs[1] @ Li])
        return dict(fo=fo, dmo=dmo, dm=dm, trs=trs, layouts=layouts)

    def _ustep(self, st):
        front = st.pop("front", None)
        if front is None:
            if st["cycle"] >= self.diis_start_cycle and st["diis"].count > 0:
                fo = st["diis"].extrapolate()
            else:
                fo = st["fo"]
            if self.level_shift:   # F'_s + shift (1 - X_s): virtual space of each spin raised
                eye = torch.eye(fo.shape[-1], dtype=fo.dtype, device=fo.device)
                fo = fo + self.level_shift * (eye.unsqueeze(0) - st["dmo"])
            front = self._udensities(st, fo)
        saved_count = st["diis"].count
        e_prev = st["e_tot"]
        ctx = self._ulaunch(st, front["dm"], front["dmo"], st["cycle"] + 1, front["trs"])
        nxt = self._ufront(st)
        ok = self._ufinish(st, ctx, front["layouts"], e_prev)
        if not ok:
            # a planned purification had not converged (the spectrum left the planned bounds): roll the DIIS push back and
            # redo the cycle by diagonalisation, which also refreshes the plans
            nxt = None
            self.n_redo = getattr(self, "n_redo", 0) + 1
            st["diis"].count = saved_count
            redo = self._udensities(st, front["fo"], allow_plan=False)
            ctx = self._ulaunch(st, redo["dm"], redo["dmo"], st["cycle"] + 1, redo["trs"])
            self._ufinish(st, ctx, redo["layouts"], e_prev)
        if nxt is not None:
            st["front"] = nxt
        st["cycle"] += 1
        return st

    def _udm0(self, dm0):
        """Starting spin densities [2, N, N] on the device (`self.nelec` set): the guess when `dm0` is None, a spin-summed
        density split by electron count, the same on every rank."""
        na, nb = self.nelec
        if dm0 is None:
            dm0 = self.get_init_guess()
        dm0 = np.asarray(dm0)
        if dm0.ndim == 2:
            ne = max(na + nb, 1)
            dm0 = np.stack([dm0 * (na / ne), dm0 * (nb / ne)])
        dm = torch.as_tensor(dm0, dtype=torch.float64, device=self.engine.device).contiguous()
        if self._nranks > 1:   # one-off: identical starting density on every rank (see SCF._start)
            from . import parallel
            parallel.broadcast0(dm, self._pg)
        return dm

    def _uorbitals(self, F):
        """(mo_energy[2, N], mo_coeff[2, N, N]) on the device: one `eigh` of the Cholesky-orthogonalised Fock matrix per spin
        (per matrix of the stack `F`: ROHF passes its one effective Fock matrix)."""
        Li = self._Linv
        es, cs = [], []
        for f in F:
            e_, c_ = torch.linalg.eigh(Li @ f @ Li.T)
            es.append(e_); cs.append(Li.T @ c_)
        return torch.stack(es), torch.stack(cs)

    # --- what the plain loop asks of its class (rohf.ROHF overrides them) --------------------
    def _diis_pair(self, F, dm):
        """(matrices CDIIS extrapolates and the orbitals come from, their AO error vectors, squared norm of the error vectors in
        the orthonormal basis as a device scalar) for the Fock pair F of the spin densities dm: the pair itself with
        F_s D_s S - S D_s F_s."""
        S, Li = self._S, self._Linv
        err = torch.stack([F[s_] @ dm[s_] @ S - S @ dm[s_] @ F[s_] for s_ in range(2)])
        # |g| = |F_vo| of both spins = |[F', D']|_F / sqrt(2) in the orthonormal basis (D' is a projector)
        eo = torch.stack([Li @ err[s_] @ Li.T for s_ in range(2)])
        return F, err, torch.sum(eo * eo)

    def _shift_densities(self, dm):
        """Occupied-space projectors (AO densities of occupation 1) that `level_shift` leaves unshifted, one per matrix of
        `_diis_pair`."""
        return dm

    def _n_rotations(self):
        """Number of independent orbital rotations, the normalisation of |g|."""
        n = self.engine.nao
        na, nb = self.nelec
        return max(na * (n - na) + nb * (n - nb), 1)

    def _set_orbitals(self, dm, F, mo_e, mo_c):
        """Host copies of the final orbitals with aufbau occupations, and the purification plans of the next kernel()."""
        na, nb = self.nelec
        self.mo_energy = mo_e.cpu().numpy()
        self._seed_plans(mo_e)
        self.mo_coeff = mo_c.cpu().numpy()
        occ = np.zeros((2, self.engine.nao))
        occ[0, :na] = 1.0
        occ[1, :nb] = 1.0
        self.mo_occ = occ

    def _uresult(self, dm, F, e_tot, mo_e, mo_c, t_start):
        """Results of a finished loop onto the object; returns e_tot."""
        self._dm, self._fock = dm, F
        self.e_tot = e_tot
        self._set_orbitals(dm, F, mo_e, mo_c)
        self.timing["total_seconds"] = time.time() - t_start
        if self.converged:
            ss, mult = self.spin_square()
            self._log(3, f"converged SCF energy = {self.e_tot:.15g}  <S^2> = {ss:.8g}  2S+1 = {mult:.8g}")
        else:
            self._log(3, f"SCF not converged.\nSCF energy = {self.e_tot:.15g} after {self.max_cycle} cycles")
        return self.e_tot

    def _occupied_density(self, mo_c):
        na, nb = self.nelec
        ca, cb = mo_c[0][:, :na], mo_c[-1][:, :nb]      # (one orbital set: the beta orbitals are the first n_beta of it)
        return torch.stack([ca @ ca.T, cb @ cb.T])

    def _ufinal(self, st, t_start):
        """After `_iterate`, for both loops: the final orbitals, the `conv_check` extra cycle (density of those orbitals, one Fock
        build, no extrapolation), the results.  Where the two loops differ they do so on purpose:"""
        plain = st["plain"]
        check = self.converged and self.conv_check
        if plain and st["use_sp2"]:
            # the pass count of the spin purified last carries over to the object (the fast loop's purifiers live on the object)
            self._purifier.iters = st["pur"][1 if self.nelec[1] else 0].iters
        if plain:
            # plain loop: the matrix CDIIS extrapolates (ROHF: F_eff) is diagonalised for the extra cycle, when the loop has made no
            # orbitals (max_cycle = 0) and when it purified; otherwise -- not converged, or conv_check off -- the orbitals of the
            # last in-loop `eigh` are kept, which belong to the last EXTRAPOLATED (and level-shifted) matrix, not to `Fd`
            Fd, fresh = st["Fd"], check or st["mo_e"] is None or st["use_sp2"]
        else:
            # fast loop: always the orbitals of the last Fock pair (its cycles keep projectors, not orbitals)
            Fd, fresh = st["F"], True
        mo_e, mo_c = self._uorbitals(Fd) if fresh else (st["mo_e"], st["mo_c"])
        dm, F, e_tot = st["dm"], st["F"], st["e_tot"]
        if check:
            dm = self._occupied_density(mo_c)
            F, e_el = self._fock_pair(dm)
            if st.get("sync") is not None:        # plain loop, sharded: rank 0's energy on every rank, like the cycles' scalars
                e_el = e_el.reshape(1)
                st["sync"](e_el)
            e_new = float(e_el) + st["enuc"]
            self._log(4, f"Extra cycle  E= {e_new:.15g}  delta_E= {e_new - e_tot:.3g}")
            e_tot = e_new
        return self._uresult(dm, F, e_tot, mo_e, mo_c, t_start)

    # --- the plain loop: AO basis, host-side pair DIIS, one host sync per cycle -------------------------------------------
    def _plain_start(self, dm0):
        """State of the plain loop after the first Fock build (`self.nelec` set)."""
        dm = self._udm0(dm0)
        enuc = self.energy_nuc()
        # sharded runs: the all-reduced J/K(/Vxc) are identical on every rank and the replicated algebra below is made of
        # deterministic library reductions, so the ranks stay bit-identical without broadcasting control scalars;
        # `sync_control` (auto-on for sharded runs, see scf.SCF) makes rank 0's Gram row / scalars authoritative
        sync = None
        if self._sync_control_on():
            from . import parallel
            sync = lambda t: parallel.broadcast0(t, self._pg)
        F, e_el = self._fock_pair(dm)
        st = {"plain": True, "enuc": enuc, "cycle": 0, "diis": PairDIIS(self.diis_space, sync), "sync": sync,
              "nvo": self._n_rotations(), "dm": dm, "F": F, "e_tot": float(e_el) + enuc, "de": 0.0, "gnorm": 0.0,
              "mo_e": None, "mo_c": None}
        # larger matrices: occupied projector of each spin by SP2 purification (same GEMM-only path as RHF, `scf.py`)
        # instead of a diagonalisation per cycle; orbitals are then only needed once, after convergence
        st["use_sp2"] = self._purify_spins and self.eig_method == "sp2" and self.engine.nao >= self.sp2_min_nao
        # one purifier per spin for this kernel() only (plans from the traces of its checked runs), starting from the object's
        # pass count
        st["pur"] = [Purifier(self, self._purifier.iters) for _ in range(2)]
        st["Fd"], st["err"], _g2 = self._diis_pair(F, dm)
        return st

    def _plain_density(self, st, Fx):
        """(spin densities, spin projectors X_s in the orthonormal basis or None, (mo_e, mo_c) or None) from the matrices `Fx`:
        by `eigh` (orbitals, no projectors) or by purifying each spin (projectors unless a spin fell back to `eigh`; no
        orbitals)."""
        if not st["use_sp2"]:
            mo = self._uorbitals(Fx)
            return self._occupied_density(mo[1]), None, mo
        n, Li = self.engine.nao, self._Linv
        out = []
        xs = []        # (UKS takes rho_s from a low-rank factor of X_s, `_xc_projector_pair`)
        for s_, no in enumerate(self.nelec):
            if no == 0:
                out.append(torch.zeros(n, n, dtype=torch.float64, device=self.engine.device))
                xs.append(out[-1])
                continue
            fo = (Li @ Fx[s_] @ Li.T).contiguous()
            p = st["pur"][s_]
            dmo = self._planned_spin_density(fo, no, p)
            if dmo is None:
                dmo = p.checked(fo, no)
                g_prev = st["gnorm"] if st["cycle"] > 0 else 1.0e9      # (no orbital gradient before the first cycle has finished)
                if (p.trace_bounds is not None and self.sp2_planned and self.sp2_trace_plan
                        and g_prev <= self.sp2_trace_plan_gnorm):
                    p.plan_from_traces()
                p.trace_bounds = None
            if dmo is None:      # purification did not converge (vanishing gap): diagonalise this spin
                e_, c_ = torch.linalg.eigh(fo)
                co = Li.T @ c_[:, :no]
                out.append(co @ co.T)
                xs = None
            else:
                out.append(0.5 * (Li.T @ dmo @ Li))
                if xs is not None:
                    xs.append(0.5 * dmo)
        return torch.stack(out), xs, None

    def _fock_pair_of_projectors(self, dm, xs):
        """`_fock_pair(dm)` with the spin densities declared projectors `xs` of known rank: UKS takes rho_s from their low-rank
        factors (one pass over the AO values instead of an N x N x n_grid product per spin), exactly as in the fast loop.  A
        failed factorisation poisons itself with NaN: the pair is then rebuilt from the full densities."""
        self._xc_projector_pair = (dm, xs, self.nelec) if xs is not None else None
        F, e_el = self._fock_pair(dm)
        if xs is not None and not bool(torch.isfinite(e_el).all()):
            self._xc_projector_pair = None
            F, e_el = self._fock_pair(dm)
        self._xc_projector_pair = None
        return F, e_el

    def _plain_step(self, st):
        """One cycle: CDIIS extrapolation (and level shift) -> spin densities -> Fock pair -> energy and |g|, one host sync."""
        S = self._S
        Fx = st["diis"].update(st["Fd"], st["err"]) if st["cycle"] + 1 >= self.diis_start_cycle else st["Fd"]
        if self.level_shift:   # F_s + shift (S - S D_s S): virtual space of each spin raised (AO form of PySCF's level_shift)
            Fx = Fx + self.level_shift * (S.unsqueeze(0) - torch.stack([S @ d @ S for d in self._shift_densities(st["dm"])]))
        dm, xs, mo = self._plain_density(st, Fx)
        if mo is not None:
            st["mo_e"], st["mo_c"] = mo
        F, e_el = self._fock_pair_of_projectors(dm, xs)
        Fd, err, g2 = self._diis_pair(F, dm)
        ctrl = torch.stack([e_el.reshape(()), g2.reshape(())])
        if st["sync"] is not None:
            st["sync"](ctrl)
        ctrl = ctrl.cpu().numpy()
        e_tot = float(ctrl[0]) + st["enuc"]
        gnorm = float(np.sqrt(max(ctrl[1], 0.0) / 2.0)) / np.sqrt(st["nvo"])
        st.update(dm=dm, F=F, Fd=Fd, err=err, de=e_tot - st["e_tot"], e_tot=e_tot, gnorm=gnorm, cycle=st["cycle"] + 1)
        return st

    # --- the fast loop: orthonormal basis, device-side pair DIIS, pipelined step (`_ustep`) -------------------------------
    def _fast_start(self, dm0):
        """State of the fast loop after the first Fock build (`self.nelec` set)."""
        eng, L = self.engine, self._L
        n = eng.nao
        na, nb = self.nelec
        dm = self._udm0(dm0)
        st = {"plain": False, "nocc": (na, nb), "enuc": self.energy_nuc(), "cycle": 0,
              "diis": DeviceDIIS(eng, self.diis_space, nmat=2), "spin": self._spin_states(n),
              "nvo": max(na * (n - na) + nb * (n - nb), 1), "e_tot": None}
        dmo0 = torch.stack([L.T @ dm[0] @ L, L.T @ dm[1] @ L])
        ctx = self._ulaunch(st, dm, dmo0, 0, [None, None])
        self._ufinish(st, ctx, [None, None], None)
        return st

    def dip_moment(self, mol=None, dm=None, unit="Debye", verbose=None, **kw):
        if dm is None:
            dm = self.make_rdm1()
        dm = np.asarray(dm)
        if dm.ndim == 3:
            dm = dm[0] + dm[1]
        return SCF.dip_moment(self, mol, dm, unit, verbose, **kw)

    def nuc_grad_method(self):
        from . import grad
        return grad.UGradients(self)

    Gradients = nuc_grad_method
