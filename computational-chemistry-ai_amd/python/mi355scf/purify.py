"""The SCF's density step: the occupied-space projector of one spin channel's orthonormal-basis Fock matrix F' by SP2
purification, without diagonalisation.

One `Purifier` per spin channel owns the state of that channel -- the purification plan (`sp2plan.py`), the pass count of the
trace-correcting recursion, the trace bounds a plan can be made from, and the device workspaces -- and offers three routes:

  checked     trace-correcting SP2, validated on the host inside (a host sync); None when it does not converge
  optimistic  trace-correcting SP2 with a given pass count, no host sync: the caller validates the traces with the cycle's
              other scalars
  planned     the planned sequence of quadratics (about half the passes), no host sync, validated like `optimistic`

Each route takes F' and the occupation and returns the result together with the `Layout` of the traces the caller must
check (`accept`).  N <= `sp2_fused_max` runs the fused HIP kernels, larger N rocBLAS DGEMMs plus small kernels.  The knobs
(`sp2_tol`, `sp2_margin`, `sp2_fused_max`, ...) stay on the SCF object that owns the purifier.
"""
import weakref
from collections import namedtuple

import numpy as np
import torch

from . import sp2plan

HEAD_MAX = 4096   # doubles reserved in front of the planned-path trace history for [E partials | |g|^2 partials | extra]
TRACE_SLOTS = 64  # doubles per pass in a trace history: 2 ceil(n / 16) interleaved partials used (n <= 512), the rest never written

# Trace history of `passes` passes, 2 `nbd` partials used per pass, `ndiscs` Gershgorin values behind it (cold objects: the bounds
# of a plan).  `planned`: a failed check rejects the plan, a passed one trims it.  `head`: the buffer the history sits in,
# HEAD_MAX doubles behind its start -- the Fock build writes its partial sums into that head, so that the cycle's scalars
# leave the device as one copy.  A layout of None means a single (tr X, tr X^2) pair.
Layout = namedtuple("Layout", "passes nbd ndiscs planned head", defaults=(0, False, None))


def pair_traces(tr_host):
    """(tr X, tr X^2) from interleaved partial traces (or a plain pair), added in index order."""
    t = np.asarray(tr_host, dtype=np.float64).reshape(-1, 2)
    return float(t[:, 0].sum()), float(t[:, 1].sum())


def check_history(hist, layout, nocc, tol):
    """Check a trace history read back from the device: per pass, |tr X - tr X^2| < `tol` and |tr X - nocc| < 1e-8.

    Returns (first, tx, tx2, discs): `first` is the first pass that met the test, or None when the LAST pass did not (the
    result is rejected); tx, tx2 the per-pass traces; discs the Gershgorin values of the tail (None without a tail)."""
    hist = np.asarray(hist, dtype=np.float64)
    size = layout.passes * TRACE_SLOTS
    if hist.size != size + layout.ndiscs:
        raise ValueError(f"trace history of {hist.size} doubles, layout {layout} needs {size + layout.ndiscs}")
    discs = hist[size:] if layout.ndiscs else None
    h = hist[:size].reshape(layout.passes, TRACE_SLOTS // 2, 2)[:, :layout.nbd, :]
    tx, tx2 = h[:, :, 0].sum(axis=1), h[:, :, 1].sum(axis=1)     # per pass, partials added in index order
    ok = (np.abs(tx - tx2) < tol) & (np.abs(tx - nocc) < 1e-8)
    first = int(np.argmax(ok)) if ok[-1] else None
    return first, tx, tx2, discs


class Purifier:
    def __init__(self, mf, iters=24):
        # a weak reference: the SCF object holds its purifier, and a cycle would keep the object -- and its engine, whose
        # library context must be destroyed while the HIP runtime is still up -- alive until interpreter shutdown
        self._owner = weakref.ref(mf)
        self.plan = None          # sp2plan.plan coefficients [steps + 1, 3]
        self.plan_len = 0         # steps of the plan actually run (trimmed by `accept`)
        self.plan_gen = 0         # bumped by every new plan (part of the HIP-graph key of the SCF head)
        self.from_traces = False  # the plan came from the traces of a trace-correcting run, not from a spectrum
        self.iters = iters        # passes of the trace-correcting recursion that sufficed last time
        self.validated = False    # True once a pass count has passed a check for this Fock spectrum
        self.trace_bounds = None  # (tx, tx2, emin, emax) of the last checked run of a cold object: what a plan needs
        self.ws = {}              # device workspaces by route

    @property
    def mf(self):
        """The SCF object that owns this purifier (its knobs and engine)."""
        return self._owner()

    def rebind(self, mf):
        """This purifier's state for another SCF object sharing it (solvent.PCM wraps a copy of the object's attributes)."""
        p = Purifier.__new__(Purifier)
        p.__dict__.update(self.__dict__)
        p._owner = weakref.ref(mf)
        return p

    def _buf(self, key, fo, make):
        n = fo.shape[0]
        ws = self.ws.get(key)
        if ws is None or ws["n"] != n:
            ws = self.ws[key] = dict(n=n, **make(n, lambda *s: torch.empty(*s, dtype=torch.float64, device=fo.device)))
        return ws

    # --- routes --------------------------------------------------------------------------------------------------------
    def checked(self, fo, nocc):
        """D' = 2 P_occ(F') by the trace-correcting recursion, checked on the host, the pass count adapted; None if it does
        not converge (e.g. vanishing HOMO-LUMO gap): the caller then diagonalises."""
        n = fo.shape[0]
        if nocc == 0 or nocc >= n:
            return None
        if n <= self.mf.sp2_fused_max:
            return self._checked_fused(fo, nocc)
        eng, mf = self.mf.engine, self.mf
        ws = self._gemm_ws(fo)
        buf, cur = ws["buf"], 0
        X = buf[cur][2:].view(n, n)
        eng.sp2_init(fo.contiguous(), X, buf[1 - cur])
        X2 = ws["x2"]
        nit = self.iters
        target = float(nocc)
        done = 0
        for attempt in range(6):
            for _ in range(nit - done):
                torch.matmul(X, X, out=X2)
                eng.sp2_update(X, X2, target, buf[1 - cur])   # one fused launch: traces, branch, update
                cur = 1 - cur
                X = buf[cur][2:].view(n, n)
            done = nit
            torch.matmul(X, X, out=X2)
            tr = torch.stack([torch.trace(X), torch.trace(X2)]).cpu()
            err = float(tr[0] - tr[1])          # = sum lambda (1 - lambda) >= 0
            if abs(err) < mf.sp2_tol and abs(float(tr[0]) - target) < 1e-8:
                self.iters = nit
                self.validated = True
                return X + X.T                     # exactly symmetric 2 X (see _planned_gemm)
            nit += 8
        return None

    def _gemm_ws(self, fo):
        return self._buf("gemm", fo, lambda n, mk: dict(buf=[mk(2 + n * n) for _ in range(2)], x2=mk(n, n)))

    def _fused_ws(self, fo):
        return self._buf("fused", fo, lambda n, mk: dict(X=mk(n, n), X2=mk(n, n), work=mk(2 * n * n), tr=mk(TRACE_SLOTS * 80),
                                                         b=mk(2 * n), pp=(mk(2, n, n), mk(2, n, n))))

    def _wants_discs(self):
        """Cold object: the Gershgorin discs of F' travel with the traces, so that a plan can be made from the run."""
        return self.mf.sp2_trace_plan and self.mf.sp2_planned and self.plan is None

    def _checked_fused(self, fo, nocc):
        """Same recursion, one fused HIP launch per pass (`sp2_fused_kernel`, FP64 MFMA)."""
        eng, mf = self.mf.engine, self.mf
        n = fo.shape[0]
        ws = self._fused_ws(fo)
        nit = min(self.iters, 72)
        target = float(nocc)
        nbd = (n + 15) // 16
        for attempt in range(5):
            eng.sp2_init(fo.contiguous(), ws["X"], ws["b"])
            off = eng.sp2_iterate(ws["X"], ws["X2"], nit, target, ws["work"], ws["tr"])
            trx, trx2 = pair_traces(ws["tr"][off:off + 2 * nbd].cpu().numpy())
            if abs(trx - trx2) < mf.sp2_tol and abs(trx - target) < 1e-8:
                self.iters = nit
                self.validated = True
                if self._wants_discs() and off == TRACE_SLOTS * nit:
                    # the history of this checked run and the Gershgorin discs give the bounds for a plan (one more small copy
                    # in a path that waits for the device anyway)
                    h = torch.cat([ws["tr"][:off + TRACE_SLOTS], ws["b"][:2 * n]]).cpu().numpy()
                    _, tx, tx2, discs = check_history(h, Layout(nit + 1, nbd, 2 * n), nocc, mf.sp2_tol)
                    self.trace_bounds = (tx, tx2, float(discs[:n].min()), float(discs[n:].max()))
                return 2.0 * ws["X"]
            nit = min(nit + 8, 76)
        return None

    def optimistic(self, fo, nocc, passes=None):
        """Trace-correcting recursion with `passes` passes (default: the count that worked last time), enqueued WITHOUT a host
        sync: (D', device traces, layout).  The caller validates them together with the cycle's other scalars and redoes the
        cycle through `checked` if the count was too small."""
        eng = self.mf.engine
        n = fo.shape[0]
        ws = self._fused_ws(fo)
        nit = min(self.iters if passes is None else passes, 76)
        if n <= self.mf.sp2_fused_max:
            pp = ws["pp"]   # two [X | X2] buffers: the passes ping-pong between them and the result is read where it lands
            eng.sp2_init(fo.contiguous(), pp[0][0], ws["b"])
            res, off = eng.sp2_iterate_pingpong(pp[0], pp[1], nit, float(nocc), ws["tr"])
            # the partial traces of EVERY pass: the host validates the last one and reads off the first pass at which the
            # projector was already converged (-> pass count of the next cycle)
            layout = Layout(nit + 1, (n + 15) // 16)
            if self._wants_discs():
                layout = layout._replace(ndiscs=2 * n)
                return 2.0 * res[0], torch.cat([ws["tr"][:off + TRACE_SLOTS], ws["b"][:2 * n]]), layout
            return 2.0 * res[0], ws["tr"][:off + TRACE_SLOTS], layout
        eng.sp2_init(fo.contiguous(), ws["X"], ws["b"])
        # larger N: rocBLAS DGEMM + fused update kernel per pass, still without a host sync
        buf = self._gemm_ws(fo)["buf"]
        X, X2, cur = ws["X"], ws["X2"], 0
        for _ in range(nit):
            torch.matmul(X, X, out=X2)
            eng.sp2_update(X, X2, float(nocc), buf[cur])
            X = buf[cur][2:].view(n, n)
            cur = 1 - cur
        torch.matmul(X, X, out=X2)
        return X + X.T, torch.stack([torch.trace(X), torch.trace(X2)]), None   # exactly symmetric 2 X (see _planned_gemm)

    def planned(self, fo, nocc, scale=2.0, slot=0):
        """Planned purification, no host sync: (scale X, device traces, layout), validated by the caller like `optimistic`.
        N <= sp2_fused_max: the traces of every pass land HEAD_MAX doubles into a persistent buffer (`layout.head`) whose head
        the Fock build fills afterwards.  `slot` picks one of two such output sets (result and traces), so that two captured
        SCF heads never write over each other's outputs."""
        n = fo.shape[0]
        if n > self.mf.sp2_fused_max:
            return self._planned_gemm(fo, scale)
        eng = self.mf.engine
        ws = self._buf(("planned", slot), fo, lambda n, mk: dict(scal=mk(HEAD_MAX + TRACE_SLOTS * 80), pp=(mk(2, n, n), mk(2, n, n))))
        want = int(bool(self.mf.sp2_direct))
        if getattr(eng, "_sp2_direct", None) != want:
            eng.set_option("sp2_direct", want)
            eng._sp2_direct = want
        coef = self.plan[:self.plan_len + 1]
        tr = ws["scal"][HEAD_MAX:]
        res, off = eng.sp2_iterate_planned(fo.contiguous(), ws["pp"][0], ws["pp"][1], coef, tr, out_scale=scale)
        # the result is a view of the ping-pong buffers: consumed by this cycle's Fock build, before the next pass
        return res[0], tr[:off + TRACE_SLOTS], Layout(coef.shape[0], (n + 15) // 16, planned=True, head=ws["scal"])

    def _planned_gemm(self, fo, scale):
        """Planned purification beyond the fused kernel (ibuprofen N = 573, C60 N = 840): X_{k+1} = a X_k^2 + b X_k + c I as ONE
        `addmm` (rocBLAS DGEMM with beta) plus a diagonal shift per pass -- half the passes of the trace-correcting recursion,
        and no branch decisions on the device.  Only the last pass is checked: tr X and tr X^2 = |X|_F^2 (X is symmetric)
        travel to the host with the cycle's other scalars."""
        n = fo.shape[0]
        coef = self.plan[:self.plan_len + 1]
        buf = self._buf("planned_gemm", fo, lambda n, mk: dict(x=[mk(n, n) for _ in range(3)]))["x"]
        X = torch.mul(fo, float(coef[0, 1]), out=buf[0])
        X.diagonal().add_(float(coef[0, 2]))
        cur, nit = 0, coef.shape[0] - 1
        for k in range(1, nit + 1):
            a, b, c = (float(v) for v in coef[k])
            Y = torch.addmm(X, X, X, beta=b, alpha=a, out=buf[(cur + 1) % 3])
            cur = (cur + 1) % 3
            if c != 0.0:
                Y.diagonal().add_(c)
            if k % 4 == 0 or k == nit:
                # a library GEMM does not return X.X exactly symmetric, and the antisymmetric part A obeys A <- a (SA + AS) + b A:
                # it can double per pass while the gap is being opened (1e-16 -> 1e-12 over 20 passes, measured).  The J/K kernel
                # reads one triangle of D, so an asymmetric D shows up as 1e-9 Ha cycle-to-cycle jitter of a 650 Ha energy
                # (tools/noise_check.py; the fused kernel's mirror stores keep X exactly symmetric)
                Y = torch.add(Y, Y.T, out=buf[(cur + 1) % 3]).mul_(0.5)
                cur = (cur + 1) % 3
            X = Y
        tr = torch.stack([torch.trace(X), torch.sum(X * X)])
        return scale * X, tr, None

    # --- acceptance and planning ---------------------------------------------------------------------------------------
    def accept(self, hist, layout, nocc):
        """Check the read-back traces of an `optimistic` or `planned` result.  False: reject it (nothing changed).  True: a
        trace history also trims the plan to the passes that were needed, or sets the next pass count of the recursion (and,
        with Gershgorin discs behind it, the bounds a plan can be made from)."""
        tol = self.mf.sp2_tol
        if layout is None:
            trx, trx2 = pair_traces(hist)
            return abs(trx - trx2) < tol and abs(trx - nocc) < 1e-8
        first, tx, tx2, discs = check_history(hist, layout, nocc, tol)
        if first is None:
            return False
        self.validated = True
        if layout.planned:
            self.plan_len = min(self.plan.shape[0] - 1, max(first + 1, 4))   # passes beyond `first` were not needed
        else:
            self.iters = max(first + self.mf.sp2_margin, 4)
            if discs is not None:
                nd = discs.size // 2
                self.trace_bounds = (tx, tx2, float(discs[:nd].min()), float(discs[nd:].max()))
        return True

    def _set_plan(self, plan):
        self.plan = plan
        self.plan_gen += 1
        if plan is not None:
            self.plan_len = plan.shape[0] - 1

    def replan(self, mo_e, nocc):
        """New plan from the eigenvalues of the (orthonormal-basis) Fock matrix just diagonalised."""
        mf = self.mf
        e = mo_e.cpu().numpy() if torch.is_tensor(mo_e) else np.asarray(mo_e)
        self.from_traces = False
        plan = None
        if mf.sp2_planned and mf.eig_method == "sp2" and 0 < nocc < len(e):
            plan = sp2plan.plan(*sp2plan.bounds_from_spectrum(e, nocc, mf.sp2_inner_margin, mf.sp2_outer_margin))
        self._set_plan(plan)

    def plan_from_traces(self):
        """A plan from `trace_bounds` (which it consumes); True if one was made."""
        tx, tx2, emin, emax = self.trace_bounds
        self.trace_bounds = None
        b = sp2plan.bounds_from_traces(tx, tx2, emin, emax, self.mf.sp2_inner_margin)
        plan = sp2plan.plan(*b) if b is not None else None
        if plan is None:
            return False
        self._set_plan(plan)
        self.from_traces = True
        return True
