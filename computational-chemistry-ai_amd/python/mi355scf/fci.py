"""Determinant full CI in an active space behind `pyscf.fci` and `mcscf.CASCI(...).fcisolver`
(`templates/calculate_casscf.py:126-131,187`): PySCF's `direct_spin1` problem on the MI355X.

Convention (the same in `csrc/fci_kernels.h`).  `norb` <= 16 spatial orbitals, `(na, nb)` electrons.  A string is an occupation
bit mask (bit p = orbital p); the strings of one spin are numbered in ascending integer order (`make_strings`).  The determinant
|Ia Ib> is (alpha creators in ascending orbital order)(beta creators in ascending orbital order)|0>, so a same-spin replacement
a+_p a_q carries the sign of its own string only: (-1)^(occupied orbitals strictly between p and q).  A CI vector is an FP64
array [n_alpha_strings, n_beta_strings], beta fastest.  No spin adaptation: a vector lives in one (na, nb) sector.

sigma = H c in the Knowles-Handy form, H = sum h~_pq E_pq + 1/2 sum (pq|rs) E_pq E_rs, h~_pq = h_pq - 1/2 sum_r (pr|rq):

    D[rs, J]  = <J|E_rs|c>                          gather over the link tables      (mi_fci_gather_d)
    F[pq, J]  = sum_rs 1/2 (pq|rs) D[rs, J] + h~_pq c[J]   ONE FP64 GEMM (rocBLAS): D carries c as an extra plane
    sigma[I] += sum_pq <I|E_pq|F_pq>                gather over the same tables      (mi_fci_gather_sigma)

D and F take 2 (norb^2 + 1) 8 bytes per determinant and vector; the determinants are processed in chunks of whole alpha rows
(all beta strings of a range of alpha strings, ragged last chunk) so that both stay below `max_workspace_mb`; all trial
vectors of a Davidson iteration go through the same launches.  The diagonal (mi_fci_hdiag), the density matrices and <S^2>
(gather + GEMM on the same D) use the same tables.

Davidson: `tdscf.davidson_tda` is a plain symmetric-operator Davidson on device tensors (matvec on a stack of rows, diagonal
preconditioner, restart) and is used as it is.  The start space (`_start_vectors`) is the determinant of lowest diagonal energy,
or for `nroots > 1` the 4 nroots lowest, so that the first Rayleigh-Ritz step is a small p-space diagonalisation; a little
fixed noise on them keeps roots of other symmetries reachable.

There is no CPU fallback: everything but the host-side string tables needs the engine library and a GPU.
"""
import ctypes
import sys
from math import comb

import numpy as np

MAX_NORB = 16
LINK_MODE_ALPHA, LINK_MODE_BETA, LINK_MODE_BOTH = 1, 2, 3


# =================================================================================================
# strings and link tables (host, NumPy)
# =================================================================================================
def num_strings(n, m):
    """Number of strings of `m` electrons in `n` orbitals."""
    return comb(int(n), int(m)) if 0 <= m <= n else 0


def make_strings(orb_list, nelec):
    """Occupation bit masks of `nelec` electrons in the orbitals `orb_list` (an int n means range(n)), ascending (int64)."""
    orbs = list(range(orb_list)) if isinstance(orb_list, (int, np.integer)) else [int(o) for o in orb_list]
    nelec = int(nelec)
    if nelec < 0 or nelec > len(orbs):
        raise ValueError(f"{nelec} electrons do not fit in {len(orbs)} orbitals")
    if max(orbs, default=0) >= 62:
        raise ValueError("orbital indices must be below 62")
    level = {0: np.zeros(1, dtype=np.int64)}      # k -> all masks with k bits among the orbitals seen so far
    for o in sorted(orbs):
        nxt = {}
        for k, arr in level.items():
            nxt.setdefault(k, []).append(arr)
            if k < nelec:
                nxt.setdefault(k + 1, []).append(arr | (np.int64(1) << np.int64(o)))
        level = {k: np.concatenate(v) for k, v in nxt.items()}
    return np.sort(level[nelec])


def str2addr(norb, nelec, string):
    """Position of the bit mask `string` in `make_strings(norb, nelec)` (ascending integers = colexicographic rank)."""
    s, addr, k = int(string), 0, 0
    if bin(s).count("1") != nelec or s >> norb:
        raise ValueError(f"{bin(s)} is not a string of {nelec} electrons in {norb} orbitals")
    for p in range(norb):
        if (s >> p) & 1:
            k += 1
            addr += comb(p, k)
    return addr


def addr2str(norb, nelec, addr):
    """Inverse of `str2addr`."""
    addr = int(addr)
    if not 0 <= addr < num_strings(norb, nelec):
        raise ValueError(f"address {addr} outside [0, {num_strings(norb, nelec)})")
    s, p = 0, norb
    for k in range(nelec, 0, -1):
        p -= 1
        while comb(p, k) > addr:
            p -= 1
        addr -= comb(p, k)
        s |= 1 << p
    return s


def dense_link_table(norb, nelec):
    """[norb^2, nstr] int32: entry [ann * norb + cre, J] = sgn * (T + 1) when a+_cre a_ann |J> = sgn |T>, else 0."""
    strs = make_strings(norb, nelec)
    tab = np.zeros((norb * norb, len(strs)), dtype=np.int32)
    one = np.int64(1)
    for q in range(norb):          # annihilated
        has_q = (strs >> np.int64(q)) & one == 1
        for p in range(norb):      # created
            ok = has_q if p == q else has_q & ((strs >> np.int64(p)) & one == 0)
            if not ok.any():
                continue
            src = strs[ok]
            new = (src ^ (one << np.int64(q))) | (one << np.int64(p))
            lo, hi = min(p, q), max(p, q)
            between = src & np.int64(((1 << hi) - 1) ^ ((1 << (lo + 1)) - 1)) if hi > lo else np.zeros_like(src)
            par = np.zeros_like(src)
            for b in range(lo + 1, hi):
                par ^= (between >> np.int64(b)) & one
            tgt = np.searchsorted(strs, new)
            tab[q * norb + p, ok] = ((1 - 2 * par) * (tgt + 1)).astype(np.int32)
    return tab


def link_table(norb, nelec):
    """[nstr, nlink, 4] int32 rows (cre, ann, target address, sign) of the nlink = nelec (norb - nelec) + nelec single
    replacements a+_cre a_ann |J> = sign |target> of every string J."""
    tab = dense_link_table(norb, nelec)
    nstr = tab.shape[1]
    nlink = nelec * (norb - nelec) + nelec
    J, rs = np.nonzero(tab.T)
    assert len(J) == nstr * nlink
    t = tab.T[J, rs]
    out = np.stack([rs % norb, rs // norb, np.abs(t) - 1, np.sign(t)], axis=1).astype(np.int32)
    return out.reshape(nstr, nlink, 4)


def _unpack_nelec(nelec):
    if isinstance(nelec, (int, np.integer)):
        n = int(nelec)
        nb = n // 2          # Ms = 0, or Ms = 1/2 for an odd count
        return n - nb, nb
    na, nb = nelec
    return int(na), int(nb)


def restore_eri(eri, norb):
    """(pq|rs) as a [norb]*4 array from a 4-index array, the 4-fold packed [npair, npair] or the 8-fold packed [npair (npair+1)/2]
    form (pairs p >= q in row-major triangular order, as PySCF's ao2mo.restore [MEM])."""
    eri = np.asarray(eri, dtype=np.float64)
    n, npair = norb, norb * (norb + 1) // 2
    if eri.shape == (n, n, n, n):
        return eri
    if eri.size == n ** 4:
        return eri.reshape(n, n, n, n)
    tri = np.zeros((n, n), dtype=np.int64)
    il = np.tril_indices(n)
    tri[il] = np.arange(npair)
    tri = np.maximum(tri, tri.T)
    if eri.size == npair * npair:
        e4 = eri.reshape(npair, npair)
    elif eri.size == npair * (npair + 1) // 2:
        e4 = np.zeros((npair, npair))
        e4[np.tril_indices(npair)] = eri.ravel()
        e4 = e4 + e4.T - np.diag(np.diag(e4))
    else:
        raise ValueError(f"eri of shape {eri.shape} is neither 4-index nor 4-/8-fold packed for norb = {norb}")
    return e4[tri.reshape(-1)][:, tri.reshape(-1)].reshape(n, n, n, n)


def absorb_h1e(h1e, eri, norb, nelec, fac=1.0):
    """PySCF's `direct_spin1.absorb_h1e` [MEM]: g = fac (eri + (h~ x 1 + 1 x h~) / N), h~_pq = h_pq - 1/2 sum_r (pr|rq), so that
    with fac = 1/2, sum g_pqrs E_pq E_rs = H on N-electron states (sum_r E_rr = N): `contract_2e(g, c, norb, nelec)` is H c.
    Needs at least one electron."""
    n = sum(_unpack_nelec(nelec))
    if n < 1:
        raise ValueError("absorb_h1e needs at least one electron")
    eri = restore_eri(eri, norb)
    ht = np.asarray(h1e, dtype=np.float64) - 0.5 * np.einsum("prrq->pq", eri)
    g = eri.copy()
    eye = np.eye(norb)
    g += (np.einsum("pq,rs->pqrs", ht, eye) + np.einsum("pq,rs->pqrs", eye, ht)) / n
    return g * fac


def _start_vectors(hdiag, n):
    """Davidson start space: unit vectors on the `n` determinants of lowest diagonal energy (degenerate ones kept together), each
    with 1 % of fixed pseudo-random noise.  Without the noise a start space that is closed under a symmetry of the Hamiltonian
    (orbital permutations, point group, spin flip) confines every later correction vector to the representations it happens to
    contain, and a low root of another one is never found; with it the residual of every Ritz vector carries all of them, at a
    size the convergence test sees."""
    import torch
    from .tdscf import initial_guess
    V = initial_guess(hdiag, n)
    gen = torch.Generator().manual_seed(20251017)
    noise = torch.randn(V.shape, generator=gen, dtype=torch.float64)
    noise /= torch.linalg.norm(noise, dim=1, keepdim=True)
    return V + 1e-2 * noise.to(V.device)


# =================================================================================================
# the solver
# =================================================================================================
class FCISolver:
    """`direct_spin1.FCISolver`-shaped solver.  `max_workspace_mb` bounds the D and F work arrays of one sigma / density-matrix
    chunk (default 16 GiB: three chunks for a 14-orbital, 14-electron space and ~250 GB left for its 94 MB vectors);
    `max_memory` (MB; None = 90 % of the device's memory) bounds work arrays plus CI vectors (`nroots`, the Davidson
    subspace V and H V of `max_space` vectors each, a few temporaries): a space that does not fit is refused."""
    nroots = 1
    conv_tol = 1e-10
    max_cycle = 100
    max_space = None          # None: max(40, 12 nroots), the Davidson's own default
    max_workspace_mb = 16384
    max_memory = None
    verbose = 0
    stdout = None
    profile = False           # True: synchronise around the three parts of sigma and add their seconds to `timing`

    def __init__(self, mol=None):
        self.mol = mol
        if mol is not None:
            self.verbose = getattr(mol, "verbose", 0)
            self.stdout = getattr(mol, "stdout", None)
        self.converged = None
        self.eci = None
        self.ci = None
        self.timing = {"gather_d": 0.0, "gemm": 0.0, "gather_sigma": 0.0, "sigma_calls": 0, "chunks": 0}
        self._tables = {}

    def _log(self, level, msg):
        if self.verbose >= level:
            (self.stdout or sys.stdout).write(msg + "\n")

    # ---- device plumbing ------------------------------------------------------------------------------------------------------
    @staticmethod
    def _device():
        import torch
        from . import engine
        engine.require_gpu()
        return torch.device("cuda", torch.cuda.current_device())

    def _tab(self, norb, nelec):
        import torch
        na, nb = _unpack_nelec(nelec)
        if not 1 <= norb <= MAX_NORB:
            raise NotImplementedError(f"FCI: norb = {norb}; the string masks and kernels hold 1..{MAX_NORB} orbitals")
        if not (0 <= na <= norb and 0 <= nb <= norb):
            raise ValueError(f"FCI: ({na}, {nb}) electrons do not fit in {norb} orbitals")
        dev = self._device()
        key = (norb, na, nb, dev.index)
        if key not in self._tables:
            astr, bstr = make_strings(norb, na), make_strings(norb, nb)
            la = link_table(norb, na)
            alink = np.stack([la[:, :, 1] * norb + la[:, :, 0], la[:, :, 3] * (la[:, :, 2] + 1)], axis=2).astype(np.int32)
            btab = dense_link_table(norb, nb)
            assert np.abs(btab).max(initial=0) <= len(bstr) and (alink.size == 0 or np.abs(alink[:, :, 1]).max() <= len(astr))
            T = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=torch.int32, device=dev)
            self._tables[key] = dict(norb=norb, na=na, nb=nb, nsa=len(astr), nsb=len(bstr), nla=alink.shape[1], dev=dev,
                                     alink=T(alink.reshape(-1) if alink.size else np.zeros(2)), btab=T(btab), astr=T(astr), bstr=T(bstr))
        return self._tables[key]

    @staticmethod
    def _stream(dev):
        import torch
        return ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

    def _vecs(self, tb, ci):
        """CI vector(s) (NumPy or torch, one [nsa, nsb] / flat vector or a stack) -> contiguous device tensor [nvec, nsa, nsb]."""
        import torch
        if isinstance(ci, (list, tuple)):
            ci = torch.stack([torch.as_tensor(np.asarray(c) if not torch.is_tensor(c) else c) for c in ci])
        v = torch.as_tensor(ci, dtype=torch.float64, device=tb["dev"])
        ndet = tb["nsa"] * tb["nsb"]
        if v.numel() % ndet:
            raise ValueError(f"CI vector of {v.numel()} elements for {tb['nsa']} x {tb['nsb']} determinants")
        return v.reshape(-1, tb["nsa"], tb["nsb"]).contiguous()

    def _chunks(self, tb, nvec, narrays=2):
        """(vectors per batch, alpha rows per chunk) that keep `narrays` work arrays below `max_workspace_mb`."""
        ld = tb["norb"] ** 2 + 1
        per_row = narrays * ld * tb["nsb"] * 8
        cap = int(self.max_workspace_mb * 2 ** 20)
        if per_row > cap:
            raise NotImplementedError(f"FCI: one alpha row of the work arrays needs {per_row / 2 ** 20:.1f} MB "
                                      f"({narrays} x {ld} planes x {tb['nsb']} beta strings), max_workspace_mb = {self.max_workspace_mb}")
        vb = min(nvec, cap // per_row)
        rows = min(tb["nsa"], cap // (per_row * vb))
        return vb, rows

    def _gather_d(self, tb, c, a0, nrow, mode=LINK_MODE_BOTH):
        import torch
        from . import engine
        nvec, ld = c.shape[0], tb["norb"] ** 2 + 1
        D = torch.empty((ld, nvec, nrow * tb["nsb"]), dtype=torch.float64, device=tb["dev"])
        with torch.cuda.device(tb["dev"]):
            engine._check(engine.lib().mi_fci_gather_d(c.data_ptr(), nvec, tb["nsa"], tb["nsb"], tb["norb"], a0, nrow,
                                                       tb["alink"].data_ptr(), tb["nla"], tb["btab"].data_ptr(), mode,
                                                       D.data_ptr(), self._stream(tb["dev"])))
        return D

    def _sigma(self, M, c, tb):
        """H c for the stack c [nvec, nsa, nsb] and the operator M [norb^2, norb^2 + 1] = [g_pqrs | t_pq]:
        sum g_pqrs E_pq E_rs + sum t_pq E_pq."""
        import time
        import torch
        from . import engine
        dev, nsa, nsb, n2 = tb["dev"], tb["nsa"], tb["nsb"], tb["norb"] ** 2
        out = torch.zeros_like(c)
        vb, rows = self._chunks(tb, c.shape[0])
        tm = self.timing
        tm["sigma_calls"] += 1

        def lap(key, t0):
            """Profile mode: wait for the device and book the seconds since t0 under `key` (None: just take the time)."""
            if not self.profile:
                return 0.0
            torch.cuda.synchronize(dev)
            t1 = time.perf_counter()
            if key:
                tm[key] += t1 - t0
            return t1

        for v0 in range(0, c.shape[0], vb):
            cv, ov = c[v0:v0 + vb], out[v0:v0 + vb]
            for a0 in range(0, nsa, rows):
                nrow = min(rows, nsa - a0)
                t = lap(None, 0.0)
                D = self._gather_d(tb, cv, a0, nrow)
                t = lap("gather_d", t)
                F = torch.mm(M, D.view(n2 + 1, -1))
                t = lap("gemm", t)
                with torch.cuda.device(dev):
                    engine._check(engine.lib().mi_fci_gather_sigma(F.data_ptr(), cv.shape[0], nsa, nsb, tb["norb"], a0, nrow,
                                                                   tb["alink"].data_ptr(), tb["nla"], tb["btab"].data_ptr(),
                                                                   ov.data_ptr(), self._stream(dev)))
                lap("gather_sigma", t)
                tm["chunks"] += 1
                del D, F
        return out

    def _operator(self, h1e, eri, norb, dev):
        """M = [1/2 (pq|rs) | h~_pq] (device) and the host arrays (h1e, eri4)."""
        import torch
        h1 = np.asarray(h1e, dtype=np.float64).reshape(norb, norb)
        e4 = restore_eri(eri, norb)
        ht = h1 - 0.5 * np.einsum("prrq->pq", e4)
        M = np.concatenate([0.5 * e4.reshape(norb * norb, norb * norb), ht.reshape(-1, 1)], axis=1)
        return torch.as_tensor(M, dtype=torch.float64, device=dev).contiguous(), h1, e4

    def _hdiag(self, h1, e4, tb):
        import torch
        from . import engine
        dev, norb = tb["dev"], tb["norb"]
        T = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64, device=dev)
        jd, kd = T(np.einsum("ppqq->pq", e4)), T(np.einsum("pqqp->pq", e4))
        h = T(h1)
        out = torch.empty((tb["nsa"], tb["nsb"]), dtype=torch.float64, device=dev)
        with torch.cuda.device(dev):
            engine._check(engine.lib().mi_fci_hdiag(h.data_ptr(), jd.data_ptr(), kd.data_ptr(), norb, tb["astr"].data_ptr(), tb["nsa"],
                                                    tb["bstr"].data_ptr(), tb["nsb"], out.data_ptr(), self._stream(dev)))
        return out

    # ---- PySCF-shaped surface -------------------------------------------------------------------------------------------------
    absorb_h1e = staticmethod(absorb_h1e)

    def contract_2e(self, eri, fcivec, norb, nelec, **kw):
        """sum_pqrs eri[p,q,r,s] E_pq E_rs |fcivec> (PySCF: `eri` from `absorb_h1e(h1e, eri, norb, nelec, .5)` makes this H c).
        One vector [nsa, nsb] or a stack [nvec, nsa, nsb]; returns a NumPy array of the same shape."""
        import torch
        tb = self._tab(norb, nelec)
        e4 = restore_eri(eri, norb)
        M = np.concatenate([e4.reshape(norb * norb, -1), np.zeros((norb * norb, 1))], axis=1)
        c = self._vecs(tb, fcivec)
        s = self._sigma(torch.as_tensor(M, dtype=torch.float64, device=tb["dev"]).contiguous(), c, tb)
        return s.cpu().numpy().reshape(np.shape(fcivec) if not isinstance(fcivec, (list, tuple)) else s.shape)

    def contract_h(self, h1e, eri, fcivec, norb, nelec):
        """H c with H = sum h_pq E_pq + 1/2 sum (pq|rs) (E_pq E_rs - delta_qr E_ps): the product `kernel` iterates."""
        tb = self._tab(norb, nelec)
        M, _, _ = self._operator(h1e, eri, norb, tb["dev"])
        c = self._vecs(tb, fcivec)
        s = self._sigma(M, c, tb)
        return s.cpu().numpy().reshape(np.shape(fcivec) if not isinstance(fcivec, (list, tuple)) else s.shape)

    def make_hdiag(self, h1e, eri, norb, nelec):
        tb = self._tab(norb, nelec)
        h1 = np.asarray(h1e, dtype=np.float64).reshape(norb, norb)
        return self._hdiag(h1, restore_eri(eri, norb), tb).cpu().numpy().reshape(-1)

    def _check_memory(self, tb, nroots, n_guess):
        import torch
        ndet = tb["nsa"] * tb["nsb"]
        space = min(self.max_space or max(40, 12 * nroots), ndet)
        nvec = nroots + 2 * space + 4
        vec_mb = nvec * ndet * 8 / 2 ** 20
        work_mb = min(float(self.max_workspace_mb), 2 * (tb["norb"] ** 2 + 1) * ndet * 8 * max(n_guess, 1) / 2 ** 20)
        if self.max_memory is None:
            limit_mb = 0.9 * torch.cuda.mem_get_info(tb["dev"])[1] / 2 ** 20
        else:
            limit_mb = float(self.max_memory)
        if vec_mb + work_mb > limit_mb:
            raise NotImplementedError(
                f"FCI: ({tb['na']}, {tb['nb']}) electrons in {tb['norb']} orbitals = {ndet} determinants: {nvec} CI vectors "
                f"({nroots} roots + Davidson subspace 2 x {space} + 4) need {vec_mb:.1f} MB and the work arrays {work_mb:.1f} MB; "
                f"the limit is {limit_mb:.1f} MB (max_memory)")

    def kernel(self, h1e, eri, norb, nelec, ci0=None, ecore=0, nroots=None, **kw):
        import torch
        from .tdscf import davidson_tda
        nroots = int(nroots or self.nroots)
        tb = self._tab(norb, nelec)
        ndet = tb["nsa"] * tb["nsb"]
        nroots = min(nroots, ndet)
        n_guess = nroots if nroots == 1 else min(ndet, 4 * nroots)
        self._check_memory(tb, nroots, n_guess)
        M, h1, e4 = self._operator(h1e, eri, norb, tb["dev"])
        hd = self._hdiag(h1, e4, tb).reshape(-1)
        if ci0 is not None:
            guess = self._vecs(tb, ci0).reshape(-1, ndet)
        else:
            guess = _start_vectors(hd, n_guess)
        matvec = lambda V: self._sigma(M, V.reshape(-1, tb["nsa"], tb["nsb"]).contiguous(), tb).reshape(-1, ndet)
        w, X, conv = davidson_tda(matvec, hd, nroots, self.conv_tol, self.max_cycle, self.max_space, guess,
                                  log=(lambda m: self._log(4, "FCI " + m)))
        X = X / torch.linalg.norm(X, dim=1, keepdim=True)
        e = w.cpu().numpy() + float(ecore)
        civ = X.cpu().numpy().reshape(-1, tb["nsa"], tb["nsb"])
        conv = np.asarray(conv, dtype=bool)
        self._log(3, "FCI: " + ", ".join(f"E[{i}] = {e[i]:.12f}" for i in range(len(e))) + f"  converged {conv.tolist()}")
        if nroots > 1:
            self.eci, self.ci, self.converged = e, [c for c in civ], conv
        else:
            self.eci, self.ci, self.converged = float(e[0]), civ[0], bool(conv[0])
        return self.eci, self.ci

    # ---- density matrices and spin --------------------------------------------------------------------------------------------
    def _rdm_raw(self, cibra, ciket, norb, nelec, with_2=True):
        """E1[r,s] = <bra|E_rs|ket> and (with_2) EE[p,q,r,s] = <bra|E_pq E_rs|ket> as NumPy arrays."""
        import torch
        tb = self._tab(norb, nelec)
        n2 = norb * norb
        ket = self._vecs(tb, ciket)
        bra = ket if cibra is ciket else self._vecs(tb, cibra)
        if ket.shape[0] != 1 or bra.shape[0] != 1:
            raise ValueError("density matrices take one CI vector per state")
        _, rows = self._chunks(tb, 1)
        A = torch.zeros((n2 + 1, n2) if with_2 else (n2,), dtype=torch.float64, device=tb["dev"])
        for a0 in range(0, tb["nsa"], rows):
            nrow = min(rows, tb["nsa"] - a0)
            Dk = self._gather_d(tb, ket, a0, nrow).view(n2 + 1, -1)
            if with_2:
                Db = Dk if bra is ket else self._gather_d(tb, bra, a0, nrow).view(n2 + 1, -1)
                A += Db @ Dk[:n2].T
            else:
                A += Dk[:n2] @ bra[0, a0:a0 + nrow].reshape(-1)
        A = A.cpu().numpy()
        if not with_2:
            return A.reshape(norb, norb), None
        E1 = A[n2].reshape(norb, norb)
        EE = A[:n2].reshape(norb, norb, norb, norb).transpose(1, 0, 2, 3)   # row index of A is (q, p): <K|E_qp|bra> = <bra|E_pq|K>
        return E1, EE

    def trans_rdm1(self, cibra, ciket, norb, nelec, **kw):
        """dm1[p,q] = <bra| a+_q a_p |ket>, spin-summed (PySCF's convention)."""
        return self._rdm_raw(cibra, ciket, norb, nelec, with_2=False)[0].T.copy()

    def make_rdm1(self, fcivec, norb, nelec, **kw):
        return self.trans_rdm1(fcivec, fcivec, norb, nelec)

    def trans_rdm12(self, cibra, ciket, norb, nelec, **kw):
        """(dm1, dm2) with dm2[p,q,r,s] = <bra| a+_p a+_r a_s a_q |ket>, spin-summed; for bra = ket
        E = sum h_pq dm1[p,q] + 1/2 sum (pq|rs) dm2[p,q,r,s]."""
        E1, EE = self._rdm_raw(cibra, ciket, norb, nelec, with_2=True)
        dm2 = EE.copy()
        for q in range(norb):
            dm2[:, q, q, :] -= E1            # E_pq E_rs = delta_qr E_ps + a+_p a+_r a_s a_q
        return E1.T.copy(), dm2

    def make_rdm12(self, fcivec, norb, nelec, **kw):
        return self.trans_rdm12(fcivec, fcivec, norb, nelec)

    def spin_square(self, fcivec, norb, nelec):
        """(<S^2>, 2S + 1) of one vector: S^2 = S_z (S_z + 1) + N_beta - sum_pq E^alpha_pq E^beta_qp."""
        import torch
        tb = self._tab(norb, nelec)
        c = self._vecs(tb, fcivec)
        if c.shape[0] != 1:
            raise ValueError("spin_square takes one CI vector")
        n2 = norb * norb
        _, rows = self._chunks(tb, 1)
        x = torch.zeros((), dtype=torch.float64, device=tb["dev"])
        for a0 in range(0, tb["nsa"], rows):
            nrow = min(rows, tb["nsa"] - a0)
            Da = self._gather_d(tb, c, a0, nrow, LINK_MODE_ALPHA)
            Db = self._gather_d(tb, c, a0, nrow, LINK_MODE_BETA)
            x += torch.sum(Da[:n2] * Db[:n2])
        norm = float(torch.sum(c * c))
        sz = 0.5 * (tb["na"] - tb["nb"])
        ss = sz * (sz + 1.0) + tb["nb"] - float(x) / norm
        s = np.sqrt(abs(ss) + 0.25) - 0.5
        return ss, 2.0 * s + 1.0

    def large_ci(self, fcivec, norb, nelec, tol=0.1, return_strs=True):
        """[(coefficient, alpha string, beta string)] of the determinants with |coefficient| > tol; strings as `bin()` text
        (return_strs) or as lists of occupied orbitals."""
        na, nb = _unpack_nelec(nelec)
        astr, bstr = make_strings(norb, na), make_strings(norb, nb)
        c = np.asarray(fcivec, dtype=np.float64).reshape(len(astr), len(bstr))
        ia, ib = np.nonzero(np.abs(c) > tol)
        fmt = (lambda s: bin(int(s))) if return_strs else (lambda s: [p for p in range(norb) if (int(s) >> p) & 1])
        return [(float(c[i, j]), fmt(astr[i]), fmt(bstr[j])) for i, j in zip(ia, ib)]

    def energy(self, h1e, eri, fcivec, norb, nelec):
        c = np.asarray(fcivec, dtype=np.float64)
        return float(np.sum(c * self.contract_h(h1e, eri, c, norb, nelec)) / np.sum(c * c))


def FCI(mol_or_mf=None, mo=None, singlet=False):
    """`fci.FCI(mol)`: a bare solver.  `fci.FCI(mf)`: a solver whose `kernel()` without arguments runs the full CI of the
    converged RHF `mf` in all its orbitals (through `casci.CASCI` with no core and every orbital active: at most 16 orbitals)."""
    if mol_or_mf is None or not hasattr(mol_or_mf, "mo_coeff"):
        return FCISolver(mol_or_mf)
    return _SCFBoundSolver(mol_or_mf, mo)


class _SCFBoundSolver(FCISolver):
    def __init__(self, mf, mo=None):
        super().__init__(mf.mol)
        self._scf, self._mo = mf, mo

    def kernel(self, h1e=None, eri=None, norb=None, nelec=None, **kw):
        if h1e is not None:
            return super().kernel(h1e, eri, norb, nelec, **kw)
        from .casci import CASCI
        mf = self._scf
        if mf.mo_coeff is None:
            mf.kernel()
        mc = CASCI(mf, np.asarray(mf.mo_coeff).shape[1], mf.mol.nelectron, ncore=0)
        mc.fcisolver = self        # the driver calls kernel(h1e, eri, ...): the plain solver above
        return mc.kernel(self._mo)[0], self.ci
