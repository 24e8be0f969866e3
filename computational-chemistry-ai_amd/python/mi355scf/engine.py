"""ctypes binding of the gfx950 engine library (`include/mi355scf.h`) on PyTorch-ROCm tensors.

PyTorch is plumbing here: it owns device memory for the N x N matrices, the current HIP stream and
(in `parallel.py`) the RCCL process group.  All hot-path arithmetic happens inside
`libmi355scf.so`.  There is NO CPU fallback: if the library or a GPU is missing this module raises.
"""
import ctypes
import os

import numpy as np
import torch  # must be imported before the engine library so both share one HIP runtime (libamdhip64.so.7)

_HERE = os.path.dirname(os.path.abspath(__file__))
_CSRC = os.path.normpath(os.path.join(_HERE, "..", "..", "csrc"))
LIB_PATH = os.path.join(_CSRC, "libmi355scf.so")
_lib = None


class EngineError(RuntimeError):
    pass


class EngineOutOfMemory(EngineError):
    """`mi_eri_prepare` returned MI_ERR_NOMEM: this rank's share of the tile store exceeds free HBM."""

    def __init__(self, msg, need_bytes, free_bytes):
        super().__init__(msg)
        self.need_bytes, self.free_bytes = need_bytes, free_bytes


MI_ERR_NOMEM = -2


class _Stats(ctypes.Structure):
    _fields_ = [("n_tiles", ctypes.c_int64), ("n_runs", ctypes.c_int64), ("stored_bytes", ctypes.c_int64),
                ("n_unique_eri", ctypes.c_int64), ("n_quartets", ctypes.c_int64), ("seconds_eri", ctypes.c_double)]


def build_library(force=False):
    """Compile csrc/ for gfx950 in-tree (hipcc cross-compiles without a GPU)."""
    import subprocess
    src = os.path.join(_CSRC, "mi355scf.hip")
    stale = (not os.path.exists(LIB_PATH)) or any(
        os.path.getmtime(os.path.join(_CSRC, f)) > os.path.getmtime(LIB_PATH)
        for f in ("mi355scf.hip", "rys_tables.h", "fci_kernels.h", "cc_kernels.h", "Makefile") if os.path.exists(os.path.join(_CSRC, f)))
    if force or stale:
        subprocess.check_call(["make", "-C", _CSRC, "-s"] + (["-B"] if force else []))
    return LIB_PATH


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise EngineError(f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                              "(this engine has no CPU fallback)")
        L = ctypes.CDLL(LIB_PATH)
        L.mi_last_error.restype = ctypes.c_char_p
        vp, ip, dp = ctypes.c_void_p, ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_double)
        L.mi_ctx_create.argtypes = [ip, ctypes.c_int, ip, ctypes.c_int, dp, ctypes.c_int, ctypes.c_int, ctypes.POINTER(vp)]
        L.mi_ctx_destroy.argtypes = [vp]
        L.mi_ctx_destroy.restype = None
        L.mi_ctx_nao.argtypes = [vp]
        L.mi_release_cache.restype = None
        L.mi_set_option.argtypes = [vp, ctypes.c_char_p, ctypes.c_double]
        L.mi_int1e.argtypes = [vp, vp, vp, vp, vp, dp, vp]
        L.mi_eri_prepare.argtypes = [vp, ctypes.c_double, ctypes.c_int, ctypes.c_int, vp]
        L.mi_eri_get_stats.argtypes = [vp, ctypes.POINTER(_Stats)]
        L.mi_build_jk.argtypes = [vp, vp, ctypes.c_int, vp, vp, vp]
        L.mi_jk_describe.argtypes = [vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_char_p, ctypes.c_size_t]
        L.mi_build_jk_multi.argtypes = [vp, vp, ctypes.c_int, ip, vp, vp, vp]
        L.mi_eri_unpack.argtypes = [vp, vp, vp]
        L.mi_eri_qtrans.argtypes = [vp, vp, ctypes.c_int, ctypes.c_int, vp, vp]
        L.mi_eri_active_j.argtypes = [vp, vp, ctypes.c_int, ctypes.c_int, vp, vp]
        L.mi_time_jk_kernel.argtypes = [vp, vp, ctypes.c_int, dp, vp]
        L.mi_time_jk_variant.argtypes = [vp, vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, dp, vp]
        L.mi_diis_errvec.argtypes = [vp, vp, vp, vp]
        L.mi_diis_combine.argtypes = [vp, vp, dp, ctypes.c_int, vp, vp]
        L.mi_diis_dots.argtypes = [vp, vp, vp, ctypes.c_int, dp, vp]
        L.mi_diis_dots_dev.argtypes = [vp, vp, vp, ctypes.c_int, vp, vp]
        L.mi_xc_rho_mo.argtypes = [vp, vp, ctypes.c_int, ctypes.c_int64, ctypes.c_int, vp, vp, vp]
        L.mi_xc_rho_lowrank.argtypes = [vp, vp, vp, ctypes.c_int, ctypes.c_int64, ctypes.c_int, vp, vp, vp]
        L.mi_diis_dots_dev_n.argtypes = [vp, vp, vp, ctypes.c_int, ctypes.c_int64, vp, vp]
        L.mi_diis_combine_dev_n.argtypes = [vp, vp, vp, ctypes.c_int, ctypes.c_int64, vp, vp]
        L.mi_diis_solve.argtypes = [vp, vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, vp, vp, vp]
        L.mi_diis_combine_dev.argtypes = [vp, vp, vp, ctypes.c_int, vp, vp]
        i64 = ctypes.c_int64
        L.mi_grid_becke.argtypes = [vp, vp, vp, vp, i64, vp, vp, vp]
        L.mi_grid_becke_grad.argtypes = [vp, vp, vp, vp, vp, i64, vp, vp, vp]
        L.mi_eval_ao.argtypes = [vp, vp, i64, ctypes.c_int, vp, vp]
        L.mi_xc_rho.argtypes = [vp, vp, vp, i64, ctypes.c_int, vp, vp]
        L.mi_xc_eval.argtypes = [ip, dp, ctypes.c_int, vp, vp, i64, ctypes.c_int, vp, vp, vp, vp, vp]
        L.mi_xc_eval_spin.argtypes = [ip, dp, ctypes.c_int, vp, vp, vp, i64, ctypes.c_int, vp, vp, vp, vp]
        L.mi_xc_eval_p.argtypes = [ip, dp, dp, ctypes.c_int, vp, vp, i64, ctypes.c_int, vp, vp, vp, vp, vp]
        L.mi_xc_eval_spin_p.argtypes = [ip, dp, dp, ctypes.c_int, vp, vp, vp, i64, ctypes.c_int, vp, vp, vp, vp]
        L.mi_xc_aow.argtypes = [vp, vp, vp, i64, ctypes.c_int, vp, vp]
        L.mi_xc_fxc_prep.argtypes = [ip, dp, dp, ctypes.c_int, vp, vp, i64, ctypes.c_int, ctypes.c_int, vp, vp]
        L.mi_xc_fxc_apply.argtypes = [vp, vp, vp, ctypes.c_int, i64, ctypes.c_int, vp, vp]
        L.mi_xc_eval_mgga.argtypes = [ip, dp, ctypes.c_int, vp, vp, vp, i64, vp, vp, vp]
        L.mi_xc_eval_mgga_spin.argtypes = [ip, dp, ctypes.c_int, vp, vp, vp, vp, vp, i64, vp, vp, vp, vp]
        L.mi_xc_vmat.argtypes = [vp, vp, vp, i64, vp, vp]
        L.mi_xc_vmat_fold.argtypes = [vp, vp, vp, i64, ctypes.c_int, vp, vp]
        L.mi_nystrom_warm.argtypes = [vp, vp, vp, vp, vp, ctypes.c_int, ctypes.c_int, vp]
        L.mi_xc_tail.argtypes = [vp, vp, vp, vp, vp, i64, vp, vp]
        L.mi_build_fock.argtypes = [vp, vp, vp, vp, ctypes.c_int, ctypes.c_double, vp, vp, vp]
        L.mi_nystrom_factor.argtypes = [vp, vp, vp, ctypes.c_int, ctypes.c_int, vp, vp, vp]
        L.mi_sp2_init.argtypes = [vp, vp, vp, vp, vp]
        L.mi_sp2_update.argtypes = [vp, vp, vp, ctypes.c_double, vp, vp]
        L.mi_sp2_iterate.argtypes = [vp, vp, vp, ctypes.c_int, ctypes.c_double, ctypes.c_int, vp, vp, ctypes.POINTER(vp), vp]
        L.mi_sp2_iterate_pingpong.argtypes = [vp, vp, vp, ctypes.c_int, ctypes.c_double, vp, ctypes.POINTER(vp), ctypes.POINTER(vp), vp]
        L.mi_sp2_iterate_planned.argtypes = [vp, vp, vp, vp, ctypes.c_int, dp, ctypes.c_double, vp, ctypes.POINTER(vp), ctypes.POINTER(vp), vp]
        L.mi_grad_1e.argtypes = [vp, vp, vp, vp, vp]
        L.mi_grad_eri.argtypes = [vp, vp, ctypes.c_double, vp, vp]
        L.mi_grad_eri_spin.argtypes = [vp, vp, vp, ctypes.c_double, vp, vp]
        L.mi_grad_eri_sharded.argtypes = [vp, vp, vp, ctypes.c_double, vp, ctypes.c_int, ctypes.c_int, vp]
        L.mi_grad_eri_pairs.argtypes = [vp, vp, vp, ctypes.c_double, vp, dp, ctypes.c_int, vp, ctypes.c_int, ctypes.c_int, vp]
        L.mi_grad_eri_xpairs.argtypes = [vp, vp, vp, ctypes.c_double, vp, dp, ctypes.c_int, vp, dp, ctypes.POINTER(ctypes.c_int), ctypes.c_int,
                                         vp, ctypes.c_int, ctypes.c_int, vp]
        L.mi_eri_get_memory.argtypes = [vp, ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int64)]
        L.mi_eri_release.argtypes = [vp]
        L.mi_tile_store_allocations.restype = ctypes.c_int64
        L.mi_tile_store_allocations.argtypes = [ctypes.c_int64]
        L.mi_eri_read_quartet.argtypes = [vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, dp]
        L.mi_schwarz_get.argtypes = [vp, dp]
        L.mi_df_build.argtypes = [vp, vp, vp, vp, vp]
        L.mi_df_grad.argtypes = [vp, vp, vp, vp, vp, ctypes.c_int, ctypes.c_int, vp]
        L.mi_reduce_blocks.argtypes = [vp]
        L.mi_plan_shards.argtypes = [ctypes.c_int, dp, ctypes.c_double, ctypes.c_int, ctypes.POINTER(ctypes.c_int64),
                                     ctypes.POINTER(ctypes.c_int64)]
        L.mi_fock_energy.argtypes = [vp, vp, vp, vp, vp, vp, ctypes.c_double, vp, vp, vp]
        L.mi_commutator_norm.argtypes = [vp, vp, vp, vp, vp]
        L.mi_c2s_table.argtypes = [ctypes.c_int, dp]
        L.mi_rys_roots_host.argtypes = [ctypes.c_int, ctypes.c_double, dp, dp]
        L.mi_pcm_pairs.argtypes = [vp, ctypes.c_int, ip]
        L.mi_pcm_eval.argtypes = [vp, vp, ctypes.c_int, vp, ctypes.c_int, i64, vp, vp]
        L.mi_pcm_grad.argtypes = [vp, vp, ctypes.c_int, vp, ctypes.c_int, vp, vp, vp, vp]
        L.mi_pcm_potential.argtypes = [vp, vp, ctypes.c_int, i64, vp, vp, vp, vp, vp]
        L.mi_pcm_fock_chunks.argtypes = [ctypes.c_int, i64]
        L.mi_pcm_fock.argtypes = [vp, vp, ctypes.c_int, i64, vp, ctypes.c_double, ctypes.c_int, vp, vp, vp]
        L.mi_pc_fock_chunks.argtypes = [ctypes.c_int, i64]
        L.mi_pc_fock.argtypes = [vp, vp, vp, ctypes.c_int, ctypes.c_double, ctypes.c_int, vp, vp, vp]
        L.mi_pc_grad_work.restype = i64
        L.mi_pc_grad_work.argtypes = [vp, ctypes.c_int]
        L.mi_pc_grad.argtypes = [vp, vp, vp, ctypes.c_int, vp, vp, vp, vp, vp]
        ci = ctypes.c_int
        L.mi_fci_gather_d.argtypes = [vp, ci, ci, ci, ci, ci, ci, vp, ci, vp, ci, vp, vp]
        L.mi_fci_gather_sigma.argtypes = [vp, ci, ci, ci, ci, ci, ci, vp, ci, vp, vp, vp]
        L.mi_fci_hdiag.argtypes = [vp, vp, vp, ci, vp, ci, vp, ci, vp, vp]
        L.mi_cc_amp_update.argtypes = [vp, vp, vp, vp, vp, vp, vp, ci, ci, vp, vp, vp]
        L.mi_cc_t_blocks.argtypes = [ci]
        L.mi_cc_t_energy.argtypes = [vp, ci, ci, ci, vp, vp, vp, vp, vp, vp, vp, vp, vp]
        L.mi_rohf_fock.argtypes = [vp, vp, i64, ci, ci, ci, vp, vp, vp, vp]
        _lib = L
    return _lib


def plan_shards(nao, qblk, tol, nranks):
    """Host-only sharding plan (no GPU needed): (bytes per rank, runs per rank) for a block-pair Schwarz table."""
    q = np.ascontiguousarray(qblk, dtype=np.float64)
    b = np.zeros(nranks, dtype=np.int64)
    r = np.zeros(nranks, dtype=np.int64)
    i64p = ctypes.POINTER(ctypes.c_int64)
    _check(lib().mi_plan_shards(int(nao), _dp(q), float(tol), int(nranks), b.ctypes.data_as(i64p), r.ctypes.data_as(i64p)))
    return b, r


def tile_store_allocations(min_bytes=0):
    """Fresh device allocations of tile stores >= `min_bytes` made by this process (reuse of a parked store does not count)."""
    return int(lib().mi_tile_store_allocations(int(min_bytes)))


def release_cache():
    """Free tile stores parked by destroyed contexts (kept for reuse across geometry steps)."""
    lib().mi_release_cache()


def _check(rc):
    if rc != 0:
        raise EngineError(lib().mi_last_error().decode())


def _dp(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))


def require_gpu():
    if not torch.cuda.is_available():
        raise EngineError("no MI355X/HIP device visible: the SCF engine runs on the GPU only (no CPU fallback)")


def c2s_table(l):
    out = np.zeros(((l + 1) * (l + 2) // 2, 2 * l + 1))
    _check(lib().mi_c2s_table(l, _dp(out)))
    return out


def rys_roots(n, x):
    r, w = np.zeros(n), np.zeros(n)
    _check(lib().mi_rys_roots_host(n, float(x), _dp(r), _dp(w)))
    return r, w


XPAIRS_MAX = 8


def _term_matrices(name, A, K, nao, device):
    """ValueError unless A holds the K matrices of the `pairs` / `xpairs` argument as the C entry point reads them."""
    if K > 0 and not (torch.is_tensor(A) and A.dtype == torch.float64 and A.device == torch.device(device) and A.is_contiguous()
                      and tuple(A.shape) == (K, nao, nao)):
        raise ValueError(f"grad_eri: {name} needs a contiguous float64 [{K}, {nao}, {nao}] tensor on {device}")


def xpairs_args(xpairs, nao, device):
    """(R, t [Kx] float64, sym [Kx] intc, Kx) of the `xpairs` argument of `Engine.grad_eri`, or ValueError: what the C entry point
    cannot see of a device tensor (shape, type, contiguity, device), and what it refuses itself, before any launch."""
    try:
        R, t, sym = xpairs
    except (TypeError, ValueError):
        raise ValueError("grad_eri: xpairs must be (R, t, sym)") from None
    t = np.ascontiguousarray(np.asarray(t, dtype=np.float64).ravel())
    sym = np.asarray(sym).ravel()
    Kx = int(t.size)
    if Kx > XPAIRS_MAX:
        raise ValueError(f"grad_eri: xpairs takes at most {XPAIRS_MAX} matrices, got {Kx}")
    if sym.size != Kx:
        raise ValueError(f"grad_eri: xpairs has {Kx} weights and {sym.size} symmetry flags")
    if not np.all(np.isfinite(t)):
        raise ValueError("grad_eri: xpairs weights must be finite")
    if not all(v == 1 or v == -1 for v in sym.tolist()):
        raise ValueError(f"grad_eri: xpairs symmetry flags must be +1 (symmetric) or -1 (antisymmetric), got {sym.tolist()}")
    _term_matrices("xpairs", R, Kx, nao, device)
    return R, t, np.ascontiguousarray(sym.astype(np.intc)), Kx


class Engine:
    """One engine context = one molecule/basis on one GPU (rows a2-a6, a10 of SURVEY.md section 8)."""

    def __init__(self, mol, device=None):
        require_gpu()
        self.mol = mol
        if device is None:
            device = torch.cuda.current_device()
        self.device = torch.device("cuda", device if isinstance(device, int) else device.index)
        _warm_libraries(self.device, mol.nao, max(1, int(getattr(mol, "nelectron", 48)) // 2))
        self._atm = np.ascontiguousarray(mol._atm, dtype=np.int32)
        self._bas = np.ascontiguousarray(mol._bas, dtype=np.int32)
        self._env = np.ascontiguousarray(mol._env, dtype=np.float64)
        self.nao = mol.nao
        h = ctypes.c_void_p()
        ip = ctypes.POINTER(ctypes.c_int32)
        _check(lib().mi_ctx_create(self._atm.ctypes.data_as(ip), len(self._atm), self._bas.ctypes.data_as(ip),
                                   len(self._bas), _dp(self._env), len(self._env), self.device.index, ctypes.byref(h)))
        self._h = h
        self.eri_ready = False

    def __del__(self):
        try:
            if getattr(self, "_h", None):
                lib().mi_ctx_destroy(self._h)
                self._h = None
        except Exception:
            pass

    close = __del__

    def set_option(self, key, value):
        _check(lib().mi_set_option(self._h, key.encode(), float(value)))

    def _stream(self):
        return ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _new(self, *shape):
        return torch.empty(*shape, dtype=torch.float64, device=self.device)

    # --- row a2 ------------------------------------------------------------------------------
    def int1e(self, with_dipole=False, origin=None):
        n = self.nao
        S, T, V = self._new(n, n), self._new(n, n), self._new(n, n)
        dip = self._new(3, n, n) if with_dipole else None
        org = np.zeros(3) if origin is None else np.ascontiguousarray(origin, dtype=np.float64)
        with torch.cuda.device(self.device):
            _check(lib().mi_int1e(self._h, S.data_ptr(), T.data_ptr(), V.data_ptr(),
                                  dip.data_ptr() if dip is not None else None, _dp(org), self._stream()))
        return (S, T, V, dip) if with_dipole else (S, T, V)

    # --- rows a3, a4 ---------------------------------------------------------------------------
    def prepare_eri(self, tol=1e-13, rank=0, nranks=1):
        with torch.cuda.device(self.device):
            rc = lib().mi_eri_prepare(self._h, float(tol), int(rank), int(nranks), self._stream())
        if rc == MI_ERR_NOMEM:
            self.eri_ready = False
            need, free = self.eri_memory()
            raise EngineOutOfMemory(lib().mi_last_error().decode(), need, free)
        _check(rc)
        self.eri_ready = True
        return self.stats()

    def release_eri(self):
        """Drop the resident tile store (parked for reuse) and the pair data of the last `prepare_eri`."""
        _check(lib().mi_eri_release(self._h))
        self.eri_ready = False

    def eri_memory(self):
        """(bytes the last prepare_eri needed, free HBM bytes it saw)."""
        need, free = ctypes.c_int64(), ctypes.c_int64()
        _check(lib().mi_eri_get_memory(self._h, ctypes.byref(need), ctypes.byref(free)))
        return need.value, free.value

    def schwarz(self):
        """q[nbas, nbas] = sqrt(max |(ab|ab)|) of the shell pairs kept by prepare_eri (0: dropped)."""
        q = np.zeros((len(self._bas), len(self._bas)))
        _check(lib().mi_schwarz_get(self._h, _dp(q)))
        return q

    def eri_read_quartet(self, i, j, k, l):
        """(ij|kl) shell block read back from the resident tiles (tests): NumPy [di,dj,dk,dl]."""
        d = [2 * int(self._bas[s_, 1]) + 1 for s_ in (i, j, k, l)]
        out = np.zeros(d)
        _check(lib().mi_eri_read_quartet(self._h, int(i), int(j), int(k), int(l), _dp(out)))
        return out

    def stats(self):
        s = _Stats()
        _check(lib().mi_eri_get_stats(self._h, ctypes.byref(s)))
        return {k: getattr(s, k) for k, _ in _Stats._fields_}

    # --- rows a5, a6 ---------------------------------------------------------------------------
    def get_jk(self, dm, with_j=True, with_k=True, out_j=None, out_k=None):
        """J, K for one [N,N] or several [n_dm,N,N] densities.  `out_j` / `out_k`: contiguous device tensors of the result
        shape to write into (views of a caller-owned buffer, e.g. the fused [J|K|Vxc|N|Exc] all-reduce buffer of RKS)."""
        if not self.eri_ready:
            self.prepare_eri()
        dm = torch.as_tensor(dm, dtype=torch.float64, device=self.device).contiguous()
        if out_j is not None or out_k is not None:
            assert (out_j is None or (out_j.is_contiguous() and out_j.shape == dm.shape)) and \
                   (out_k is None or (out_k.is_contiguous() and out_k.shape == dm.shape))
            with torch.cuda.device(self.device):
                _check(lib().mi_build_jk(self._h, dm.data_ptr(), 1 if dm.dim() == 2 else dm.shape[0],
                                         out_j.data_ptr() if (with_j and out_j is not None) else None,
                                         out_k.data_ptr() if (with_k and out_k is not None) else None, self._stream()))
            return (out_j if with_j else None), (out_k if with_k else None)
        squeeze = dm.dim() == 2
        if squeeze:
            dm = dm.unsqueeze(0)
        # J and K are views of ONE buffer so that a sharded run can all-reduce [J|K] in place with one collective
        buf = torch.empty((int(with_j) + int(with_k),) + tuple(dm.shape), dtype=torch.float64, device=self.device)
        J = buf[0] if with_j else None
        K = buf[int(with_j)] if with_k else None
        self.last_jk_buffer = buf
        with torch.cuda.device(self.device):
            _check(lib().mi_build_jk(self._h, dm.data_ptr(), dm.shape[0], J.data_ptr() if with_j else None,
                                     K.data_ptr() if with_k else None, self._stream()))
        if squeeze:
            J = J[0] if with_j else None
            K = K[0] if with_k else None
        return J, K

    def jk_describe(self, with_j=True, with_k=True, n_dm=1):
        """What `get_jk` would run on the current store and options (mi_jk_describe; nothing is launched): dict with `family`
        ("plain", "kjlt", "pipe", "pair") and the integers `nt`, `dpp`, `tri`, `waves`, `segments`, `n_jk_cached`."""
        buf = ctypes.create_string_buffer(256)
        _check(lib().mi_jk_describe(self._h, int(with_j), int(with_k), int(n_dm), buf, len(buf)))
        d = dict(f.split("=", 1) for f in buf.value.decode().split())
        return {k: (v if k == "family" else int(v)) for k, v in d.items()}

    def get_jk_multi(self, dms, sym, with_j=True, with_k=True):
        """J, K of a stack [n, N, N] of densities that are each symmetric (sym[m] = +1) or antisymmetric (-1), every resident
        tile read once per launch of up to `jk_multi_batch` densities (mi_build_jk_multi; default 8, at most 16).  J of an
        antisymmetric member is zero.  J / K is None when `with_j` / `with_k` is False (J only skips the exchange
        contractions).  Sharded engines return this rank's partial sums."""
        if not self.eri_ready:
            self.prepare_eri()
        dms = torch.as_tensor(dms, dtype=torch.float64, device=self.device).contiguous()
        assert dms.dim() == 3 and dms.shape[1] == dms.shape[2] == self.nao
        n = dms.shape[0]
        sym = [int(s) for s in sym]
        assert len(sym) == n and all(s in (1, -1) for s in sym), "sym: +1 or -1 per density"
        assert with_j or with_k
        J = torch.empty_like(dms) if with_j else None
        K = torch.empty_like(dms) if with_k else None
        if n == 0:
            return J, K
        s = (ctypes.c_int32 * n)(*sym)
        with torch.cuda.device(self.device):
            _check(lib().mi_build_jk_multi(self._h, dms.data_ptr(), n, s, J.data_ptr() if with_j else None,
                                           K.data_ptr() if with_k else None,
                                           self._stream()))
        return J, K

    def df_build(self, aux_engine, int3c, int2c):
        """(ij|P) -> int3c[nao, nao, naux], (P|Q) -> int2c[naux, naux]; `aux_engine`: context of the auxiliary basis whose last
        shell is the unit function (see `df.DF.build`)."""
        with torch.cuda.device(self.device):
            _check(lib().mi_df_build(self._h, aux_engine._h, int3c.data_ptr() if int3c is not None else None,
                                     int2c.data_ptr() if int2c is not None else None, self._stream()))

    def df_grad(self, aux_engine, z3, z2, grad, rank=0, nranks=1):
        """grad[natm, 3] += sum Z3[a, b, P] d(ab|P)/dX + sum Z2[P, Q] d(P|Q)/dX (this rank's share of the batches)."""
        for t in (z3, z2):
            if t is not None and not (t.is_contiguous() and t.dtype == torch.float64 and t.device == self.device):
                raise ValueError("df_grad: contiguous float64 tensors on the engine's device are required")
        n, na = self.nao, aux_engine.nao - 1
        if z3 is not None and tuple(z3.shape) != (n, n, na):
            raise ValueError(f"df_grad: Z3 must be [{n}, {n}, {na}]")
        if z2 is not None and tuple(z2.shape) != (na, na):
            raise ValueError(f"df_grad: Z2 must be [{na}, {na}]")
        if tuple(grad.shape) != (len(self._atm), 3) or not grad.is_contiguous() or grad.dtype != torch.float64:
            raise ValueError("df_grad: grad must be a contiguous float64 [natm, 3] tensor")
        with torch.cuda.device(self.device):
            _check(lib().mi_df_grad(self._h, aux_engine._h, z3.data_ptr() if z3 is not None else None,
                                    z2.data_ptr() if z2 is not None else None, grad.data_ptr(), int(rank), int(nranks), self._stream()))

    def eri_dense(self):
        """(ij|kl) as a dense [nao]*4 device tensor (small molecules only: 8 nao^4 bytes)."""
        if not self.eri_ready:
            self.prepare_eri()
        n = self.nao
        out = self._new(n, n, n, n)
        with torch.cuda.device(self.device):
            _check(lib().mi_eri_unpack(self._h, out.data_ptr(), self._stream()))
        return out

    @staticmethod
    def qtrans_batch():
        """Columns `eri_qtrans` transforms per pass over the store (more run as several passes)."""
        return int(lib().mi_eri_qtrans_batch())

    def eri_qtrans(self, C_batch, out=None):
        """Y[o, p, q, r] = sum_s C_batch[s, o] (s p|q r) from the resident tiles (mi_eri_qtrans): device tensor [nb, N, N, N],
        symmetric in (q, r).  `out`: contiguous [nb, N, N, N] device tensor to write into.  Unsharded resident store only."""
        if not self.eri_ready:
            self.prepare_eri()
        C = torch.as_tensor(C_batch, dtype=torch.float64, device=self.device)
        if C.dim() == 1:
            C = C[:, None]
        C = C.contiguous()
        n = self.nao
        if C.dim() != 2 or C.shape[0] != n:
            raise ValueError(f"eri_qtrans: C_batch must be [{n}, nb]")
        nb = C.shape[1]
        if out is None:
            out = self._new(nb, n, n, n)
        elif tuple(out.shape) != (nb, n, n, n) or not out.is_contiguous() or out.dtype != torch.float64 or out.device != self.device:
            raise ValueError(f"eri_qtrans: out must be a contiguous float64 [{nb}, {n}, {n}, {n}] tensor on the engine's device")
        if nb:
            with torch.cuda.device(self.device):
                _check(lib().mi_eri_qtrans(self._h, C.data_ptr(), nb, nb, out.data_ptr(), self._stream()))
        return out

    @staticmethod
    def active_pair_width():
        """Pairs `active_pair_j` finishes per pass over the store (more run as several passes)."""
        return int(lib().mi_eri_active_j_width())

    def active_pair_j(self, Ca):
        """Jp[vw, p, q] = sum_rs (pq|rs) Ca[r, v] Ca[s, w] for the pairs v >= w of the columns of Ca [N, ncas <= 16], packed as
        vw = v (v + 1) / 2 + w (mi_eri_active_j): device tensor [ncas (ncas + 1) / 2, N, N], exactly symmetric in (p, q).
        Unsharded resident store only."""
        if not self.eri_ready:
            self.prepare_eri()
        C = torch.as_tensor(Ca, dtype=torch.float64, device=self.device)
        if C.dim() == 1:
            C = C[:, None]
        C = C.contiguous()
        n = self.nao
        if C.dim() != 2 or C.shape[0] != n or not 1 <= C.shape[1] <= 16:
            raise ValueError(f"active_pair_j: Ca must be [{n}, ncas] with 1 <= ncas <= 16")
        nc = C.shape[1]
        out = self._new(nc * (nc + 1) // 2, n, n)
        with torch.cuda.device(self.device):
            _check(lib().mi_eri_active_j(self._h, C.data_ptr(), nc, nc, out.data_ptr(), self._stream()))
        return out

    def time_jk_kernel(self, dm, reps=20, with_j=True, with_k=True):
        dm = torch.as_tensor(dm, dtype=torch.float64, device=self.device).contiguous()
        ms = ctypes.c_double()
        with torch.cuda.device(self.device):
            _check(lib().mi_time_jk_variant(self._h, dm.data_ptr(), int(with_j), int(with_k), reps, ctypes.byref(ms),
                                            self._stream()))
        return ms.value

    # --- rows a7-a9 (DFT) ------------------------------------------------------------------------
    def becke_weights(self, coords, atom_of, vol, adjust):
        w = torch.empty_like(vol)
        _check(lib().mi_grid_becke(self._h, coords.data_ptr(), atom_of.data_ptr(), vol.data_ptr(), vol.numel(),
                                   adjust.data_ptr(), w.data_ptr(), self._stream()))
        return w

    def becke_weights_grad(self, coords, atom_of, vol, adjust, e, out=None):
        """out[natm, 3] += sum_g e_g vol_g d(P_o / sum_B P_B)/dR_C (mi_grid_becke_grad): the weight derivative of the
        quadrature sum_g w_g e_g with the points riding on their parent atoms; `e` is the unweighted energy density."""
        ng = vol.numel()
        if out is None:
            out = torch.zeros(self.mol.natm, 3, dtype=torch.float64, device=self.device)
        assert coords.is_contiguous() and coords.shape == (ng, 3) and atom_of.dtype == torch.int32 and atom_of.numel() == ng
        assert vol.is_contiguous() and e.is_contiguous() and e.numel() == ng and adjust.is_contiguous()
        assert out.is_contiguous() and out.shape == (self.mol.natm, 3) and out.dtype == torch.float64
        _check(lib().mi_grid_becke_grad(self._h, coords.data_ptr(), atom_of.data_ptr(), vol.data_ptr(), e.data_ptr(), ng,
                                        adjust.data_ptr(), out.data_ptr(), self._stream()))
        return out

    def eval_ao(self, coords, deriv=1, out=None):
        ng = coords.shape[0]
        if out is None:
            out = self._new({0: 1, 1: 4, 2: 10}[int(deriv)], self.nao, ng)
        _check(lib().mi_eval_ao(self._h, coords.data_ptr(), ng, int(deriv), out.data_ptr(), self._stream()))
        return out

    def xc_rho(self, ao, C, deriv=1, out=None):
        ng = ao.shape[-1]
        rho = self._new(4 if deriv else 1, ng) if out is None else out
        assert rho.is_contiguous() and rho.shape == (4 if deriv else 1, ng)
        _check(lib().mi_xc_rho(self._h, ao.data_ptr(), C.data_ptr(), ng, int(deriv), rho.data_ptr(), self._stream()))
        return rho

    def xc_rho_mo(self, psi, deriv=1, with_tau=False):
        """rho[(1|4)][ng] (and tau[ng]) from occupied-orbital values psi[(1|4)][nocc][ng] of a density D = Z Z^T."""
        ng, nocc = psi.shape[-1], psi.shape[-2]
        rho = self._new(4 if deriv else 1, ng)
        tau = self._new(ng) if with_tau else None
        _check(lib().mi_xc_rho_mo(self._h, psi.data_ptr(), nocc, ng, int(deriv), rho.data_ptr(),
                                  tau.data_ptr() if tau is not None else None, self._stream()))
        return (rho, tau) if with_tau else rho

    def xc_rho_lowrank(self, ao, Zp, deriv=1, with_tau=False):
        """rho[(1|4)][ng] (and tau[ng]) of D = Z Z^T straight from the AO values: Zp [nao, ldz] (zero-padded columns)."""
        ng = ao.shape[-1]
        assert Zp.is_contiguous() and Zp.shape[0] == self.nao
        rho = self._new(4 if deriv else 1, ng)
        tau = self._new(ng) if with_tau else None
        _check(lib().mi_xc_rho_lowrank(self._h, ao.data_ptr(), Zp.data_ptr(), Zp.shape[1], ng, int(deriv), rho.data_ptr(),
                                       tau.data_ptr() if tau is not None else None, self._stream()))
        return (rho, tau) if with_tau else rho

    @staticmethod
    def _xc_spec(terms, params=None):
        """terms [(coef, kind_id)] and params (one per term, or None) -> the (kinds, coefs, params-or-NULL, n) arguments of the
        mi_xc_* entry points, and the arrays behind them, which the caller holds until the call has returned."""
        kinds = np.array([k for _c, k in terms], dtype=np.int32)
        coefs = np.array([c for c, _k in terms], dtype=np.float64)
        prm = None if params is None else np.ascontiguousarray(params, dtype=np.float64)
        assert prm is None or prm.shape == (len(kinds),)
        args = (kinds.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), _dp(coefs), None if prm is None else _dp(prm), len(kinds))
        return args, (kinds, coefs, prm)

    def xc_eval_spin(self, terms, rhoa, rhob, weights, gga=True, params=None):
        """Spin-polarised functionals: (exc[ng], wva[(1|4)][ng], wvb[(1|4)][ng]).  `params`: one runtime parameter per term
        (the omega of a short-range B88 term, `dft.xc_params`), None for functionals without one."""
        ng = rhoa.shape[-1]
        exc = self._new(ng)
        wva = self._new(4 if gga else 1, ng)
        wvb = self._new(4 if gga else 1, ng)
        spec, _keep = self._xc_spec(terms, params)
        _check(lib().mi_xc_eval_spin_p(*spec, rhoa.data_ptr(), rhob.data_ptr(), weights.data_ptr(), ng, int(gga), exc.data_ptr(),
                                       wva.data_ptr(), wvb.data_ptr(), self._stream()))
        return exc, wva, wvb

    def xc_eval(self, terms, rho, weights, gga=True, want_raw=False, params=None):
        """terms: [(coef, kind_id)] -> (exc[ng], wv[(1|4)][ng]) (+ vrho, vsigma if want_raw).  `params` as in xc_eval_spin."""
        ng = rho.shape[-1]
        exc = self._new(ng)
        wv = self._new(4 if gga else 1, ng)
        vr = self._new(ng) if want_raw else None
        vs = self._new(ng) if want_raw else None
        spec, _keep = self._xc_spec(terms, params)
        _check(lib().mi_xc_eval_p(*spec, rho.data_ptr(), weights.data_ptr(), ng, int(gga), exc.data_ptr(), wv.data_ptr(),
                                  vr.data_ptr() if want_raw else None, vs.data_ptr() if want_raw else None, self._stream()))
        return (exc, wv, vr, vs) if want_raw else (exc, wv)

    def xc_fxc_prep(self, terms, rho, weights, gga=True, triplet=False, params=None):
        """XC response coefficients coef[(4|1)][ng] = w {f_rr, f_rs, f_ss, v_sigma} of the ground-state density rho (singlet:
        closed-shell functional; triplet: spin-difference kernel of the spin-polarised one).  `params` as in xc_eval."""
        ng = rho.shape[-1]
        assert rho.is_contiguous() and weights.is_contiguous() and rho.shape[0] == (4 if gga else 1)
        coef = self._new(4 if gga else 1, ng)
        spec, _keep = self._xc_spec(terms, params)
        _check(lib().mi_xc_fxc_prep(*spec, rho.data_ptr(), weights.data_ptr(), ng, int(bool(gga)), int(bool(triplet)),
                                    coef.data_ptr(), self._stream()))
        return coef

    def xc_fxc_apply(self, rho0, coef, rho1, gga=True):
        """wv1[m][(4|1)][ng] (the layout of xc_eval's wv) of m trial densities rho1[m][(4|1)][ng] from the coefficients of
        xc_fxc_prep and the ground-state density rho0 whose gradient they were made at."""
        m, nc, ng = rho1.shape
        assert nc == (4 if gga else 1) and coef.shape == (nc, ng) and rho0.shape[-1] == ng and rho0.shape[0] >= nc
        assert rho0.is_contiguous() and coef.is_contiguous() and rho1.is_contiguous()
        wv1 = self._new(m, nc, ng)
        _check(lib().mi_xc_fxc_apply(rho0.data_ptr(), coef.data_ptr(), rho1.data_ptr(), m, ng, int(bool(gga)), wv1.data_ptr(),
                                     self._stream()))
        return wv1

    def xc_tau(self, ao, dm):
        """tau[ng] = 1/2 sum_k sum_mu,nu D_mu,nu d_k phi_mu d_k phi_nu from AO gradients ao[1..3] (three D.ao_k GEMMs)."""
        tau = None
        for k in (1, 2, 3):
            t = (ao[k] * (dm @ ao[k])).sum(dim=0)
            tau = t if tau is None else tau + t
        return 0.5 * tau

    def xc_eval_mgga(self, terms, rho, tau, weights):
        """meta-GGA: (exc[ng], wv[5][ng]); wv[4] = w/4 de/dtau."""
        ng = rho.shape[-1]
        exc, wv = self._new(ng), self._new(5, ng)
        (kp, cp, _no_params, n), _keep = self._xc_spec(terms)
        _check(lib().mi_xc_eval_mgga(kp, cp, n, rho.data_ptr(), tau.data_ptr(), weights.data_ptr(), ng, exc.data_ptr(), wv.data_ptr(),
                                     self._stream()))
        return exc, wv

    def xc_eval_mgga_spin(self, terms, rhoa, rhob, taua, taub, weights):
        ng = rhoa.shape[-1]
        exc, wva, wvb = self._new(ng), self._new(5, ng), self._new(5, ng)
        (kp, cp, _no_params, n), _keep = self._xc_spec(terms)
        _check(lib().mi_xc_eval_mgga_spin(kp, cp, n, rhoa.data_ptr(), rhob.data_ptr(), taua.data_ptr(), taub.data_ptr(),
                                          weights.data_ptr(), ng, exc.data_ptr(), wva.data_ptr(), wvb.data_ptr(), self._stream()))
        return exc, wva, wvb

    def xc_tail(self, w, vals, tail):
        """tail[q] += dot(w, vals[q]) for up to three contiguous vectors, one launch, deterministic."""
        assert 1 <= len(vals) <= 3 and all(v.is_contiguous() and v.numel() == w.numel() for v in vals) and w.is_contiguous()
        assert tail.is_contiguous() and tail.numel() >= len(vals)
        p = [v.data_ptr() for v in vals] + [None] * (3 - len(vals))
        _check(lib().mi_xc_tail(self._h, w.data_ptr(), p[0], p[1], p[2], w.numel(), tail.data_ptr(), self._stream()))

    NYSTROM_MAX_OCC = 64

    def nystrom_factor(self, M, W, Zt=None, info=None):
        """(Zt [nocc, n] = R^-1 W^T, info) with M [nocc, nocc] = R R^T and W [n, nocc]: Cholesky factorisation and triangular
        solve in one launch (nocc <= NYSTROM_MAX_OCC)."""
        n, nocc = W.shape
        assert M.is_contiguous() and W.is_contiguous() and M.shape == (nocc, nocc) and nocc <= self.NYSTROM_MAX_OCC
        if Zt is None:
            Zt = self._new(nocc, n)
        if info is None:
            info = torch.empty((), dtype=torch.int32, device=self.device)
        _check(lib().mi_nystrom_factor(self._h, M.data_ptr(), W.data_ptr(), n, nocc, Zt.data_ptr(), info.data_ptr(), self._stream()))
        return Zt, info

    def nystrom_warm(self, Zt, info, G0, G):
        """G[n, nocc] = 0.05 G0 + Zt^T / |Zt[0]| if the factor Zt [nocc, n] is finite and `info` (int32 device scalar of
        cholesky_ex) is 0, else G0 -- one launch (dft.RKS._lowrank_factor)."""
        assert Zt.is_contiguous() and G0.is_contiguous() and G.is_contiguous() and info.dtype == torch.int32
        _check(lib().mi_nystrom_warm(self._h, Zt.data_ptr(), info.data_ptr(), G0.data_ptr(), G.data_ptr(), Zt.shape[0], Zt.shape[1],
                                     self._stream()))
        return G

    def xc_aow(self, ao, wv, gga=True):
        ng = ao.shape[-1]
        aow = self._new(self.nao, ng)
        _check(lib().mi_xc_aow(self._h, ao.data_ptr(), wv.data_ptr(), ng, int(gga), aow.data_ptr(), self._stream()))
        return aow

    def xc_vmat_fold(self, ao, wv, gga, vmat):
        """vmat += ao_0 . (sum_c wv_c ao_c)^T with the weighted AOs formed inside the kernel (no `xc_aow` pass)."""
        _check(lib().mi_xc_vmat_fold(self._h, ao.data_ptr(), wv.data_ptr(), ao.shape[-1], int(bool(gga)), vmat.data_ptr(), self._stream()))

    def xc_vmat(self, ao0, aow, vmat):
        _check(lib().mi_xc_vmat(self._h, ao0.data_ptr(), aow.data_ptr(), ao0.shape[-1], vmat.data_ptr(), self._stream()))

    # --- row a15: gradient pieces -----------------------------------------------------------------
    def grad_1e(self, D, W, grad):
        _check(lib().mi_grad_1e(self._h, D.data_ptr(), W.data_ptr(), grad.data_ptr(), self._stream()))

    def grad_eri(self, D, hyb, grad, spin_density=None, rank=0, nranks=1, pairs=None, xpairs=None):
        """D: total density; spin_density: Da - Db for UHF/UKS (None: closed shell); (rank, nranks): this process's share
        of the derivative-quartet batches (explicit: in direct mode the last prepare_eri split is a tile group, not a rank).
        pairs = (Q [K, N, N] device tensor of symmetric matrices, s [K]): the same pass with sum_k s_k Q^k_ab Q^k_cd added to
        every quartet's two-particle density (`mi_grad_eri_pairs`), i.e. plus the gradient of 1/2 sum_k s_k (Q^k|Q^k).
        xpairs = (R [Kx, N, N] device tensor, t [Kx], sym [Kx] of +1 / -1): the same pass with sum_m t_m (R^m_ac R^m_bd +
        R^m_ad R^m_bc) added as well (`mi_grad_eri_xpairs`), i.e. plus the gradient of sum_m t_m sum_ijkl (ik|jl) R^m_ij R^m_kl;
        R^m is symmetric (sym +1) or antisymmetric (-1) as declared, Kx <= 8.
        One C call serves all of it: an absent term is K = 0 / Kx = 0 of `mi_grad_eri_xpairs`."""
        R, t, sym, Kx = xpairs_args(xpairs if xpairs is not None else (None, (), ()), self.nao, D.device)
        Q, s = pairs if pairs is not None else (None, ())
        s = np.ascontiguousarray(np.asarray(s, dtype=np.float64).ravel())
        K = int(s.size)
        _term_matrices("pairs", Q, K, self.nao, D.device)
        if not self.eri_ready:
            self.prepare_eri()
        pd, pi = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int)
        _check(lib().mi_grad_eri_xpairs(self._h, D.data_ptr(), spin_density.data_ptr() if spin_density is not None else None, float(hyb),
                                        Q.data_ptr() if K > 0 else None, s.ctypes.data_as(pd) if K > 0 else None, K,
                                        R.data_ptr() if Kx > 0 else None, t.ctypes.data_as(pd) if Kx > 0 else None,
                                        sym.ctypes.data_as(pi) if Kx > 0 else None, Kx,
                                        grad.data_ptr(), int(rank), int(nranks), self._stream()))

    # --- C-PCM (pcm.py): surface-charge integrals and the two per-cycle passes over them -----------------------------------
    def pcm_pairs(self, ordered=False):
        """Shell pairs [n, 2] in the order of the rows of `pcm_grad`'s output (ordered: derivative on the first shell)."""
        n = lib().mi_pcm_pairs(self._h, int(bool(ordered)), None)
        _check(0 if n >= 0 else n)
        out = np.zeros((max(n, 1), 2), dtype=np.int32)
        lib().mi_pcm_pairs(self._h, int(bool(ordered)), out.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)))
        return out[:n]

    @staticmethod
    def _pcm_points(pts, blk):
        assert pts.is_contiguous() and pts.dtype == torch.float64 and pts.dim() == 2 and pts.shape[1] == 4
        assert blk.is_contiguous() and blk.dtype == torch.int32 and blk.dim() == 2 and blk.shape[1] == 3
        b = blk.cpu().numpy()
        assert b.shape[0] > 0 and (b[:, 1] >= 1).all() and (b[:, 1] <= 64).all() and (b[:, 0] >= 0).all() \
            and (b[:, 0] + b[:, 1] <= pts.shape[0]).all(), "point blocks must lie inside the point list (1..64 points each)"

    def pcm_eval(self, pts, blk, ld, B):
        """B[g, m(m+1)/2 + n] = (mn | erf(zeta_g r) / r at s_g) for pts [n, 4] = (x, y, z, zeta), blocks [nblk, 3]."""
        self._pcm_points(pts, blk)
        assert B.is_contiguous() and B.shape == (pts.shape[0], ld) and ld % 2 == 0 and ld >= self.nao * (self.nao + 1) // 2
        with torch.cuda.device(self.device):
            _check(lib().mi_pcm_eval(self._h, pts.data_ptr(), pts.shape[0], blk.data_ptr(), blk.shape[0], int(ld), B.data_ptr(),
                                     self._stream()))

    def pcm_grad(self, pts, blk, D, q, part):
        """part[pair (i, j), block, 3] = -2 sum_{g in block} q_g sum_{m in i, n in j} D_mn <d_A m|erf/r|n>_g for the pairs of
        `pcm_pairs(ordered=True)`: d_A = d/d(centre of shell i) of the bra function alone, D as given (not symmetrised)."""
        self._pcm_points(pts, blk)
        assert D.is_contiguous() and D.shape == (self.nao, self.nao) and q.is_contiguous() and q.numel() == pts.shape[0]
        assert part.is_contiguous() and part.numel() == len(self.pcm_pairs(True)) * blk.shape[0] * 3
        with torch.cuda.device(self.device):
            _check(lib().mi_pcm_grad(self._h, pts.data_ptr(), pts.shape[0], blk.data_ptr(), blk.shape[0], D.data_ptr(), q.data_ptr(),
                                     part.data_ptr(), self._stream()))

    def pcm_potential(self, B, ld, D, dpack, vn, v):
        """v = vn - B d (vn None: v = B d), d = D packed (m >= n, off-diagonals D_mn + D_nm) into `dpack` [ld]."""
        n = B.shape[0]
        assert B.is_contiguous() and B.shape[1] == ld and ld % 2 == 0 and ld >= self.nao * (self.nao + 1) // 2
        assert D.is_contiguous() and D.shape == (self.nao, self.nao) and dpack.numel() == ld and v.numel() == n
        assert vn is None or vn.numel() == n
        _check(lib().mi_pcm_potential(self._h, B.data_ptr(), n, int(ld), D.data_ptr(), dpack.data_ptr(),
                                      vn.data_ptr() if vn is not None else None, v.data_ptr(), self._stream()))

    @staticmethod
    def pcm_fock_chunks(npts, ld):
        return int(lib().mi_pcm_fock_chunks(int(npts), int(ld)))

    def pcm_fock(self, B, ld, q, scale, accumulate, part, V):
        """V (+)= scale sum_g q_g B_g unpacked to [nao, nao]; `part`: pcm_fock_chunks(npts, ld) * ld doubles of scratch."""
        n = B.shape[0]
        assert B.is_contiguous() and B.shape[1] == ld and ld % 2 == 0 and ld >= self.nao * (self.nao + 1) // 2
        assert q.is_contiguous() and q.numel() == n and V.is_contiguous() and V.shape == (self.nao, self.nao)
        assert part.numel() >= self.pcm_fock_chunks(n, ld) * ld
        _check(lib().mi_pcm_fock(self._h, B.data_ptr(), n, int(ld), q.data_ptr(), float(scale), int(bool(accumulate)),
                                 part.data_ptr(), V.data_ptr(), self._stream()))

    # --- point-charge embedding (qmmm.py): fused integral-and-contract passes over 10^4 .. 10^5 sites ------------------------
    @staticmethod
    def pc_fock_chunks(npts, ld):
        """Point chunks of `pc_fock` (its scratch is this many rows of ld doubles)."""
        return int(lib().mi_pc_fock_chunks(int(npts), int(ld)))

    def _pc_points(self, pts, q):
        assert pts.is_contiguous() and pts.dtype == torch.float64 and pts.dim() == 2 and pts.shape[1] == 4
        assert q.is_contiguous() and q.dtype == torch.float64 and q.numel() == pts.shape[0]
        if pts.shape[0] == 0:      # empty tensors have no address: any valid one serves, nothing is read through it
            pts = q = torch.zeros(4, dtype=torch.float64, device=q.device)
        return pts.data_ptr(), q.data_ptr()

    def pc_fock(self, pts, q, V, scale=1.0, accumulate=False, work=None):
        """V (+)= scale sum_k q_k (m| g_k |n) for the sites pts [n, 4] = (x, y, z, zeta) in Bohr: zeta <= 0 a point charge
        (g = 1/r), zeta > 0 a Gaussian one (g = erf(zeta r)/r).  `work`: pc_fock_chunks(n, ld) * ld doubles, ld the packed
        size nao (nao + 1) / 2 rounded up to even (allocated here when None)."""
        ppts, pq = self._pc_points(pts, q)
        assert V.is_contiguous() and V.dtype == torch.float64 and V.shape == (self.nao, self.nao)
        n = pts.shape[0]
        ld = self.nao * (self.nao + 1) // 2
        ld += ld & 1
        need = self.pc_fock_chunks(n, ld) * ld
        if work is None:
            work = torch.empty(need, dtype=torch.float64, device=self.device)
        assert work.is_contiguous() and work.numel() >= need
        with torch.cuda.device(self.device):
            _check(lib().mi_pc_fock(self._h, ppts, pq, n, float(scale), int(bool(accumulate)), work.data_ptr(),
                                    V.data_ptr(), self._stream()))
        return V

    def pc_grad_work(self, npts):
        n = int(lib().mi_pc_grad_work(self._h, int(npts)))
        _check(0 if n >= 0 else n)
        return n

    def pc_grad(self, pts, q, D, work=None, out=None):
        """(g_atoms [natm, 3], g_pts [n, 3]): the derivatives of sum_k q_k sum_mn D_mn (m| g_k |n) with respect to the basis
        centres and to the sites, for a symmetric D (the kernels put the derivative on the first shell of every ordered pair and
        double it).  `work`: pc_grad_work(n) doubles; `out`: the pair of output tensors (both allocated here when None)."""
        ppts, pq = self._pc_points(pts, q)
        assert D.is_contiguous() and D.dtype == torch.float64 and D.shape == (self.nao, self.nao)
        n = pts.shape[0]
        need = self.pc_grad_work(n)
        if work is None:
            work = torch.empty(max(need, 1), dtype=torch.float64, device=self.device)
        if out is None:
            out = (torch.empty(self.mol.natm, 3, dtype=torch.float64, device=self.device),
                   torch.empty(n, 3, dtype=torch.float64, device=self.device))
        ga, gp = out
        assert work.is_contiguous() and work.numel() >= need
        assert ga.is_contiguous() and ga.numel() == 3 * self.mol.natm and gp.is_contiguous() and gp.numel() == 3 * n
        with torch.cuda.device(self.device):
            _check(lib().mi_pc_grad(self._h, ppts, pq, n, D.data_ptr(), work.data_ptr(), ga.data_ptr(),
                                    gp.data_ptr() if n else work.data_ptr(), self._stream()))
        return ga, gp

    # --- row a11: SP2 purification helpers ------------------------------------------------------
    def sp2_init(self, f_orth, X, work):
        _check(lib().mi_sp2_init(self._h, f_orth.data_ptr(), X.data_ptr(), work.data_ptr(), self._stream()))

    def sp2_update(self, X, X2, nocc, out):
        _check(lib().mi_sp2_update(self._h, X.data_ptr(), X2.data_ptr(), float(nocc), out.data_ptr(), self._stream()))

    def sp2_iterate(self, X, X2, nit, nocc, work, tr):
        """Fused SP2 passes (N <= 512); returns the offset (in doubles) inside `tr` of the 2*ceil(N/16) interleaved partial
        traces {tr X, tr X^2} (add them in index order: `sp2_traces`)."""
        out = ctypes.c_void_p()
        _check(lib().mi_sp2_iterate(self._h, X.data_ptr(), X2.data_ptr(), int(nit), float(nocc), 0, work.data_ptr(),
                                    tr.data_ptr(), ctypes.byref(out), self._stream()))
        return (out.value - tr.data_ptr()) // 8

    def sp2_iterate_pingpong(self, A, B, nit, nocc, tr):
        """Fused SP2 passes on two [X|X2] buffers, no final copy: returns (result buffer, offset of {tr X, tr X^2} in `tr`)."""
        out, res = ctypes.c_void_p(), ctypes.c_void_p()
        _check(lib().mi_sp2_iterate_pingpong(self._h, A.data_ptr(), B.data_ptr(), int(nit), float(nocc), tr.data_ptr(),
                                             ctypes.byref(out), ctypes.byref(res), self._stream()))
        return (A if res.value == A.data_ptr() else B), (out.value - tr.data_ptr()) // 8

    @property
    def reduce_blocks(self):
        """Number of fixed-order partial sums `fock_energy` / `commutator_norm` write (ceil(nao^2 / 256))."""
        return (self.nao * self.nao + 255) // 256

    def sp2_iterate_planned(self, F, A, B, coef, tr, out_scale=1.0):
        """Planned purification (`sp2plan.plan` coefficients [nit+1, 3]) of the orthonormal-basis Fock matrix F on two
        [X|X2] buffers: returns (result buffer, offset in `tr` of the last pass's partial traces)."""
        coef = np.ascontiguousarray(coef, dtype=np.float64)
        nit = coef.shape[0] - 1
        out, res = ctypes.c_void_p(), ctypes.c_void_p()
        _check(lib().mi_sp2_iterate_planned(self._h, F.data_ptr(), A.data_ptr(), B.data_ptr(), nit, _dp(coef), float(out_scale),
                                            tr.data_ptr(), ctypes.byref(out), ctypes.byref(res), self._stream()))
        return (A if res.value == A.data_ptr() else B), (out.value - tr.data_ptr()) // 8

    def build_fock(self, D, h, kscale, F, part, with_k=True, vxc_unsym=None):
        """F = h + J(D) - kscale K(D) (+ V + V^T) and the energy partial sums in `part`, without forming J and K (single rank,
        resident tiles): pad -> J/K digestion -> fused finalize."""
        if not self.eri_ready:
            self.prepare_eri()
        assert D.is_contiguous() and F.is_contiguous() and part.numel() == self.reduce_blocks and part.is_contiguous()
        assert vxc_unsym is None or vxc_unsym.is_contiguous()
        with torch.cuda.device(self.device):
            _check(lib().mi_build_fock(self._h, D.data_ptr(), h.data_ptr(), vxc_unsym.data_ptr() if vxc_unsym is not None else None,
                                       int(bool(with_k)), float(kscale), F.data_ptr(), part.data_ptr(), self._stream()))
        return F

    def fock_energy(self, h, J, K, Vxc, D, kscale, F, part):
        """F = h + J - kscale K (+ Vxc); part[reduce_blocks] = partial sums of E_elec (add them in index order)."""
        assert part.numel() == self.reduce_blocks and part.is_contiguous()
        _check(lib().mi_fock_energy(self._h, h.data_ptr(), J.data_ptr(), K.data_ptr() if K is not None else None,
                                    Vxc.data_ptr() if Vxc is not None else None, D.data_ptr(), float(kscale), F.data_ptr(),
                                    part.data_ptr(), self._stream()))

    def commutator_norm(self, M, E, part):
        assert part.numel() == self.reduce_blocks and part.is_contiguous()
        _check(lib().mi_commutator_norm(self._h, M.data_ptr(), E.data_ptr(), part.data_ptr(), self._stream()))

    # --- row a10 -------------------------------------------------------------------------------
    def diis_errvec(self, sdf, out):
        _check(lib().mi_diis_errvec(self._h, sdf.data_ptr(), out.data_ptr(), self._stream()))

    def diis_combine(self, hist, coef, out):
        c = np.ascontiguousarray(coef, dtype=np.float64)
        _check(lib().mi_diis_combine(self._h, hist.data_ptr(), _dp(c), len(c), out.data_ptr(), self._stream()))

    def diis_dots_dev(self, hist_e, e, n, out):
        # vector length from the tensors: nao^2 for RHF/RKS, 2 nao^2 for the spin-stacked pair of UHF/UKS
        _check(lib().mi_diis_dots_dev_n(self._h, hist_e.data_ptr(), e.data_ptr(), n, e.numel(), out.data_ptr(), self._stream()))

    def diis_solve(self, part, m, slot, space, B, coef):
        """Pulay system of the m stored vectors solved on the device (B, coef: device tensors [space,space], [space])."""
        _check(lib().mi_diis_solve(self._h, part.data_ptr(), m, slot, space, B.data_ptr(), coef.data_ptr(), self._stream()))

    def diis_combine_dev(self, hist, coef, n, out):
        _check(lib().mi_diis_combine_dev_n(self._h, hist.data_ptr(), coef.data_ptr(), n, out.numel(), out.data_ptr(), self._stream()))

    def diis_dots(self, hist_e, e, n):
        out = np.zeros(n)
        _check(lib().mi_diis_dots(self._h, hist_e.data_ptr(), e.data_ptr(), n, _dp(out), self._stream()))
        return out


_WARM = {"started": False}


def _warm_libraries(device, n=32, nocc=24):
    """First use of rocSOLVER (syevd, potrf), rocBLAS (trsm, small GEMMs) and of the pinned-memory allocator costs ~0.3 s in
    a fresh process -- more than a whole SCF of a BASELINE config-3 molecule, and the reference's templates start one process
    per molecule.  The one-off initialisation (library handles, workspaces, the Tensile / rocSOLVER code objects of the n x n
    shapes the SCF loop uses) is triggered once per process on a helper thread with throw-away n x n inputs while the main
    thread sets up integrals (the library calls release the GIL); nothing of the calculation depends on it.
    MI355_NO_WARMUP=1 disables it."""
    if _WARM["started"] or os.environ.get("MI355_NO_WARMUP"):
        return
    _WARM["started"] = True
    import threading

    def work():
        try:
            with torch.cuda.device(device):
                s = torch.cuda.Stream(device=device)
                with torch.cuda.stream(s):
                    n_ = int(max(8, min(n, 1024)))
                    a = torch.eye(n_, dtype=torch.float64, device=device) * 2.0 + 0.01 / n_
                    # in the order the SCF needs them: the loop's GEMMs / element-wise kernels first (needed ~0.2 s into a cold
                    # benzene run), the solver last (eigh: only after convergence; its initialisation alone takes ~0.15 s)
                    (a @ a).sum()
                    torch.addmm(a, a, a, beta=0.5, alpha=0.5)
                    torch.matmul(a @ a, a.T, out=torch.empty_like(a))
                    m_ = int(max(1, min(nocc, n_)))        # the n_occ-sized products of the low-rank XC densities
                    (a[:, :m_].T @ a)
                    w_ = a @ a[:, :m_]
                    (a[:, :m_].T @ w_)
                    torch.dot(a[0], a[1])
                    # element-wise / gather kernels of torch are loaded lazily too (first torch.cat: 17 ms)
                    torch.cat([a[0], a[1], a[2, :2]])
                    torch.stack([torch.trace(a), torch.sum(a * a)])
                    a.diagonal().add_(0.0)
                    (a + a.T).mul_(0.5)
                    (2.0 * a)
                    torch.where(torch.isfinite(a).all(), a, a)
                    torch.empty(64, dtype=torch.float64).pin_memory()
                    s.synchronize()
                    torch.linalg.eigh(a)
                    r, _ = torch.linalg.cholesky_ex(a)
                    torch.linalg.solve_triangular(r, a, upper=False)
                    r2, _ = torch.linalg.cholesky_ex(a[:m_, :m_].contiguous())
                    torch.linalg.solve_triangular(r2, a[:m_, :].contiguous(), upper=False)
                s.synchronize()
        except Exception:
            pass

    t = threading.Thread(target=work, name="mi355scf-warmup", daemon=True)
    t.start()
    _WARM["thread"] = t
    import atexit
    atexit.register(lambda: t.join(timeout=10.0))   # never tear the interpreter down under a HIP call of the helper thread


def wait_warm(timeout=30.0):
    """Block until the library warm-up thread (`_warm_libraries`) has finished.  Measurement code calls this before a timed
    region: the helper thread initialises rocSOLVER for ~0.3 s after the first Engine is created and competes with the SCF
    loop for the interpreter lock while it runs (seen as a doubled host time per cycle in bench.py)."""
    t = _WARM.get("thread")
    if t is not None and t.is_alive():
        t.join(timeout)


_ENGINES = {}


def engine_for(mol):
    key = id(mol)
    eng = _ENGINES.get(key)
    if eng is None or eng.mol is not mol or not np.array_equal(eng._env, mol._env):
        eng = Engine(mol)
        _ENGINES.clear()
        _ENGINES[key] = eng
    return eng


def intor(mol, name, **kw):
    """`mol.intor('int1e_ovlp' | 'int1e_kin' | 'int1e_nuc' | 'int1e_r')` on the GPU, returned as NumPy."""
    eng = engine_for(mol)
    key = name.replace("_sph", "")
    if key == "int1e_r":
        return eng.int1e(with_dipole=True, origin=kw.get("origin"))[3].cpu().numpy()
    S, T, V = eng.int1e()
    table = {"int1e_ovlp": S, "int1e_kin": T, "int1e_nuc": V}
    if key not in table:
        raise NotImplementedError(f"intor('{name}') is outside the Fock-build hot path")
    return table[key].cpu().numpy()
