"""What the post-HF methods (`mp2`, `tdscf`, `casci`, `ccsd`, `casscf`) share on top of the resident ERI tile store: the store
guard (`resident_engine`), the AO -> MO integral transformation (`transform`: one `Engine.eri_qtrans` pass and three FP64 GEMMs)
with its work-space plan, the symmetrisation of transformed integrals and the frozen-core Fock matrix.  Plain functions; each
method module keeps its own algorithm.  Which references a method takes is its row of `reference.SUPPORT`."""
import time

import numpy as np
import torch

from .reference import traits


# ---- the reference --------------------------------------------------------------------------------------------------------------
def resident_engine(mf, who):
    """The engine of `mf` with the resident, unsharded ERI store of one GPU ready; sharded and direct-mode references are refused.
    Whether a reference runs in the direct mode is known only after its set-up, which therefore runs first."""
    if traits(mf).nranks > 1:
        raise NotImplementedError(f"{who}: sharded references are not supported (one GPU, unsharded ERI store)")
    mf._setup_once()
    if getattr(mf, "_stream_groups", 1) > 1:
        raise NotImplementedError(f"{who}: the ERI store does not fit (direct mode); not supported")
    eng = mf.engine
    if not eng.eri_ready:
        eng.prepare_eri()
    return eng


def active_mask(frozen, nmo):
    """[nmo] bool, True for the correlated orbitals: `frozen` None / 0 = all, an int n = all but the n lowest, a list = all but those."""
    act = np.ones(nmo, dtype=bool)
    if frozen is None:
        return act
    if isinstance(frozen, (int, np.integer)):
        if frozen < 0 or frozen > nmo:
            raise ValueError(f"frozen = {frozen}: between 0 and {nmo} orbitals can be frozen")
        act[:int(frozen)] = False
        return act
    idx = np.asarray(list(frozen), dtype=int)
    if idx.size and (idx.min() < 0 or idx.max() >= nmo):
        raise ValueError(f"frozen: MO indices must lie in [0, {nmo})")
    act[idx] = False
    return act


# ---- the transformation ---------------------------------------------------------------------------------------------------------
def qtrans_work_bytes(N, ncols_second):
    """Device bytes `transform` needs per column of C1: Y [N^3] plus the larger of the kernel's padded accumulator
    ((N_pad + 8)^3, alive during the kernel only) and the first GEMM's output [ncols_second, N^2]; with one target no wider
    than N the later GEMMs stay below that (each frees its input before the next allocates)."""
    ldp = 8 * ((N + 7) // 8) + 8
    return 8 * (N ** 3 + max(ldp ** 3, ncols_second * N * N))


def free_hbm(device):
    """Free HBM bytes of `device` once torch's cached blocks are returned."""
    torch.cuda.empty_cache()
    return torch.cuda.mem_get_info(device)[0]


def plan_qtrans_batch(eng, n_first, per_orb_bytes, reserve_bytes=0, forced=None):
    """(columns of C1 per `transform` call, free HBM bytes seen): as many columns of `per_orb_bytes` each as fit in 80 % of the
    free HBM beside the store less `reserve_bytes`, rounded down to whole `Engine.qtrans_batch()` passes, at most `n_first`; 0
    when not even one fits (the caller words the refusal).  `forced`: take this many (at most `n_first`) and look nothing up."""
    if forced:
        return max(1, min(int(forced), n_first)), None
    free = free_hbm(eng.device)
    nb = max(0, int((0.8 * free - reserve_bytes) // per_orb_bytes))
    q = eng.qtrans_batch()
    if nb > q:
        nb -= nb % q        # whole kernel passes
    return min(nb, n_first), free


def transform(eng, C1, C2, targets, timing=None):
    """[(1 2|3 4) as [n1, n2, n3, n4] for every (C3, C4) of `targets`] over the columns of the AO coefficient blocks, from one
    transformation of the store, Y[o, p, q, r] = sum_s C1[s, o] (sp|qr) (`Engine.eri_qtrans`, one pass per `qtrans_batch()`
    columns), and three FP64 GEMMs (rocBLAS).  `timing`: a dict whose `qtrans_seconds`, `gemm_seconds` and `passes` are
    advanced; the GEMMs are waited for only then."""
    n, n1, n2 = eng.nao, C1.shape[1], C2.shape[1]
    t0 = time.perf_counter()
    Y = eng.eri_qtrans(C1)                                         # synchronises
    t1 = time.perf_counter()
    X = torch.matmul(C2.T, Y.view(n1, n, n * n)).view(n1 * n2, n, n)      # (1 2|q r)
    del Y
    out = []
    for C3, C4 in targets:
        X2 = torch.matmul(C3.T, X)                                 # (1 2|3 r)
        if len(out) == len(targets) - 1:
            del X          # the last target: its third GEMM has the room of X, which `qtrans_work_bytes` counts on
        out.append(torch.matmul(X2, C4).view(n1, n2, C3.shape[1], C4.shape[1]))
        del X2
    if timing is not None:
        torch.cuda.synchronize(eng.device)
        timing["qtrans_seconds"] += t1 - t0
        timing["gemm_seconds"] += time.perf_counter() - t1
        timing["passes"] += -(-n1 // eng.qtrans_batch())
    return out


def symmetrize8(eri):
    """The [n, n, n, n] torch tensor (pq|rs) averaged over its eight index permutations (a new tensor; two more of its size exist
    on the way).  Integrals transformed from a screened store have the symmetries only to the screening threshold.  The pair
    exchange comes last: it keeps the two index exchanges before it, so the result is invariant under all eight to the last bit
    and a second application changes nothing."""
    for perm in ((1, 0, 2, 3), (0, 1, 3, 2), (2, 3, 0, 1)):
        eri = (eri + eri.permute(perm)).mul_(0.5)
    return eri


# ---- the frozen core ------------------------------------------------------------------------------------------------------------
def core_fock(mf, C, ncore):
    """AO-basis (F^I, E_core) of the `ncore` doubly occupied leading columns of the device tensor C: Dc = 2 Cc Cc^T,
    Vc = J(Dc) - K(Dc) / 2 from one J/K pass of the reference, F^I = h + Vc, E_core = E_nuc + Tr[Dc (h + Vc / 2)].  Without a
    core: h itself and E_nuc."""
    h, e_nuc = mf._h1, float(mf.mol.energy_nuc())
    if not ncore:
        return h, e_nuc
    Dc = 2.0 * C[:, :ncore] @ C[:, :ncore].T
    J, K = mf._jk(Dc)
    Vc = J - 0.5 * K
    return h + Vc, e_nuc + float(torch.sum(Dc * (h + 0.5 * Vc)))
