"""The dense per-cycle kernels after the Fock build -- XC matrix (`xc_vmat`, `xc_vmat_fold`, `xc_aow`), purification (`sp2_*`),
DIIS and the fused reductions -- pinned one by one against numpy at the tile edges where kernels go wrong.

Sizes come from hydrogen chains in STO-3G (nao == number of atoms, any N).  Most cases fill the inputs with small integers:
every product and partial sum is then exact, the result does not depend on split-K, MFMA order or atomics, and the device
result must equal numpy bit for bit -- a wrong index, mask, transposition, mirror store or a split counted twice shows.  One
real-valued case per kernel checks scaling and sign against a rounding bound |C - ref| <= 16 u sqrt(k) (|A| |B|^T) with
u = 2^-53 and k the contraction length; the reference of the GEMMs is exact to ~2^-64 (`_gemm_nt_ref`).  Every output lives
in a flat buffer followed by GUARD doubles of sentinel that must come back unchanged."""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
GUARD = 4096
# sentinel: -0.0 and a NaN with a payload, alternating, compared bit for bit (an atomic add of 0.0 changes -0.0)
_SENT_BITS = np.array([-2 ** 63, 0x7FF8DEAD0000BEEF], dtype=np.int64)
_ENG = {}


def engine(n):
    """One engine per N on an H_n chain (STO-3G: nao == n), no ERIs."""
    if n not in _ENG:
        from mi355scf.mole import Mole
        from mi355scf.engine import Engine
        mol = Mole(atom="; ".join(f"H 0 0 {1.0 * i}" for i in range(n)), basis="sto-3g", spin=n % 2, unit="Bohr", verbose=0).build()
        e = Engine(mol)
        assert e.nao == n
        _ENG[n] = e
    return _ENG[n]


def _sentinel_bits(start, m):
    """Sentinel bits of buffer positions start .. start + m (the pattern follows the absolute position)."""
    return _SENT_BITS[(start + np.arange(m)) % 2]


def guarded(size, init=None):
    """Device buffer of `size` doubles (initialised from `init`, else sentinel) followed by GUARD doubles of sentinel."""
    import torch
    host = _sentinel_bits(0, size + GUARD).view(np.float64)
    if init is not None:
        host[:size] = np.asarray(init, dtype=np.float64).ravel()
    return torch.as_tensor(host, device="cuda")


def assert_guard(flat, size, what=""):
    tail = flat[size:].cpu().numpy().view(np.int64)
    bad = np.flatnonzero(tail != _sentinel_bits(size, tail.size))
    assert bad.size == 0, f"{what}: {bad.size} guard doubles overwritten, first at +{bad[0]}"


def untouched(host, start=0):
    """host = buffer[start:] (or a slice of it starting there) still holds the sentinel."""
    return np.array_equal(host.view(np.int64), _sentinel_bits(start, host.size))


def ints(rng, shape, lo=-8, hi=8):
    return rng.integers(lo, hi + 1, size=shape).astype(np.float64)


def record(name, ratio, limit=1.0):
    print(f"[rounding] {name}: worst |err| / bound = {ratio:.3g}")
    assert ratio <= limit, (name, ratio)


def cdiv(a, b):
    return -(-a // b)


def _row_scale(X):
    mx = np.abs(X).max(axis=1, keepdims=True)
    return np.ldexp(1.0, np.frexp(np.where(mx > 0, mx, 1.0))[1])          # power of two with |X / scale| < 1


def _slices(X, scale, nbits, nsl):
    """X = sum of nsl slices of <= nbits significant bits each relative to the row scale, plus a remainder < 2^-(nbits nsl)."""
    R = X / scale
    out = []
    for s in range(nsl):
        f = 2.0 ** (nbits * (s + 1))
        P = np.trunc(R * f) / f
        out.append(P * scale)
        R = R - P
    return out


def _gemm_nt_ref(A, B, chunk=1 << 16):
    """A @ B^T in extended precision: per chunk of the contraction, A and B are cut into slices whose pairwise products and
    sums are exact in float64 (2 nbits + log2(chunk) <= 53), and the exact pieces are added in long double."""
    nbits = (53 - int(math.ceil(math.log2(max(2, min(chunk, A.shape[1])))))) // 2
    acc = np.zeros((A.shape[0], B.shape[0]), dtype=np.longdouble)
    ra, rb = _row_scale(A), _row_scale(B)
    for k0 in range(0, A.shape[1], chunk):
        sa_all = _slices(A[:, k0:k0 + chunk], ra, nbits, 4)
        sb_all = _slices(B[:, k0:k0 + chunk], rb, nbits, 4)
        for s, sa in enumerate(sa_all):
            for t, sb in enumerate(sb_all):
                if s + t <= 3:                     # the rest is below 2^-(4 nbits) of the row scales
                    acc += (sa @ sb.T).astype(np.longdouble)
    return acc


def gemm_bound(A, B, k):
    return 16.0 * U * math.sqrt(k) * (np.abs(A) @ np.abs(B).T)


# ------------------------------------------------------------------------------------------------------------------------------
# xc_vmat: C += A W^T  (split-K FP64 MFMA, 64 x 64 tiles, edge-tile branch, XCD-aware order)
# ------------------------------------------------------------------------------------------------------------------------------
VMAT_N = [1, 15, 16, 17, 31, 33, 63, 64, 65, 80, 127, 128, 129, 200, 264]
VMAT_NG = [1, 3, 63, 64, 65, 511, 512, 513, 4097]
VMAT_CASES = [(n, VMAT_NG[(i + j) % len(VMAT_NG)]) for i, n in enumerate(VMAT_N) for j in (0, 3, 6)]   # every ng, 3 per N


def vmat_plan(n, ng, wgs_opt=0, xcd_opt=1):
    """(nsplit, kchunk, xcd_order) as mi_xc_vmat derives them."""
    ntt = cdiv(n, 64) ** 2
    wgs = wgs_opt if wgs_opt > 0 else 1024
    cap = wgs // ntt if wgs_opt >= 0 else cdiv(1024, ntt)
    nsplit = max(1, min(cdiv(ng, 512), cap))
    kchunk = cdiv(cdiv(ng, nsplit), 64) * 64
    nsplit = cdiv(ng, kchunk)
    ns8 = nsplit // 8 * 8
    xcd = bool(xcd_opt and ns8 >= 8 and ns8 * 10 >= nsplit * 9)
    if xcd:
        nsplit = ns8
        kchunk = cdiv(cdiv(ng, nsplit), 64) * 64
    return nsplit, kchunk, xcd


def _run_vmat(e, A, W, C0, alias=False):
    import torch
    n = e.nao
    a = torch.as_tensor(A, device="cuda")
    w = a if alias else torch.as_tensor(W, device="cuda")
    C = guarded(n * n, C0)
    e.xc_vmat(a, w, C[:n * n].view(n, n))
    got = C[:n * n].view(n, n).cpu().numpy()
    assert_guard(C, n * n, "xc_vmat")
    return got


@pytest.mark.parametrize("n,ng", VMAT_CASES)
def test_xc_vmat_exact(n, ng):
    e = engine(n)
    rng = np.random.default_rng(1000 * n + ng)
    A, W, C0 = ints(rng, (n, ng)), ints(rng, (n, ng)), ints(rng, (n, n))
    assert np.array_equal(_run_vmat(e, A, W, C0), C0 + A @ W.T)           # A != W: a transposed product differs
    assert np.array_equal(_run_vmat(e, A, None, C0, alias=True), C0 + A @ A.T)   # A aliased with W (the DF K call)


VMAT_OPT_CASES = [(n, ng, xcd, wgs) for n, ng in ((65, 4097), (264, 20000)) for xcd in (0, 1) for wgs in (0, -1, 16, 4096)]


def test_xc_vmat_option_cases_reach_both_orders():
    orders = {vmat_plan(n, ng, wgs, xcd)[2] for n, ng, xcd, wgs in VMAT_OPT_CASES}
    assert orders == {False, True}
    assert vmat_plan(264, 123158)[2]                      # the production grid of benzene cc-pVTZ takes the XCD order


@pytest.mark.parametrize("n,ng,xcd,wgs", VMAT_OPT_CASES)
def test_xc_vmat_options_exact(n, ng, xcd, wgs):
    e = engine(n)
    rng = np.random.default_rng(7 * n + ng + 3 * xcd + wgs)
    A, W, C0 = ints(rng, (n, ng)), ints(rng, (n, ng)), ints(rng, (n, n))
    try:
        e.set_option("vmat_xcd", xcd)
        e.set_option("vmat_wgs", wgs)
        got = _run_vmat(e, A, W, C0)
    finally:
        e.set_option("vmat_xcd", 1)
        e.set_option("vmat_wgs", 0)
    assert np.array_equal(got, C0 + A @ W.T), vmat_plan(n, ng, wgs, xcd)


@pytest.mark.parametrize("n,ng,alias", [(65, 4097, False), (264, 123158, False), (40, 1000003, True)])
def test_xc_vmat_real_within_rounding_bound(n, ng, alias):
    """Random real inputs: a small edge-tile case, benzene cc-pVTZ's grid (N = 264) and the DF K shape (N = 40, A = W)."""
    e = engine(n)
    rng = np.random.default_rng(n + ng)
    A = rng.standard_normal((n, ng))
    W = A if alias else rng.standard_normal((n, ng)) * np.exp(rng.uniform(-3, 3, ng))
    C0 = rng.standard_normal((n, n))
    got = _run_vmat(e, A, W, C0, alias=alias)
    ref = _gemm_nt_ref(A, W) + C0
    bound = gemm_bound(A, W, ng + 1) + 16.0 * U * np.abs(C0)
    record(f"xc_vmat N={n} ng={ng}", float(np.max(np.abs(got - ref) / bound)))


def test_xc_vmat_zero_points_leaves_c_untouched():
    import torch
    from mi355scf.engine import EngineError, _check, lib
    for n in (17, 264):
        e = engine(n)
        C = guarded(n * n)            # all sentinel: -0.0 and NaN, so even an added 0.0 would show
        a = torch.zeros((n, 1), dtype=torch.float64, device="cuda")
        e.xc_vmat(a[:, :0], a[:, :0], C[:n * n].view(n, n))
        for gga in (0, 1):
            e.xc_vmat_fold(torch.zeros((4, n, 1), dtype=torch.float64, device="cuda")[..., :0], a[:0], gga, C[:n * n].view(n, n))
        torch.cuda.synchronize()
        assert untouched(C.cpu().numpy())
        with pytest.raises(EngineError):
            _check(lib().mi_xc_vmat(e._h, a.data_ptr(), a.data_ptr(), -1, C.data_ptr(), e._stream()))
        with pytest.raises(EngineError):
            _check(lib().mi_xc_vmat_fold(e._h, a.data_ptr(), a.data_ptr(), -1, 1, C.data_ptr(), e._stream()))
        assert untouched(C.cpu().numpy())


# ------------------------------------------------------------------------------------------------------------------------------
# xc_vmat_fold: C += ao_0 (sum_c wv_c ao_c)^T with the weighted AOs formed in the loader, MT x 64 rows per workgroup
# ------------------------------------------------------------------------------------------------------------------------------
def fold_mt(n, cap):
    """Template MT mi_xc_vmat_fold instantiates for N and the vmat_fold_mt cap."""
    nt = cdiv(n, 64)
    nrb = cdiv(nt, max(1, min(5, cap)))
    return cdiv(nt, nrb)


FOLD_CASES = ([(264, cap, 4097) for cap in (1, 2, 3, 5)] + [(200, 4, 4097)]
              + [(n, 3, ng) for n, ng in ((1, 65), (17, 513), (64, 512), (65, 1), (128, 3), (129, 2000))])


def test_xc_vmat_fold_cases_instantiate_every_mt():
    assert {fold_mt(n, cap) for n, cap, _ in FOLD_CASES} == {1, 2, 3, 4, 5}
    assert any(n % 64 for n, _, _ in FOLD_CASES)


def _run_fold(e, ao, wv, gga, C0):
    import torch
    n = e.nao
    C = guarded(n * n, C0)
    e.xc_vmat_fold(torch.as_tensor(ao, device="cuda"), torch.as_tensor(wv, device="cuda"), gga, C[:n * n].view(n, n))
    got = C[:n * n].view(n, n).cpu().numpy()
    assert_guard(C, n * n, "xc_vmat_fold")
    return got


def _fold_ref_w(ao, wv, gga):
    return sum(wv[c][None, :] * ao[c] for c in range(4 if gga else 1))


@pytest.mark.parametrize("gga", [0, 1])
@pytest.mark.parametrize("n,cap,ng", FOLD_CASES)
def test_xc_vmat_fold_exact(n, cap, ng, gga):
    e = engine(n)
    rng = np.random.default_rng(31 * n + cap + ng + gga)
    nc = 4 if gga else 1
    ao, wv, C0 = ints(rng, (nc, n, ng)), ints(rng, (nc, ng)), ints(rng, (n, n))
    try:
        e.set_option("vmat_fold_mt", cap)
        got = _run_fold(e, ao, wv, gga, C0)
    finally:
        e.set_option("vmat_fold_mt", 3)
    assert np.array_equal(got, C0 + ao[0] @ _fold_ref_w(ao, wv, gga).T), fold_mt(n, cap)


@pytest.mark.parametrize("xcd,wgs", [(0, 0), (1, 4096), (1, 16)])
def test_xc_vmat_fold_options_exact(xcd, wgs):
    n, ng = 80, 70001
    e = engine(n)
    rng = np.random.default_rng(xcd + wgs)
    ao, wv, C0 = ints(rng, (4, n, ng)), ints(rng, (4, ng)), ints(rng, (n, n))
    try:
        e.set_option("vmat_xcd", xcd)
        e.set_option("vmat_wgs", wgs)
        got = _run_fold(e, ao, wv, 1, C0)
    finally:
        e.set_option("vmat_xcd", 1)
        e.set_option("vmat_wgs", 0)
    assert np.array_equal(got, C0 + ao[0] @ _fold_ref_w(ao, wv, 1).T)


def test_xc_vmat_fold_real_within_rounding_bound():
    n, ng = 200, 30011
    e = engine(n)
    rng = np.random.default_rng(5)
    ao, wv, C0 = rng.standard_normal((4, n, ng)), rng.standard_normal((4, ng)), rng.standard_normal((n, n))
    try:
        e.set_option("vmat_fold_mt", 4)
        got = _run_fold(e, ao, wv, 1, C0)
    finally:
        e.set_option("vmat_fold_mt", 3)
    Wabs = sum(np.abs(wv[c])[None, :] * np.abs(ao[c]) for c in range(4))
    ref = C0 + _gemm_nt_ref(ao[0], _fold_ref_w(ao, wv, 1))
    # the weighted AO row is itself rounded (4 terms): |dW| <= 4 u Wabs, which the bound on |ao_0| Wabs^T covers
    bound = 16.0 * U * math.sqrt(ng + 4) * (np.abs(ao[0]) @ Wabs.T) + 16.0 * U * np.abs(C0)
    record(f"xc_vmat_fold N={n} ng={ng} GGA", float(np.max(np.abs(got - ref) / bound)))


# ------------------------------------------------------------------------------------------------------------------------------
# xc_aow: aow[m][g] = sum_c ao_c[m][g] wv_c[g]; rows strided by gridDim.y = min(nao, 64)
# ------------------------------------------------------------------------------------------------------------------------------
def _run_aow(e, ao, wv, gga, ng):
    import torch
    from mi355scf.engine import _check, lib
    n = e.nao
    out = guarded(n * ng)                  # sentinel everywhere: an element the kernel skips stays NaN / -0.0
    a, w = torch.as_tensor(ao, device="cuda"), torch.as_tensor(wv, device="cuda")
    _check(lib().mi_xc_aow(e._h, a.data_ptr(), w.data_ptr(), ng, gga, out.data_ptr(), e._stream()))
    got = out[:n * ng].view(n, ng).cpu().numpy()
    assert_guard(out, n * ng, "xc_aow")
    return got


@pytest.mark.parametrize("gga", [0, 1])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 129])
def test_xc_aow_exact(n, gga):
    e = engine(n)
    for ng in (1, 300, 1000):
        rng = np.random.default_rng(n * ng + gga)
        nc = 4 if gga else 1
        ao, wv = ints(rng, (nc, n, ng)), ints(rng, (nc, ng))
        assert np.array_equal(_run_aow(e, ao, wv, gga, ng), _fold_ref_w(ao, wv, gga))


def test_xc_aow_real_and_empty():
    import torch
    n, ng = 129, 4099
    e = engine(n)
    rng = np.random.default_rng(9)
    ao, wv = rng.standard_normal((4, n, ng)), rng.standard_normal((4, ng))
    got = _run_aow(e, ao, wv, 1, ng)
    ref = sum(wv[c][None, :].astype(np.longdouble) * ao[c] for c in range(4))
    bound = 16.0 * U * math.sqrt(4) * sum(np.abs(wv[c])[None, :] * np.abs(ao[c]) for c in range(4))
    record("xc_aow GGA", float(np.max(np.abs(got - ref) / bound)))
    empty = e.xc_aow(torch.zeros((4, n, 0), dtype=torch.float64, device="cuda"), torch.zeros((4, 0), dtype=torch.float64, device="cuda"))
    assert tuple(empty.shape) == (n, 0)


# ------------------------------------------------------------------------------------------------------------------------------
# SP2: planned purification (sp2_plan_kernel<MAXM>), the checked recursion (sp2_fused_kernel) and the N > 512 helpers
# ------------------------------------------------------------------------------------------------------------------------------
SP2_N = [1, 2, 15, 16, 17, 128, 129, 192, 193, 256, 257, 320, 321, 336, 337, 400, 511, 512]
TS = 64                                   # trace slots per pass (2 x SP2_TRS)
# integer plan [nit + 1, 3]: pass 0 maps X_0 = b F + c I, pass k applies X_k = a X_{k-1}^2 + b X_{k-1} + c I
PLAN_INT = np.array([[0.0, 1.0, 1.0], [1.0, -1.0, 0.0], [-1.0, 0.0, 1.0], [1.0, 1.0, -1.0]])


def sp2_maxm(n):
    m = cdiv(n, 16)
    return 8 if m <= 8 else 12 if m <= 12 else 16 if m <= 16 else 20 if m <= 20 else "16x2"


def test_sp2_sizes_reach_every_instantiation():
    assert {sp2_maxm(n) for n in SP2_N} == {8, 12, 16, 20, "16x2"}


def sparse_sym(n, rng):
    """Symmetric {-1, 0, 1} matrix with one non-zero in every 16 x 16 tile pair (I >= J): every tile of the triangular grid
    reads and mirrors something."""
    F = np.zeros((n, n))
    nb = cdiv(n, 16)
    for bi in range(nb):
        for bj in range(bi + 1):
            i = int(rng.integers(16 * bi, min(n, 16 * bi + 16)))
            j = int(rng.integers(16 * bj, min(n, 16 * bj + 16)))
            F[i, j] = F[j, i] = rng.choice([-1.0, 1.0])
    return F


def block_traces(X, X2):
    n = X.shape[0]
    d, d2 = np.diag(X), np.diag(X2)
    return np.array([[d[b:b + 16].sum(), d2[b:b + 16].sum()] for b in range(0, n, 16)]).ravel()


def assert_exact_range(*mats):
    """Precondition of the exact tests: every partial sum of the products stays below 2^53."""
    for X in mats:
        assert (np.abs(X) @ np.abs(X)).max() * 16 < 2.0 ** 53


def plan_replay(F, coef, out_scale):
    """-> (passes: list of (X_k, traces of pass k)), result buffer content, the other buffer's content (or None)."""
    n = F.shape[0]
    I = np.eye(n)
    X = coef[0, 1] * F + coef[0, 2] * I
    nit = coef.shape[0] - 1
    passes, writes = [], []
    for k in range(nit + 1):
        assert_exact_range(X)
        X2 = X @ X
        passes.append(block_traces(X, X2))
        if k < nit:
            a, b, c = coef[k + 1]
            X = a * X2 + b * X + c * I
            writes.append(X)
        else:
            writes.append(out_scale * X)
    return passes, writes


@pytest.mark.parametrize("n", SP2_N)
def test_sp2_planned_exact(n):
    import torch
    e = engine(n)
    nn, nbd = n * n, cdiv(n, 16)
    F = sparse_sym(n, np.random.default_rng(n))
    Fd = torch.as_tensor(F, device="cuda")
    for nit in range(PLAN_INT.shape[0]):
        coef = PLAN_INT[:nit + 1]
        traces, writes = plan_replay(F, coef, 2.0)
        A, B, tr = guarded(nn), guarded(nn), guarded((nit + 2) * TS)
        res, off = e.sp2_iterate_planned(Fd, A[:nn].view(n, n), B[:nn].view(n, n), coef, tr, out_scale=2.0)
        assert off == TS * nit
        assert res.data_ptr() == (A if nit % 2 == 0 else B).data_ptr()    # pass k writes A for even k, B for odd k
        got = res.cpu().numpy().reshape(n, n)
        assert np.array_equal(got, writes[-1]) and np.array_equal(got, got.T)
        other = (B if nit % 2 == 0 else A).cpu().numpy()
        if nit == 0:
            assert untouched(other), "the second buffer is written by a single-pass plan"
        else:
            assert np.array_equal(other[:nn].reshape(n, n), writes[-2])
        trh = tr.cpu().numpy()
        for k in range(nit + 1):
            assert np.array_equal(trh[TS * k:TS * k + 2 * nbd], traces[k]), f"pass {k} traces"
            assert untouched(trh[TS * k + 2 * nbd:TS * (k + 1)], TS * k + 2 * nbd), f"pass {k}: trace slots past ceil(N/16)"
        assert untouched(trh[TS * (nit + 1):], TS * (nit + 1))
        for buf in (A, B):
            assert_guard(buf, nn, "sp2_iterate_planned")


@pytest.mark.parametrize("n", [m for m in SP2_N if m > 1])
def test_sp2_planned_projector_from_spectrum(n):
    import torch
    from mi355scf import sp2plan
    e = engine(n)
    nocc = max(1, n // 5)
    rng = np.random.default_rng(n)
    q, _ = np.linalg.qr(rng.normal(size=(n, n)))
    ev = np.sort(np.concatenate([rng.uniform(-20.0, -0.4, nocc), rng.uniform(0.1, 30.0, n - nocc)]))
    F = (q * ev) @ q.T
    F = 0.5 * (F + F.T)
    P = q[:, :nocc] @ q[:, :nocc].T
    coef = sp2plan.plan(*sp2plan.bounds_from_spectrum(ev, nocc))
    A = torch.empty((n, n), dtype=torch.float64, device="cuda")
    B = torch.empty_like(A)
    tr = torch.zeros(TS * coef.shape[0], dtype=torch.float64, device="cuda")
    res, off = e.sp2_iterate_planned(torch.as_tensor(F, device="cuda"), A, B, coef, tr, out_scale=2.0)
    X = res.cpu().numpy()
    assert np.abs(X - 2.0 * P).max() < 1e-10
    t = tr[off:off + 2 * (cdiv(n, 16))].cpu().numpy().reshape(-1, 2).sum(axis=0)
    assert abs(t[0] - nocc) < 1e-9 and abs(t[0] - t[1]) < 1e-9


def fused_replay(X0, nit, target):
    """Trace-correcting SP2 as sp2_fused_kernel runs it: pass 0 squares X_0; pass k picks X_k = X^2 if
    |tr X^2 - N| < |2 tr X - tr X^2 - N| (traces: the previous pass's block partials added in index order), else 2 X - X^2."""
    X = X0
    X2 = X @ X
    tr = [block_traces(X, X2)]
    branches = []
    for _ in range(nit):
        assert_exact_range(X)
        t = tr[-1].reshape(-1, 2)
        tx, tx2 = 0.0, 0.0
        for b in range(t.shape[0]):
            tx += t[b, 0]
            tx2 += t[b, 1]
        sq = abs(tx2 - target) < abs(2.0 * tx - tx2 - target)
        branches.append(sq)
        X = X2 if sq else 2.0 * X - X2
        assert_exact_range(X)
        X2 = X @ X
        tr.append(block_traces(X, X2))
    return X, X2, tr, branches


@pytest.mark.parametrize("n", SP2_N)
def test_sp2_fused_exact(n):
    import torch
    e = engine(n)
    nn, nbd = n * n, cdiv(n, 16)
    X0 = sparse_sym(n, np.random.default_rng(n + 1))
    X0[0, 0] = -1.0
    seen = set()
    for target in (2.0 ** 40, -2.0 ** 40):
        for nit in range(4):
            X, X2, trs, br = fused_replay(X0, nit, target)
            seen.update(br)
            # sp2_iterate: X_nit, X_nit^2 copied back into d_X / d_X2
            dX, dX2, work, tr = guarded(nn, X0), guarded(nn), guarded(2 * nn), guarded((nit + 2) * TS)
            off = e.sp2_iterate(dX[:nn].view(n, n), dX2[:nn].view(n, n), nit, target, work[:2 * nn], tr)
            assert off == TS * nit
            gx, gx2 = dX[:nn].cpu().numpy().reshape(n, n), dX2[:nn].cpu().numpy().reshape(n, n)
            assert np.array_equal(gx, X) and np.array_equal(gx2, X2) and np.array_equal(gx2, gx2.T)
            trh = tr.cpu().numpy()
            for k in range(nit + 1):
                assert np.array_equal(trh[TS * k:TS * k + 2 * nbd], trs[k]), f"sp2_iterate pass {k} traces"
                assert untouched(trh[TS * k + 2 * nbd:TS * (k + 1)], TS * k + 2 * nbd)
            assert untouched(trh[TS * (nit + 1):], TS * (nit + 1))
            for buf, size in ((dX, nn), (dX2, nn), (work, 2 * nn)):
                assert_guard(buf, size, "sp2_iterate")
            # sp2_iterate_pingpong: [X | X^2] in A or B by parity, no copy
            A, B, tr = guarded(2 * nn, np.concatenate([X0.ravel(), np.zeros(nn)])), guarded(2 * nn), guarded((nit + 2) * TS)
            res, off = e.sp2_iterate_pingpong(A, B, nit, target, tr)
            assert off == TS * nit and res.data_ptr() == (B if nit % 2 == 0 else A).data_ptr()
            got = res[:2 * nn].cpu().numpy()
            assert np.array_equal(got[:nn].reshape(n, n), X) and np.array_equal(got[nn:].reshape(n, n), X2)
            trh = tr.cpu().numpy()
            for k in range(nit + 1):
                assert np.array_equal(trh[TS * k:TS * k + 2 * nbd], trs[k]), f"pingpong pass {k} traces"
            assert untouched(trh[TS * (nit + 1):], TS * (nit + 1))
            for buf in (A, B):
                assert_guard(buf, 2 * nn, "sp2_iterate_pingpong")
    assert seen == {True, False}, "both branches of the trace-correcting step"


def test_sp2_fused_real_within_rounding_bound():
    n = 337
    e = engine(n)
    rng = np.random.default_rng(3)
    q, _ = np.linalg.qr(rng.normal(size=(n, n)))
    X0 = (q * rng.uniform(0.0, 1.0, n)) @ q.T
    X0 = 0.5 * (X0 + X0.T)
    nn = n * n
    dX, dX2, work, tr = guarded(nn, X0), guarded(nn), guarded(2 * nn), guarded(2 * TS)
    e.sp2_iterate(dX[:nn].view(n, n), dX2[:nn].view(n, n), 0, n / 2, work[:2 * nn], tr)
    got = dX2[:nn].cpu().numpy().reshape(n, n)
    assert np.array_equal(dX[:nn].cpu().numpy().reshape(n, n), X0)
    ref = _gemm_nt_ref(X0, X0)
    record(f"sp2_fused X^2 N={n}", float(np.max(np.abs(got - ref) / gemm_bound(X0, X0, n))))


@pytest.mark.parametrize("fn", ["sp2_iterate", "sp2_iterate_pingpong", "sp2_iterate_planned"])
def test_sp2_fused_paths_refuse_n_over_512(fn):
    import torch
    from mi355scf.engine import EngineError
    n = 513
    e = engine(n)
    nn = n * n
    bufs = [guarded(2 * nn) for _ in range(3)]
    tr = guarded(4 * TS)
    with pytest.raises(EngineError, match="N <= 512"):
        if fn == "sp2_iterate":
            e.sp2_iterate(bufs[0][:nn].view(n, n), bufs[1][:nn].view(n, n), 1, 1.0, bufs[2][:2 * nn], tr)
        elif fn == "sp2_iterate_pingpong":
            e.sp2_iterate_pingpong(bufs[0], bufs[1], 1, 1.0, tr)
        else:
            e.sp2_iterate_planned(bufs[2][:nn].view(n, n), bufs[0][:nn].view(n, n), bufs[1][:nn].view(n, n), PLAN_INT[:2], tr)
    torch.cuda.synchronize()
    assert all(untouched(b.cpu().numpy()) for b in bufs + [tr])


def gershgorin_x0(F):
    d = np.diag(F)
    r = np.abs(F).sum(axis=1) - np.abs(d)
    emin, emax = (d - r).min(), (d + r).max()
    return (emax * np.eye(F.shape[0]) - F) / (emax - emin), emin, emax


@pytest.mark.parametrize("n", [16, 100, 513, 600])
def test_sp2_init_and_update(n):
    import torch
    e = engine(n)
    nn = n * n
    rng = np.random.default_rng(n)
    # sp2_init, integer F: bounds and X_0 exact (one correctly rounded division per element)
    for real in (False, True):
        F = rng.standard_normal((n, n)) if real else ints(rng, (n, n))
        F = 0.5 * (F + F.T) if real else np.triu(F) + np.triu(F, 1).T
        ref, emin, emax = gershgorin_x0(F)
        X, work = guarded(nn), guarded(2 * n)
        e.sp2_init(torch.as_tensor(F, device="cuda"), X[:nn].view(n, n), work[:2 * n])
        got = X[:nn].cpu().numpy().reshape(n, n)
        assert_guard(X, nn, "sp2_init X")
        assert_guard(work, 2 * n, "sp2_init work")
        if not real:
            assert np.array_equal(got, ref)
        else:   # disc bounds differ by the rounding of the row sums: |d e| <= n u (max row sum of |F|)
            de = n * U * np.abs(F).sum(axis=1).max() * 4.0
            tol = 4.0 * U * np.abs(ref) + de * (1.0 + 2.0 * np.abs(ref)) / (emax - emin)
            record(f"sp2_init N={n}", float(np.max(np.abs(got - ref) / tol)))
    # sp2_update: [tr X, tr X^2, X_new], X_new = X^2 or 2 X - X^2 by the trace rule
    for real in (False, True):
        Xh = rng.standard_normal((n, n)) if real else ints(rng, (n, n))
        X2h = rng.standard_normal((n, n)) if real else ints(rng, (n, n))
        tx, tx2 = np.trace(Xh), np.trace(X2h)
        assert abs(tx - tx2) > 1.0
        for target, sq in ((tx2, True), (2.0 * tx - tx2, False)):     # the rule's two sides at a distance 2 |tx - tx2|
            out = guarded(2 + nn)
            e.sp2_update(torch.as_tensor(Xh, device="cuda"), torch.as_tensor(X2h, device="cuda"), target, out)
            o = out.cpu().numpy()
            assert_guard(out, 2 + nn, "sp2_update")
            assert np.array_equal(o[2:2 + nn].reshape(n, n), X2h if sq else 2.0 * Xh - X2h)
            if real:
                assert abs(o[0] - tx) <= 16 * U * math.sqrt(n) * np.abs(np.diag(Xh)).sum()
                assert abs(o[1] - tx2) <= 16 * U * math.sqrt(n) * np.abs(np.diag(X2h)).sum()
            else:
                assert o[0] == tx and o[1] == tx2


# ------------------------------------------------------------------------------------------------------------------------------
# DIIS helpers and the fused elementwise reductions
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 65, 264])
def test_diis_errvec(n):
    import torch
    e = engine(n)
    rng = np.random.default_rng(n)
    for M in (ints(rng, (n, n)), rng.standard_normal((n, n))):       # one subtraction: exact for real inputs as well
        out = guarded(n * n)
        e.diis_errvec(torch.as_tensor(M, device="cuda"), out[:n * n].view(n, n))
        assert np.array_equal(out[:n * n].cpu().numpy().reshape(n, n), M.T - M)
        assert_guard(out, n * n, "diis_errvec")


@pytest.mark.parametrize("dev", [False, True])
def test_diis_combine(dev):
    import torch
    from mi355scf.engine import EngineError
    n = 65
    e = engine(n)
    nn = n * n
    rng = np.random.default_rng(int(dev))
    worst = 0.0
    for m in range(1, 17):
        for real in (False, True):
            H = rng.standard_normal((m, n, n)) if real else ints(rng, (m, n, n))
            c = rng.standard_normal(m) if real else ints(rng, m, -3, 3)
            out = guarded(nn)
            o = out[:nn].view(n, n)
            if dev:
                e.diis_combine_dev(torch.as_tensor(H, device="cuda"), torch.as_tensor(c, device="cuda"), m, o)
            else:
                e.diis_combine(torch.as_tensor(H, device="cuda"), c, o)
            got = o.cpu().numpy()
            assert_guard(out, nn, "diis_combine")
            ref = np.einsum("i,ijk->jk", c.astype(np.longdouble), H.astype(np.longdouble))
            if real:
                bound = 16 * U * math.sqrt(m) * np.einsum("i,ijk->jk", np.abs(c), np.abs(H))
                worst = max(worst, float(np.max(np.abs(got - ref) / bound)))
            else:
                assert np.array_equal(got, ref.astype(np.float64)), m
    record(f"diis_combine{'_dev' if dev else ''}", worst)
    H = torch.zeros((17, n, n), dtype=torch.float64, device="cuda")
    out = guarded(nn)
    with pytest.raises(EngineError):
        if dev:
            e.diis_combine_dev(H, torch.ones(17, dtype=torch.float64, device="cuda"), 17, out[:nn].view(n, n))
        else:
            e.diis_combine(H, np.ones(17), out[:nn].view(n, n))
    torch.cuda.synchronize()
    assert untouched(out.cpu().numpy())


def dots_slices(length):
    per = cdiv(length, 16)
    return [(min(per * s, length), min(per * (s + 1), length)) for s in range(16)]


@pytest.mark.parametrize("m", [1, 7, 64])
def test_diis_dots_dev_partials(m):
    import torch
    e = engine(64)
    rng = np.random.default_rng(m)
    for length in (1, 15, 17, 255, 4095, 4096, 4097, 2 * 264 * 264):
        H, v = ints(rng, (m, length)), ints(rng, length)
        out = guarded(m * 16)
        e.diis_dots_dev(torch.as_tensor(H, device="cuda"), torch.as_tensor(v, device="cuda"), m, out)
        got = out[:m * 16].cpu().numpy().reshape(m, 16)
        assert_guard(out, m * 16, "diis_dots_dev")
        ref = np.array([[H[i, lo:hi] @ v[lo:hi] for lo, hi in dots_slices(length)] for i in range(m)])
        assert np.array_equal(got, ref), length
    # real inputs: each partial within the bound of its slice
    length = 4097
    H, v = rng.standard_normal((m, length)), rng.standard_normal(length)
    out = guarded(m * 16)
    e.diis_dots_dev(torch.as_tensor(H, device="cuda"), torch.as_tensor(v, device="cuda"), m, out)
    got = out[:m * 16].cpu().numpy().reshape(m, 16)
    worst = 0.0
    for s, (lo, hi) in enumerate(dots_slices(length)):
        ref = (H[:, lo:hi].astype(np.longdouble) * v[lo:hi]).sum(axis=1)
        bound = 16 * U * math.sqrt(hi - lo) * (np.abs(H[:, lo:hi]) @ np.abs(v[lo:hi]))
        worst = max(worst, float(np.max(np.abs(got[:, s] - ref) / bound)))
    record(f"diis_dots_dev m={m}", worst)


@pytest.mark.parametrize("n", [1, 4, 63, 64, 65, 264])
def test_diis_dots(n):
    import torch
    from mi355scf.engine import EngineError
    e = engine(n)
    rng = np.random.default_rng(n)
    for m in (1, 64):
        H, v = ints(rng, (m, n, n)), ints(rng, (n, n))
        got = e.diis_dots(torch.as_tensor(H, device="cuda"), torch.as_tensor(v, device="cuda"), m)
        assert np.array_equal(got, H.reshape(m, -1) @ v.ravel())
    with pytest.raises(EngineError):
        e.diis_dots(torch.zeros((65, n, n), dtype=torch.float64, device="cuda"), torch.zeros((n, n), dtype=torch.float64, device="cuda"), 65)
    with pytest.raises(EngineError):
        e.diis_dots_dev(torch.zeros((65, n, n), dtype=torch.float64, device="cuda"), torch.zeros((n, n), dtype=torch.float64, device="cuda"),
                        65, torch.zeros(65 * 16, dtype=torch.float64, device="cuda"))


def block_sums(x, nblk):
    x = np.concatenate([x.ravel(), np.zeros(nblk * 256 - x.size)])
    return x.reshape(nblk, 256).sum(axis=1)


@pytest.mark.parametrize("n", [1, 15, 16, 17, 63, 65, 264])
def test_commutator_norm(n):
    import torch
    e = engine(n)
    nb = e.reduce_blocks
    rng = np.random.default_rng(n)
    for real in (False, True):
        M = rng.standard_normal((n, n)) if real else ints(rng, (n, n))
        E, part = guarded(n * n), guarded(nb)
        e.commutator_norm(torch.as_tensor(M, device="cuda"), E[:n * n].view(n, n), part[:nb])
        gE, gp = E[:n * n].cpu().numpy().reshape(n, n), part[:nb].cpu().numpy()
        assert_guard(E, n * n, "commutator_norm E")
        assert_guard(part, nb, "commutator_norm part")
        ref_E = M - M.T
        assert np.array_equal(gE, ref_E)
        if real:
            ref = block_sums(ref_E.astype(np.longdouble) ** 2, nb)
            record(f"commutator_norm N={n}", float(np.max(np.abs(gp - ref) / (16 * U * 16.0 * block_sums(ref_E ** 2, nb) + 1e-300))))
        else:
            assert np.array_equal(gp, block_sums(ref_E ** 2, nb))


@pytest.mark.parametrize("n", [1, 17, 64, 65, 264])
def test_fock_energy(n):
    import torch
    e = engine(n)
    nb = e.reduce_blocks
    rng = np.random.default_rng(n)
    for real in (False, True):
        for with_k, with_v in ((True, True), (True, False), (False, True), (False, False)):
            h, J, K, V, D = (rng.standard_normal((n, n)) if real else ints(rng, (n, n)) for _ in range(5))
            ks = 0.37 if real else 0.5
            F, part = guarded(n * n), guarded(nb)
            t = lambda x: torch.as_tensor(x, device="cuda")
            e.fock_energy(t(h), t(J), t(K) if with_k else None, t(V) if with_v else None, t(D), ks, F[:n * n].view(n, n), part[:nb])
            gF, gp = F[:n * n].cpu().numpy().reshape(n, n), part[:nb].cpu().numpy()
            assert_guard(F, n * n, "fock_energy F")
            assert_guard(part, nb, "fock_energy part")
            v2 = J - ks * K if with_k else J
            refF = h + v2 + (V if with_v else 0.0)
            terms = D * (h + 0.5 * v2)
            if real:
                L = np.longdouble
                v2l = J.astype(L) - (ks * K.astype(L) if with_k else 0.0)
                refF = h.astype(L) + v2l + (V if with_v else 0.0)
                absF = np.abs(h) + np.abs(J) + (ks * np.abs(K) if with_k else 0.0) + (np.abs(V) if with_v else 0.0)
                rF = float(np.max(np.abs(gF - refF) / (4 * U * absF)))
                absE = np.abs(D) * (np.abs(h) + 0.5 * (np.abs(J) + (ks * np.abs(K) if with_k else 0.0)))
                refE = block_sums(D.astype(L) * (h.astype(L) + 0.5 * v2l), nb)
                rE = float(np.max(np.abs(gp - refE) / (16 * U * 16.0 * block_sums(absE, nb))))
                record(f"fock_energy N={n} K={with_k} V={with_v}", max(rF, rE))
            else:
                assert np.array_equal(gF, refF)
                assert np.array_equal(gp, block_sums(terms, nb))
