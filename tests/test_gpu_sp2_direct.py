"""Planned purification with the MFMA operands loaded straight into registers (`sp2_direct_kernel`, engine option sp2_direct)
against numpy at the tile edges, against the LDS-staged `sp2_plan_kernel`, and inside the SCF.

Sizes come from hydrogen chains in STO-3G (nao == number of atoms).  The exact cases fill the inputs with small integers: every
product and partial sum is exact, so every pass's matrix and per-block partial traces must equal numpy bit for bit whatever the
K split.  Every output buffer is followed by GUARD doubles of sentinel that must come back unchanged."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GUARD = 4096
_SENT_BITS = np.array([-2 ** 63, 0x7FF8DEAD0000BEEF], dtype=np.int64)   # -0.0 and a NaN with a payload, alternating
_ENG = {}
TS = 64                                   # trace slots per pass (2 x SP2_TRS)
# integer plan [nit + 1, 3]: pass 0 maps X_0 = b F + c I, pass k applies X_k = a X_{k-1}^2 + b X_{k-1} + c I
PLAN_INT = np.array([[0.0, 1.0, 1.0], [1.0, -1.0, 0.0], [-1.0, 0.0, 1.0], [1.0, 1.0, -1.0]])
# every N up to 40 (all partial first, second and third tiles) and the edges around the benzene/cc-pVTZ size; 320 is the
# largest N of the kernel (20 MFMA steps per wave), 321 and 336 take sp2_plan_kernel with the option on
SIZES = list(range(1, 41)) + [255, 256, 257, 263, 264, 320, 321, 336]


def engine(n):
    if n not in _ENG:
        from mi355scf.mole import Mole
        from mi355scf.engine import Engine
        mol = Mole(atom="; ".join(f"H 0 0 {1.0 * i}" for i in range(n)), basis="sto-3g", spin=n % 2, unit="Bohr", verbose=0).build()
        e = Engine(mol)
        assert e.nao == n
        _ENG[n] = e
    return _ENG[n]


def _sentinel_bits(start, m):
    return _SENT_BITS[(start + np.arange(m)) % 2]


def guarded(size):
    import torch
    return torch.as_tensor(_sentinel_bits(0, size + GUARD).view(np.float64), device="cuda")


def assert_guard(flat, size, what=""):
    tail = flat[size:].cpu().numpy().view(np.int64)
    bad = np.flatnonzero(tail != _sentinel_bits(size, tail.size))
    assert bad.size == 0, f"{what}: {bad.size} guard doubles overwritten, first at +{bad[0]}"


def untouched(host, start=0):
    return np.array_equal(host.view(np.int64), _sentinel_bits(start, host.size))


def cdiv(a, b):
    return -(-a // b)


def sparse_sym(n, rng):
    """Symmetric {-1, 0, 1} matrix with one non-zero in every 16 x 16 tile pair (I >= J)."""
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


def plan_replay(F, coef, out_scale):
    n = F.shape[0]
    I = np.eye(n)
    X = coef[0, 1] * F + coef[0, 2] * I
    nit = coef.shape[0] - 1
    passes, writes = [], []
    for k in range(nit + 1):
        assert (np.abs(X) @ np.abs(X)).max() * 16 < 2.0 ** 53
        X2 = X @ X
        passes.append(block_traces(X, X2))
        if k < nit:
            a, b, c = coef[k + 1]
            X = a * X2 + b * X + c * I
            writes.append(X)
        else:
            writes.append(out_scale * X)
    return passes, writes


def planned(e, direct, *args, **kw):
    e.set_option("sp2_direct", direct)
    try:
        return e.sp2_iterate_planned(*args, **kw)
    finally:
        e.set_option("sp2_direct", 0)


@pytest.mark.parametrize("n", SIZES)
def test_sp2_direct_exact(n):
    """Every pass of plans of 1-4 passes: result, the other ping-pong buffer, all partial traces; exact symmetry; guards."""
    import torch
    e = engine(n)
    nn, nbd = n * n, cdiv(n, 16)
    F = sparse_sym(n, np.random.default_rng(1000 + n))
    Fd = torch.as_tensor(F, device="cuda")
    for nit in range(PLAN_INT.shape[0]):
        coef = PLAN_INT[:nit + 1]
        traces, writes = plan_replay(F, coef, 2.0)
        A, B, tr = guarded(nn), guarded(nn), guarded((nit + 2) * TS)
        res, off = planned(e, 1, Fd, A[:nn].view(n, n), B[:nn].view(n, n), coef, tr, out_scale=2.0)
        assert off == TS * nit
        assert res.data_ptr() == (A if nit % 2 == 0 else B).data_ptr()
        got = res.cpu().numpy().reshape(n, n)
        assert np.array_equal(got, writes[-1]) and np.array_equal(got, got.T)
        other = (B if nit % 2 == 0 else A).cpu().numpy()
        if nit == 0:
            assert untouched(other), "the second buffer is written by a single-pass plan"
        else:
            o = other[:nn].reshape(n, n)
            assert np.array_equal(o, writes[-2]) and np.array_equal(o, o.T)
        trh = tr.cpu().numpy()
        for k in range(nit + 1):
            assert np.array_equal(trh[TS * k:TS * k + 2 * nbd], traces[k]), f"pass {k} traces"
            assert untouched(trh[TS * k + 2 * nbd:TS * (k + 1)], TS * k + 2 * nbd), f"pass {k}: trace slots past ceil(N/16)"
        assert untouched(trh[TS * (nit + 1):], TS * (nit + 1))
        for buf in (A, B):
            assert_guard(buf, nn, "sp2_direct")


@pytest.mark.parametrize("n", [17, 100, 255, 264, 320])
def test_sp2_direct_every_pass_symmetric_and_equal_to_the_plan_kernel(n):
    """Real-valued projector plan: after every pass the matrix of the new kernel is exactly symmetric, its traces repeat bit for
    bit from run to run, and it agrees with sp2_plan_kernel to rounding (1e-12); the final projector is that of eigh."""
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
    Fd = torch.as_tensor(F, device="cuda")
    A = torch.empty((n, n), dtype=torch.float64, device="cuda")
    B = torch.empty_like(A)
    nbd = cdiv(n, 16)
    for k in range(1, coef.shape[0] + 1):
        out = {}
        for direct, rep in ((1, 0), (1, 1), (0, 0)):
            tr = torch.zeros(TS * (k + 1), dtype=torch.float64, device="cuda")
            res, off = planned(e, direct, Fd, A, B, coef[:k], tr, out_scale=1.0)
            out[(direct, rep)] = (res.cpu().numpy().copy(), tr.cpu().numpy().copy())
        X, T = out[(1, 0)]
        assert np.array_equal(X, X.T), f"pass {k - 1}"
        assert np.array_equal(X, out[(1, 1)][0]) and np.array_equal(T, out[(1, 1)][1])
        assert np.abs(X - out[(0, 0)][0]).max() < 1e-12 * max(1.0, np.abs(X).max())
        for j in range(k):
            t = T[TS * j:TS * j + 2 * nbd].reshape(-1, 2).sum(axis=0)
            t0 = out[(0, 0)][1][TS * j:TS * j + 2 * nbd].reshape(-1, 2).sum(axis=0)
            assert np.abs(t - t0).max() < 1e-10 * n
    X = out[(1, 0)][0]
    assert np.abs(X - P).max() < 1e-10
    t = out[(1, 0)][1][TS * (coef.shape[0] - 1):][:2 * nbd].reshape(-1, 2).sum(axis=0)
    assert abs(t[0] - nocc) < 1e-9 and abs(t[0] - t[1]) < 1e-9


@pytest.mark.parametrize("atom,basis", [("H2O", "cc-pVDZ"), ("BENZENE", "cc-pVDZ")])
def test_planned_scf_energy_same_with_either_pass_kernel(atom, basis):
    """Planned, pipelined SCF (second kernel() of an object, HIP-graph head included) with sp2_direct_kernel and with
    sp2_plan_kernel: the same converged energy and density."""
    import gpu4pyscf
    from pyscf import gto
    from mi355scf import fixtures
    mol = gto.Mole()
    mol.atom, mol.basis, mol.verbose = getattr(fixtures, atom), basis, 0
    mol.build()
    res = {}
    for direct in (True, False):
        mf = gpu4pyscf.scf.RHF(mol).to_gpu()
        mf.sp2_direct, mf.conv_tol = direct, 1e-10
        mf.kernel()
        assert mf._purifier.plan is not None
        e = mf.kernel()                      # planned from its first cycle
        assert mf.converged
        assert mf.engine._sp2_direct == int(direct)
        D = mf.make_rdm1()
        res[direct] = (e, D.cpu().numpy() if hasattr(D, "cpu") else np.asarray(D))
    assert abs(res[True][0] - res[False][0]) < 1e-10, res
    assert np.abs(res[True][1] - res[False][1]).max() < 1e-7
