"""References and inputs for the device CDIIS tail (`diis_solve_kernel`, `scf.DeviceDIIS`): Pulay's bordered system, its
backward error in long double, its exact solution with mpmath at 50 digits, the kernel's summation order, a plain FP64
restatement of the kernel's stated algorithm (used ONLY to prove that the inputs reach its branches; the kernel is never
compared with it), and seeded families of error-vector histories.  Plain NumPy on the host, no GPU.

Two metrics.  The *plain* backward error eta is the normwise one of [0 1^T; 1 B] [lambda; c] = [1; 0].  It is blind to B once
B is small next to the border of ones: at the convergence floor (B ~ 1e-26) any c with sum 1 and lambda = 0 has eta ~ 1e-26,
and kappa_inf of the plain system is ~ 1/|B|, so no forward bound follows from it either.  Pulay's c does not change when B is
multiplied by s (lambda becomes s lambda), so every check is made a second time on the *scaled* system, s = the power of two
that brings max|B[:m,:m]| into [1, 2): there B weighs as much as the border, the floor histories are as well conditioned as
any, and a power of two changes no bit of the entries' significands."""
import math

import numpy as np

LD = np.longdouble
assert np.finfo(LD).eps < 2e-19, "these references need an 80-bit (or wider) long double"
U = 2.0 ** -53
MAXM = 16            # DIIS_MAXM of diis_solve_kernel
NS = 16              # DIIS_NS: partial sums per Gram entry
FAMILIES = ("indep", "geom", "scales", "floor", "dup", "neardup")
LEN = 49             # vector length of the solve tests: nao^2 of H2O/STO-3G, > MAXM so that 16 independent vectors exist
SEEDS = (0, 1)

# Worst plain / scaled backward error of FP64 LAPACK (numpy.linalg.solve) per family over `solve_grid()`, measured by
# tests/test_diis_reference_host.py (which re-measures and prints them); the GPU bound is 8 x these.
YARDSTICK = {
    "indep": 4.88e-17, "geom": 2.47e-17, "scales": 4.84e-18, "floor": 6.94e-17, "dup": 1.05e-16, "neardup": 2.09e-16,
}
YARDSTICK_SCALED = {
    "indep": 1.70e-16, "geom": 1.44e-17, "scales": 2.12e-17, "floor": 1.40e-16, "dup": 3.35e-17, "neardup": 2.50e-16,
}
BOUND_FACTOR = 8.0
FORWARD_GATE = 1e-3  # B4 applies where kappa * (B3 bound) is below this


def gamma(k):
    """gamma_k = k u / (1 - k u): k roundings."""
    return k * U / (1.0 - k * U)


def pulay_system(B, m):
    """([0 1^T; 1 B[:m,:m]], [1; 0]) in the dtype of B."""
    B = np.asarray(B)
    A = np.zeros((m + 1, m + 1), dtype=B.dtype)
    A[0, 1:] = 1
    A[1:, 0] = 1
    A[1:, 1:] = B[:m, :m]
    b = np.zeros(m + 1, dtype=B.dtype)
    b[0] = 1
    return A, b


def pow2_scale(B, m):
    """The power of two s with 1 <= s max|B[:m,:m]| < 2 (1.0 for a zero or non-finite block)."""
    top = float(np.abs(np.asarray(B, dtype=np.float64)[:m, :m]).max())
    if not (top > 0.0 and math.isfinite(top)):
        return 1.0
    return 2.0 ** (-math.floor(math.log2(top)))


def backward_error(A, b, x):
    """eta = |b - A x|_inf / (|A|_inf |x|_inf + |b|_inf), evaluated in long double."""
    A, b, x = (np.asarray(v, dtype=LD) for v in (A, b, x))
    r = b - A @ x
    den = np.abs(A).sum(axis=1).max() * np.abs(x).max() + np.abs(b).max()
    return float(np.abs(r).max() / den)


def lambda_from_row(A, b, c, row):
    """lambda that solves row `row` (>= 1) of the system exactly for the given c, in long double: the kernel hands out c
    only, and rows 1..m read lambda + (B c)_i = 0."""
    A, b, c = (np.asarray(v, dtype=LD) for v in (A, b, c))
    return b[row] - A[row, 1:] @ c


def eta_of_coefficients(B, m, c, slot, scaled=False):
    """Backward error of x = [lambda; c] in the plain or the scaled system of B[:m,:m], lambda from row slot + 1."""
    Bm = np.asarray(B, dtype=LD)[:m, :m]
    if scaled:
        Bm = Bm * LD(pow2_scale(B, m))
    A, b = pulay_system(Bm, m)
    lam = lambda_from_row(A, b, c, slot + 1)
    return backward_error(A, b, np.concatenate([[lam], np.asarray(c, dtype=LD)]))


def exact_solution(A, b):
    """(x, kappa_inf(A)) from mpmath at 50 digits, x = [lambda; c] as long doubles; (None, inf) for a singular A."""
    import mpmath
    with mpmath.workdps(50):
        M = mpmath.matrix([[mpmath.mpf(float(v)) for v in row] for row in np.asarray(A, dtype=np.float64)])
        rhs = mpmath.matrix([mpmath.mpf(float(v)) for v in np.asarray(b, dtype=np.float64)])
        try:
            x = mpmath.lu_solve(M, rhs)
            inv = mpmath.inverse(M)
        except ZeroDivisionError:
            return None, math.inf
        kappa = mpmath.mnorm(M, mpmath.inf) * mpmath.mnorm(inv, mpmath.inf)     # (mnorm: the operator norm; norm is entrywise)
        return np.array([LD(mpmath.nstr(v, 30)) for v in x], dtype=LD), float(kappa)


def forward_bound(kappa, eta):
    """2 kappa eta / (1 - kappa eta): relative forward error of a solution with normwise backward error eta (A and b both
    perturbed), inf where kappa eta >= 1."""
    ke = kappa * eta
    return 2.0 * ke / (1.0 - ke) if ke < 1.0 else math.inf


def sequential_sum(parts):
    """FP64 left-to-right sum over the last axis starting from 0.0: what the kernel does with the 16 partials."""
    parts = np.asarray(parts, dtype=np.float64)
    s = np.zeros(parts.shape[:-1], dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        for q in range(parts.shape[-1]):
            s = s + parts[..., q]
    return s


def kernel_model(part, m, slot, space, B):
    """Plain FP64 restatement of the kernel's stated algorithm.  Returns dict(coef[m], fallback, swaps = steps k with a row
    interchange, B = the updated [space][space] matrix).  Gaussian elimination with partial pivoting, the first row on ties;
    c = e_slot when a pivot is not > 0 or not finite, or a back-substituted value is not finite."""
    part = np.asarray(part, dtype=np.float64).reshape(-1, NS)
    B = np.array(B, dtype=np.float64).reshape(space, space)
    dot = sequential_sum(part[:m])
    B[slot, :m] = dot
    B[:m, slot] = dot
    A, b = pulay_system(B, m)
    n = m + 1
    M = np.concatenate([A, b[:, None]], axis=1)
    swaps, ok = [], True
    e_slot = np.zeros(m)
    e_slot[slot] = 1.0
    with np.errstate(all="ignore"):
        for k in range(n):
            col = np.abs(M[k:, k])
            p = k + int(np.argmax(col)) if not np.isnan(col).any() else k + int(np.flatnonzero(np.isnan(col))[0])
            val = abs(M[p, k])
            if not (val > 0.0) or not math.isfinite(val):
                ok = False
                break
            if p != k:
                M[[k, p]] = M[[p, k]]
                swaps.append(k)
            for r in range(k + 1, n):
                f = M[r, k] / M[k, k]
                M[r, k:] = M[r, k:] - f * M[k, k:]
        x = np.zeros(n)
        if ok:
            for i in range(n - 1, -1, -1):
                x[i] = M[i, n] / M[i, i]
                if not math.isfinite(x[i]):
                    ok = False
                    break
                M[:i, n] = M[:i, n] - M[:i, i] * x[i]
    return dict(coef=x[1:].copy() if ok else e_slot, fallback=not ok, swaps=swaps, B=B)


# --- inputs ------------------------------------------------------------------------------------------------------------------
def _rng(family, m, seed, length):
    return np.random.default_rng([FAMILIES.index(family), m, seed, length])


def history(family, m, seed, length=LEN):
    """Error vectors V[m, length] of a seeded family."""
    rng = _rng(family, m, seed, length)
    g = rng.normal(size=(m, length))
    if family == "indep":            # independent vectors, one scale per draw from 1e-8 .. 1
        return g * 10.0 ** int(rng.integers(-8, 1))
    if family == "geom":             # a convergent history: nearly collinear, e_i = r^i v + 1e-6 r^i w_i
        v = rng.normal(size=length)
        r = 0.3 ** np.arange(m)
        return r[:, None] * v[None, :] + 1e-6 * r[:, None] * g
    if family == "scales":           # row scales 10^0 .. 10^-12 across the history: B spans 24 decades
        return g * (10.0 ** (-12.0 * np.arange(m) / max(m - 1, 1)))[:, None]
    if family == "floor":            # the convergence floor: B ~ 1e-26 next to the border of ones
        return 1e-13 * g
    if family == "dup":              # a bitwise fixed point: the newest vector equals the oldest
        g[-1] = g[0]
        return g
    if family == "neardup":
        g[-1] = g[0] * (1.0 + 1e-15 * rng.normal(size=length))
        return g
    raise ValueError(family)


def gram(V):
    """Gram matrix of the rows of V: long-double accumulation rounded once to FP64; bitwise symmetric, and bitwise equal rows
    for bitwise equal vectors."""
    W = np.asarray(V, dtype=LD)
    return (W @ W.T).astype(np.float64)


def split_partials(value, rng):
    """16 unequal partials of `value` (random positive and negative weights), the last one adjusted so that their sequential
    FP64 sum is `value` itself wherever an adjustment by a few ulps reaches it.  The tests never rely on that: they compare
    with `sequential_sum` of what this returns.  It only makes the Gram matrix of `dup` singular to the bit."""
    w = rng.uniform(0.02, 0.2, size=NS) * rng.choice([1.0, 1.0, 1.0, -1.0], size=NS)
    p = value * w / w.sum()
    head = float(sequential_sum(p[:-1]))
    last = value - head
    for _ in range(8):
        got = head + last
        if got == value:
            break
        last = np.nextafter(last, math.inf if got < value else -math.inf)
    p[-1] = last
    return p


def solve_grid():
    """The (family, m, space, slot, seed) cases of the GPU solve test."""
    out = []
    for family in FAMILIES:
        for m in range(1, MAXM + 1):
            for space in sorted({m, MAXM}):
                for slot in sorted({0, m // 2, m - 1}):
                    for seed in SEEDS:
                        out.append((family, m, space, slot, seed))
    return out


SENT_ROW, SENT_OUT, SENT_COEF = -7.0, -3.25e300, 1.5e-300     # stale row/column, beyond m, coefficients


def solve_case(family, m, space, slot, seed):
    """Inputs of one solve case: dict(part[space*16], B0[space][space], coef0[space], Bfull[m][m] = the true Gram matrix).
    B0 holds the true Gram matrix with row and column `slot` stale and everything at index >= m a second sentinel."""
    V = history(family, m, seed)
    Bfull = gram(V)
    rng = np.random.default_rng([99, FAMILIES.index(family), m, space, slot, seed])
    B0 = np.full((space, space), SENT_OUT)
    B0[:m, :m] = Bfull
    B0[slot, :m] = SENT_ROW
    B0[:m, slot] = SENT_ROW
    part = rng.normal(size=(space, NS))                 # rows >= m: never read
    for i in range(m):
        part[i] = split_partials(Bfull[i, slot], rng)
    return dict(part=part.ravel().copy(), B0=B0, coef0=np.full(space, SENT_COEF), Bfull=Bfull)


def expected_B(case, m, slot):
    """B after the solve: B0 with row and column `slot` replaced by the sequential sums of the partials."""
    B = case["B0"].copy()
    dot = sequential_sum(case["part"].reshape(-1, NS)[:m])
    B[slot, :m] = dot
    B[:m, slot] = dot
    return B


def chain_history(space, nmat, nao, seed=0):
    """(E, F) of the DeviceDIIS drive: 2 space + 3 pairs, E[k] the `geom` family reshaped to [nmat, nao, nao] (or [nao, nao]),
    F[k] = F* + sym(E[k]) / 2-like symmetric matrices around a fixed symmetric F*."""
    npush = 2 * space + 3
    length = nmat * nao * nao
    shape = (nao, nao) if nmat == 1 else (nmat, nao, nao)
    E = history("geom", npush, seed, length).reshape((npush,) + shape)
    rng = np.random.default_rng([7, space, nmat, nao, seed])
    Fs = rng.normal(size=shape)
    Fs = 0.5 * (Fs + np.swapaxes(Fs, -1, -2))
    F = Fs[None] + 0.5 * (E + np.swapaxes(E, -1, -2))
    return np.ascontiguousarray(E), np.ascontiguousarray(F)
