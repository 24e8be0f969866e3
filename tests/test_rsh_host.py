"""CAM-B3LYP host references (no GPU): a NumPy McMurchie-Davidson ERI evaluator with the erf(omega r12)/r12 hook, the short-range
B88 (ITYH) energy density, and `dft.rsh_coeff`.  The GPU tests (test_gpu_rsh.py) check the engine against these references, so
each is validated here against something independent: the oracle's full-Coulomb ERIs, the omega -> 0 limit, and a quadrature of
the uniform-gas exchange hole."""
import math

import numpy as np
import pytest
from scipy import integrate, special

CAM_OMEGA = 0.33
ITYH_SERIES_A = 1.0   # the kernel's switch from the closed form of F(a) to its series in 1/a^2
# F(a) = u (c0 - c1 u + c2 u^2 - ...), u = 1/a^2: the kernel's twelve terms
ITYH_COEF = (1.0 / 36.0, 1.0 / 960.0, 1.0 / 26880.0, 1.0 / 829440.0, 1.0 / 28385280.0, 1.0 / 1073479680.0, 1.0 / 44590694400.0,
             1.0 / 2021444812800.0, 1.0 / 99407521382400.0, 1.0 / 5273830608076800.0, 1.0 / 300357209869516800.0,
             1.0 / 18282612774666240000.0)


# ---------------------------------------------------------------------------------------------
# McMurchie-Davidson ERIs over the real-spherical contracted shells of a Mole, optionally attenuated by erf(omega r12)
# ---------------------------------------------------------------------------------------------
def boys(nmax, T):
    """F_0..F_nmax at the array T: F_nmax from the regularised incomplete gamma function (Taylor series for T < 1), then
    downward recursion (stable)."""
    T = np.asarray(T, dtype=np.float64)
    out = np.empty((nmax + 1,) + T.shape)
    a = nmax + 0.5
    small = T < 1.0
    Ts = np.where(small, T, 0.0)
    ser = np.zeros_like(T)
    term = np.ones_like(T)
    for k in range(40):
        ser = ser + term / (2 * nmax + 2 * k + 1)
        term = term * (-Ts) / (k + 1)
    Tl = np.where(small, 1.0, T)
    big = math.gamma(a) * special.gammainc(a, Tl) / (2.0 * Tl ** a)
    out[nmax] = np.where(small, ser, big)
    eT = np.exp(-T)
    for n in range(nmax, 0, -1):
        out[n - 1] = (2.0 * T * out[n] + eT) / (2 * n - 1)
    return out


def _cart(l):
    return [(lx, ly, l - lx - ly) for lx in range(l, -1, -1) for ly in range(l - lx, -1, -1)]


def _c2s(l):
    from oracle import dft as odft
    return odft._c2s(l)


class MDEri:
    """(ij|kl) shell blocks by McMurchie-Davidson, vectorised over primitive quartets.  omega > 0: erf(omega r12)/r12 --
    the Hermite Coulomb tensor R is built with the exponent theta rho (theta = omega^2 / (omega^2 + rho)) and the prefactor gets
    sqrt(theta)."""

    def __init__(self, mol, omega=0.0):
        self.mol, self.omega = mol, float(omega)
        self.loc = mol.ao_loc_nr()
        self.shells = []
        for ish in range(mol.nbas):
            ia, l, npr, _nc, _k, pe, pc, _ = mol._bas[ish]
            A = mol._env[mol._atm[ia, 1]:mol._atm[ia, 1] + 3].copy()
            self.shells.append((int(l), mol._env[pe:pe + npr].copy(), mol._env[pc:pc + npr].copy(), A))
        self._pairs = {}

    def _pair(self, i, j):
        key = (i, j)
        if key in self._pairs:
            return self._pairs[key]
        la, ea, ca, A = self.shells[i]
        lb, eb, cb, B = self.shells[j]
        a, b = np.repeat(ea, len(eb)), np.tile(eb, len(ea))
        cc = np.repeat(ca, len(cb)) * np.tile(cb, len(ca))
        p = a + b
        P = (a[:, None] * A + b[:, None] * B) / p[:, None]
        L = la + lb
        E1 = []   # per direction: E[i][j][t] arrays over primitive pairs
        for d in range(3):
            XAB, XPA, XPB = A[d] - B[d], P[:, d] - A[d], P[:, d] - B[d]
            E = np.zeros((la + 1, lb + 1, L + 2, len(p)))
            E[0, 0, 0] = np.exp(-a * b / p * XAB * XAB)
            for ii in range(la + 1):
                for jj in range(lb + 1):
                    if ii == 0 and jj == 0:
                        continue
                    if ii > 0:
                        src, X, i0, j0 = E[ii - 1, jj], XPA, ii - 1, jj
                    else:
                        src, X, i0, j0 = E[ii, jj - 1], XPB, ii, jj - 1
                    for t in range(i0 + j0 + 2):
                        v = X * src[t] + (t + 1) * src[t + 1]
                        if t > 0:
                            v = v + src[t - 1] / (2 * p)
                        E[ii, jj, t] = v
            E1.append(E)
        herm = [(t, u, v) for t in range(L + 1) for u in range(L + 1 - t) for v in range(L + 1 - t - u)]
        ca_, cb_ = _cart(la), _cart(lb)
        Eab = np.zeros((len(p), len(ca_) * len(cb_), len(herm)))
        for x, (ax, ay, az) in enumerate(ca_):
            for y, (bx, by, bz) in enumerate(cb_):
                for h, (t, u, v) in enumerate(herm):
                    Eab[:, x * len(cb_) + y, h] = E1[0][ax, bx, t] * E1[1][ay, by, u] * E1[2][az, bz, v]
        Eab *= cc[:, None, None]
        out = self._pairs[key] = (p, P, Eab, herm, la, lb)
        return out

    def shell_block(self, i, j, k, l):
        """(ij|kl) [2li+1, 2lj+1, 2lk+1, 2ll+1] in the AO order of the Mole."""
        p, P, Eab, hab, la, lb = self._pair(i, j)
        q, Q, Ecd, hcd, lc, ld = self._pair(k, l)
        L = la + lb + lc + ld
        pp, qq = np.repeat(p, len(q)), np.tile(q, len(p))
        PQ = np.repeat(P, len(q), axis=0) - np.tile(Q, (len(p), 1))
        rho = pp * qq / (pp + qq)
        th = np.ones_like(rho)
        if self.omega > 0.0:
            w2 = self.omega ** 2
            th = w2 / (w2 + rho)
        alpha = rho * th
        R2 = (PQ * PQ).sum(axis=1)
        F = boys(L, alpha * R2)
        # Hermite Coulomb tensor R_{tuv} = R^0_{tuv}, recursion over the auxiliary index n
        Rn = {}
        for n in range(L + 1):
            Rn[(n, 0, 0, 0)] = (-2.0 * alpha) ** n * F[n]

        def R(n, t, u, v):
            key = (n, t, u, v)
            if key in Rn:
                return Rn[key]
            if t > 0:
                val = PQ[:, 0] * R(n + 1, t - 1, u, v)
                if t > 1:
                    val = val + (t - 1) * R(n + 1, t - 2, u, v)
            elif u > 0:
                val = PQ[:, 1] * R(n + 1, t, u - 1, v)
                if u > 1:
                    val = val + (u - 1) * R(n + 1, t, u - 2, v)
            else:
                val = PQ[:, 2] * R(n + 1, t, u, v - 1)
                if v > 1:
                    val = val + (v - 1) * R(n + 1, t, u, v - 2)
            Rn[key] = val
            return val
        Rm = np.empty((len(pp), len(hab), len(hcd)))
        for x, (t, u, v) in enumerate(hab):
            for y, (tt, uu, vv) in enumerate(hcd):
                Rm[:, x, y] = (-1) ** (tt + uu + vv) * R(0, t + tt, u + uu, v + vv)
        pref = 2.0 * math.pi ** 2.5 / (pp * qq * np.sqrt(pp + qq)) * np.sqrt(th)
        Rm *= pref[:, None, None]
        Rm = Rm.reshape(len(p), len(q), len(hab), len(hcd))
        cart = np.einsum("iah,ijhg,jbg->ab", Eab, Rm, Ecd, optimize=True)
        nca, ncb, ncc, ncd = (len(_cart(x)) for x in (la, lb, lc, ld))
        cart = cart.reshape(nca, ncb, ncc, ncd)
        return np.einsum("abcd,ai,bj,ck,dl->ijkl", cart, _c2s(la), _c2s(lb), _c2s(lc), _c2s(ld), optimize=True)

    def full(self):
        """The whole [nao]^4 tensor (8-fold symmetry)."""
        n, loc, nb = self.mol.nao, self.loc, self.mol.nbas
        out = np.zeros((n, n, n, n))
        for i in range(nb):
            for j in range(i + 1):
                for k in range(i + 1):
                    for l in range(k + 1 if k < i else j + 1):
                        blk = self.shell_block(i, j, k, l)
                        si, sj, sk, sl = (slice(loc[s], loc[s + 1]) for s in (i, j, k, l))
                        for (a, b, c, d), g in (((si, sj, sk, sl), blk), ((sj, si, sk, sl), blk.transpose(1, 0, 2, 3)),
                                                ((si, sj, sl, sk), blk.transpose(0, 1, 3, 2)),
                                                ((sj, si, sl, sk), blk.transpose(1, 0, 3, 2))):
                            out[a, b, c, d] = g
                            out[c, d, a, b] = g.transpose(2, 3, 0, 1)
        return out


# ---------------------------------------------------------------------------------------------
# Short-range B88 (ITYH attenuation), complex-safe for complex-step derivatives
# ---------------------------------------------------------------------------------------------
def ityh_closed(a):
    return 1.0 - 8.0 / 3.0 * a * (np.sqrt(np.pi) * special.erf(0.5 / a) + (2 * a - 4 * a ** 3) * np.exp(-0.25 / (a * a))
                                  - 3 * a + 4 * a ** 3)


def ityh_series_over_u(u):
    """P(u) = F(a) a^2 at u = 1/a^2 (Horner, as the kernel)."""
    p = ITYH_COEF[-1]
    for c in ITYH_COEF[-2::-1]:
        p = c - u * p
    return p


def ityh_series(a):
    u = 1.0 / (a * a)
    return u * ityh_series_over_u(u)


def ityh(a):
    a = np.asarray(a)
    big = np.real(a) >= ITYH_SERIES_A
    return np.where(big, ityh_series(np.where(big, a, 5.0)), ityh_closed(np.where(big, 1.0, a)))


def b88_sr_channel(r, s, omega):
    """e_s^SR of one spin channel (Slater included): e_s^B88 F(a_s), e_s^B88 = -1/2 r^(4/3) K_s, k_s = sqrt(9 pi / K_s) r^(1/3),
    a_s = omega / (2 k_s)."""
    beta = 0.0042
    r13 = r ** (1.0 / 3)
    r43 = r * r13
    x = np.sqrt(s) / r43
    asinh = np.log(x + np.sqrt(x * x + 1))
    K = 1.5 * (6 / np.pi) ** (1.0 / 3) + 2 * beta * x * x / (1 + 6 * beta * x * asinh)
    # a^2 = q K.  On the series K F(a) = P(1/a^2) / q, formed without K as in the kernel: de/dsigma = K' (F + a F'/2), whose
    # leading 1/(36 a^2) terms cancel, then comes out of P alone (also under the complex step)
    q = omega * omega / (36 * np.pi * r13 * r13)
    a2 = q * K
    big = np.real(a2) >= ITYH_SERIES_A ** 2
    series = ityh_series_over_u(1.0 / np.where(big, a2, 4.0)) / q
    closed = K * ityh_closed(np.sqrt(np.where(big, 0.25, a2)))
    return -0.5 * r43 * np.where(big, series, closed)


def b88_channel(r, s):
    beta = 0.0042
    x = np.sqrt(s) / r ** (4.0 / 3)
    asinh = np.log(x + np.sqrt(x * x + 1))
    return -0.75 * (6 / np.pi) ** (1.0 / 3) * r ** (4.0 / 3) - beta * r ** (4.0 / 3) * x * x / (1 + 6 * beta * x * asinh)


def b88_sr(rho, sigma, omega=CAM_OMEGA):
    """Closed-shell energy density per volume."""
    return 2.0 * b88_sr_channel(0.5 * rho, 0.25 * sigma, omega)


def b88_sr_derivs(rho, sigma, omega=CAM_OMEGA, h=1e-30):
    """(e, de/drho, de/dsigma) by complex step."""
    rho, sigma = np.asarray(rho, dtype=complex), np.asarray(sigma, dtype=complex)
    e = np.real(b88_sr(rho, sigma, omega))
    return e, np.imag(b88_sr(rho + 1j * h, sigma, omega)) / h, np.imag(b88_sr(rho, sigma + 1j * h, omega)) / h


def lda_sr_quadrature(a):
    """F(a) of the uniform gas: 4 int_0^inf j1(y)^2 / y erfc(2 a y) dy (the spin-sigma exchange hole with erfc(omega u)/u)."""
    def f(y):
        if y < 1e-3:
            j1 = y / 3 - y ** 3 / 30 + y ** 5 / 840
        else:
            j1 = math.sin(y) / (y * y) - math.cos(y) / y
        return j1 * j1 / y * math.erfc(2 * a * y)
    ymax = 7.0 / (2 * a)
    edges = np.unique(np.concatenate([np.arange(0.0, ymax, math.pi), [ymax]]))
    tot = 0.0
    for lo, hi in zip(edges[:-1], edges[1:]):
        tot += integrate.quad(f, lo, hi, epsabs=1e-17, epsrel=1e-13, limit=200)[0]
    return 4.0 * tot


# ---------------------------------------------------------------------------------------------
# tests
# ---------------------------------------------------------------------------------------------
def _mol(atom, basis):
    from pyscf import gto
    return gto.M(atom=atom, basis=basis, verbose=0)


H2O = "O 0 0 0; H 0 -0.757 0.587; H 0 0.757 0.587"


def test_boys_function_against_quadrature():
    T = np.array([0.0, 1e-9, 0.3, 0.99, 1.0, 3.7, 17.0, 60.0])
    F = boys(12, T)
    for n in (0, 5, 12):
        for t, got in zip(T, F[n]):
            ref = integrate.quad(lambda x: x ** (2 * n) * math.exp(-t * x * x), 0, 1, epsabs=1e-300, epsrel=1e-13)[0]
            assert abs(got - ref) <= 1e-13 * ref, (n, t, got, ref)


def test_md_eri_matches_oracle_full_coulomb():
    """theta = 1 (omega = 0): the McMurchie-Davidson tensor equals the oracle's on H2O/6-31G(d)."""
    from oracle import oracle as orc
    mol = _mol(H2O, "6-31g(d)")
    ref = orc.Oracle(mol).eri_full()
    got = MDEri(mol).full()
    assert np.abs(got - ref).max() < 1e-11, np.abs(got - ref).max()


def test_md_eri_small_omega_limit():
    """omega -> 0: erf(omega r)/r -> 2 omega / sqrt(pi), so (ab|cd)_LR -> 2 omega / sqrt(pi) S_ab S_cd (with the oracle's
    overlap)."""
    from oracle import oracle as orc
    mol = _mol(H2O, "6-31g(d)")
    S = orc.Oracle(mol).int1e()[0]
    om = 1e-5
    got = MDEri(mol, om).full()
    ref = 2 * om / math.sqrt(math.pi) * np.einsum("ab,cd->abcd", S, S)
    # the next order is relative O(omega^2 <r12^2> / 3): ~6e-8 at omega = 1e-4 for these diffuse d shells, ~6e-10 at 1e-5
    assert np.abs(got - ref).max() < 1e-8 * np.abs(ref).max(), np.abs(got - ref).max()


@pytest.mark.parametrize("rho_s", [1.0, 1e-1, 1e-2, 1e-4, 1e-6, 1e-8, 1e-10])
def test_b88_sr_uniform_gas_matches_exchange_hole_quadrature(rho_s):
    """x = 0 (LDA part): e^SR / e^LDA of one channel equals the quadrature of the uniform-gas exchange hole with erfc(omega u)."""
    e = b88_sr_channel(np.array(rho_s), np.array(0.0), CAM_OMEGA)
    e_lda = -0.75 * (6 / np.pi) ** (1.0 / 3) * rho_s ** (4.0 / 3)
    kf = (6 * np.pi ** 2 * rho_s) ** (1.0 / 3)
    a = CAM_OMEGA / (2 * kf)
    ref = lda_sr_quadrature(a)
    assert abs(float(e) / e_lda - ref) <= 1e-10 * ref, (a, float(e) / e_lda, ref)


def test_b88_sr_small_omega_is_b88():
    rng = np.random.default_rng(3)
    rho = 10.0 ** rng.uniform(-6, 2, 50)
    sigma = rho ** (8.0 / 3) * 10.0 ** rng.uniform(-3, 2, 50)
    got = b88_sr(rho, sigma, 1e-9)
    ref = 2 * b88_channel(0.5 * rho, 0.25 * sigma)
    assert np.abs(got / ref - 1).max() < 1e-7


def test_ityh_switch_is_continuous():
    a = ITYH_SERIES_A
    assert abs(ityh_closed(a) - ityh_series(a)) <= 1e-9 * ityh_series(a)
    h = 1e-30
    d_closed = np.imag(ityh_closed(a + 1j * h)) / h
    d_series = np.imag(ityh_series(a + 1j * h)) / h
    assert abs(d_closed - d_series) <= 1e-7 * abs(d_series), (d_closed, d_series)
    # the series is what the kernel uses above the switch: it matches the closed form where both are still accurate
    for x in (3.0, 3.5):
        assert abs(ityh_closed(x) - ityh_series(x)) <= 3e-10 * ityh_closed(x)


def test_rsh_coeff_values_and_aliases():
    from mi355scf import dft
    for name in ("CAM-B3LYP", "CAMB3LYP", "cam-b3lyp", "cam_b3lyp"):
        assert dft.rsh_coeff(name) == (0.33, 0.65, 0.19)
        hyb, terms, level = dft.parse_xc(name)
        assert hyb == 0.19 and level == 1
        assert sorted(terms) == sorted([(0.35, 2), (0.46, 12), (0.19, 4), (0.81, 5)])
        assert dft.xc_params(name) == [0.33 if k == 12 else 0.0 for _c, k in terms]
        assert dft.is_rsh(name)
    for name in ("HF", "B3LYP", "B3LYPG", "B3LYP5", "PBE", "PBE0", "LDA", "SVWN", "BLYP", "TPSS", "M062X"):
        hyb = dft.parse_xc(name)[0]
        assert dft.rsh_coeff(name) == (0.0, hyb, hyb)
        assert dft.xc_params(name) is None and not dft.is_rsh(name)
    assert not dft.is_rsh(None)
    with pytest.raises(NotImplementedError):
        dft.rsh_coeff("wB97X")
