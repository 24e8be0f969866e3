"""Long-double references for the DFT grid front end: AO values on the grid, Becke weights, densities from AO or orbital
values, and the Cholesky solve of the low-rank factor.  Plain NumPy on the host, written from the formulas and not from
oracle/dft.py (which the host tests compare them with), so a slip in either shows.

Every reference comes with a *majorant*: the same expression with each term replaced by its absolute value.  A kernel that
evaluates the expression in FP64 in any order is within a small multiple of u = 2^-53 times the majorant; cancellation
between terms (mixed-sign contraction coefficients, c2s rows, the two halves of a gradient) cannot excuse more."""
import math

import numpy as np

LD = np.longdouble
assert np.finfo(LD).eps < 2e-19, "these references need an 80-bit (or wider) long double"

NCOMP = {0: 1, 1: 4, 2: 10}
HESS = [(i, j) for i in range(3) for j in range(i, 3)]          # xx, xy, xz, yy, yz, zz


def _c2s(l):
    from oracle import dft as odft
    return odft._c2s(l).astype(LD)


def _monomials(d, l, k):
    """(value, |value|) [ng][ncart] of d^k (x^lx y^ly z^lz) for the derivative multi-index k, cartesians in the order
    lx = l..0, ly = l-lx..0."""
    pw = [(lx, ly, l - lx - ly) for lx in range(l, -1, -1) for ly in range(l - lx, -1, -1)]
    out = np.zeros((d.shape[0], len(pw)), dtype=LD)
    for c, p in enumerate(pw):
        if all(k[q] <= p[q] for q in range(3)):
            f = np.ones(d.shape[0], dtype=LD)
            for q in range(3):
                f = f * LD(math.perm(p[q], k[q])) * d[:, q] ** (p[q] - k[q])
            out[:, c] = f
    return out, np.abs(out)


def ao_reference(mol, pts, deriv):
    """(ref, majorant), both [ncomp][ng][nao]: the real-spherical contracted AOs at `pts` with their gradient (deriv >= 1) and
    second derivatives xx, xy, xz, yy, yz, zz (deriv == 2).  chi = R(r^2) S(x, y, z) with R = sum_p c_p exp(-a_p r^2) and S the
    c2s combination of the cartesian monomials; d_i R = R1 x_i with R1 = sum_p -2 a_p c_p e_p, and d_i d_j R = R2 x_i x_j +
    delta_ij R1 with R2 = sum_p 4 a_p^2 c_p e_p.  In the majorant each primitive carries the factor (1 + a r^2): the argument
    a r^2 of exp is itself rounded, which moves exp by the relative amount a r^2 u."""
    pts = np.asarray(pts, dtype=np.float64).astype(LD)
    ng, nao = pts.shape[0], mol.nao
    ref = np.zeros((NCOMP[int(deriv)], ng, nao), dtype=LD)
    maj = np.zeros_like(ref)
    loc = mol.ao_loc_nr()
    unit = [tuple(int(q == c) for q in range(3)) for c in range(3)]
    for ish in range(mol.nbas):
        ia, l, npr, _, _, pe, pc, _ = (int(v) for v in mol._bas[ish])
        a = mol._env[pe:pe + npr].astype(LD)
        c = mol._env[pc:pc + npr].astype(LD)
        p0 = int(mol._atm[ia, 1])
        d = pts - mol._env[p0:p0 + 3].astype(LD)
        r2 = (d * d).sum(axis=1)
        ar2 = np.outer(r2, a)
        e = np.exp(-ar2)                                         # [ng][np]
        ew = e * (1 + ar2)
        rad, radm = e @ c, ew @ np.abs(c)
        r1, r1m = e @ (-2 * a * c), ew @ np.abs(2 * a * c)
        r2d, r2m = e @ (4 * a * a * c), ew @ np.abs(4 * a * a * c)
        c2s = _c2s(l)
        ac2s = np.abs(c2s)

        def ang(k):
            v, av = _monomials(d, l, k)
            return v @ c2s, av @ ac2s
        s, sm = ang((0, 0, 0))
        sl = slice(loc[ish], loc[ish + 1])
        ref[0][:, sl] = rad[:, None] * s
        maj[0][:, sl] = radm[:, None] * sm
        if deriv >= 1:
            s1 = [ang(unit[q]) for q in range(3)]
            ad = np.abs(d)
            for q in range(3):
                ref[1 + q][:, sl] = (r1 * d[:, q])[:, None] * s + rad[:, None] * s1[q][0]
                maj[1 + q][:, sl] = (r1m * ad[:, q])[:, None] * sm + radm[:, None] * s1[q][1]
        if deriv >= 2:
            for m, (i, j) in enumerate(HESS):
                s2, s2m = ang(tuple(unit[i][q] + unit[j][q] for q in range(3)))
                ref[4 + m][:, sl] = ((r2d * d[:, i] * d[:, j] + (r1 if i == j else 0))[:, None] * s
                                     + (r1 * d[:, i])[:, None] * s1[j][0] + (r1 * d[:, j])[:, None] * s1[i][0] + rad[:, None] * s2)
                maj[4 + m][:, sl] = ((r2m * ad[:, i] * ad[:, j] + (r1m if i == j else 0))[:, None] * sm
                                     + (r1m * ad[:, i])[:, None] * s1[j][1] + (r1m * ad[:, j])[:, None] * s1[i][1]
                                     + radm[:, None] * s2m)
    return ref, maj


def becke_reference(coords, atom_of, vol, R, a):
    """(w [ng], psum [ng]): w = vol P_owner / sum_i P_i with the cell functions P_i = prod_{j != i} (1 - f3(nu_ij)) / 2,
    nu_ij = mu_ij + a_ij (1 - mu_ij^2), mu_ij = (r_i - r_j) / R_ij and f3 the three times iterated f(x) = (3 - x^2) x / 2.
    Every ordered pair is evaluated with its own a_ij (the kernel's convention: `a` need not be antisymmetric)."""
    coords, R = np.asarray(coords, dtype=np.float64).astype(LD), np.asarray(R, dtype=np.float64).astype(LD)
    a, vol = np.asarray(a, dtype=np.float64).astype(LD), np.asarray(vol, dtype=np.float64).astype(LD)
    natm = R.shape[0]
    dg = coords[:, None, :] - R[None, :, :]
    r = np.sqrt((dg * dg).sum(axis=2))                            # [ng][natm]
    dR = R[:, None, :] - R[None, :, :]
    Rij = np.sqrt((dR * dR).sum(axis=2))
    P = np.ones_like(r)
    for i in range(natm):
        oth = np.arange(natm) != i
        mu = (r[:, i:i + 1] - r[:, oth]) / Rij[i, oth][None, :]
        mu = mu + a[i, oth][None, :] * (1 - mu * mu)
        for _ in range(3):
            mu = (3 - mu * mu) * mu / 2
        P[:, i] = np.prod((1 - mu) / 2, axis=1)
    psum = P.sum(axis=1)
    w = vol * P[np.arange(len(vol)), np.asarray(atom_of)] / psum
    return w, psum


def rho_mo_reference(psi):
    """psi [(1|4)][nocc][ng] -> {"rho": [(1|4)][ng], "tau": [ng] or None} and the same dict of majorants: rho = sum_i psi_i^2,
    grad rho = 2 sum_i psi_i grad psi_i, tau = 1/2 sum_i |grad psi_i|^2."""
    psi = np.asarray(psi).astype(LD)
    ap = np.abs(psi)
    rho, maj = [(psi[0] * psi[0]).sum(axis=0)], [(ap[0] * ap[0]).sum(axis=0)]
    tau = taum = None
    if psi.shape[0] > 1:
        for k in (1, 2, 3):
            rho.append(2 * (psi[0] * psi[k]).sum(axis=0))
            maj.append(2 * (ap[0] * ap[k]).sum(axis=0))
        tau = (psi[1:4] * psi[1:4]).sum(axis=(0, 1)) / 2
        taum = tau.copy()
    return {"rho": np.array(rho), "tau": tau}, {"rho": np.array(maj), "tau": taum}


def _psi(ao, Z):
    return np.einsum("mi,cmg->cig", Z, ao)


def rho_reference(ao, Z):
    """ao [(1|4)][nao][ng], Z [nao][rank] -> `rho_mo_reference` of psi = Z^T ao.  The majorants are those of the two-level sum
    psi_i = sum_m z_mi ao_m, rho = sum_i psi_i^2: they are built from |psi|_i = sum_m |z_mi| |ao_m|, so a cancellation inside
    psi_i is not credited."""
    ao, Z = np.asarray(ao).astype(LD), np.asarray(Z).astype(LD)
    val, _ = rho_mo_reference(_psi(ao, Z))
    _, maj = rho_mo_reference(_psi(np.abs(ao), np.abs(Z)))
    return val, maj


def rho_c_reference(ao, C):
    """ao [(1|4)][nao][ng], C [nao][ng] -> (rho, majorant) [(1|4)][ng] of `xc_rho`: rho_0 = sum_m ao_0m C_m and
    rho_k = 2 sum_m ao_km C_m."""
    ao, C = np.asarray(ao).astype(LD), np.asarray(C).astype(LD)
    f = np.array([1] + [2] * (ao.shape[0] - 1), dtype=LD)[:, None]
    return f * (ao * C[None]).sum(axis=1), f * (np.abs(ao) * np.abs(C)[None]).sum(axis=1)


def cholesky_solve_reference(M, W):
    """(Zt [nocc][n], info): M [nocc][nocc] = L L^T (lower triangle read) and Zt = L^-1 W^T by forward substitution, in plain
    loops (nocc <= 64).  info is 0, or k + 1 for the first pivot that is not positive and finite (LAPACK's convention); Zt is
    then None."""
    M, W = np.asarray(M).astype(LD), np.asarray(W).astype(LD)
    nocc = M.shape[0]
    assert M.shape == (nocc, nocc) and W.shape[1] == nocc and nocc <= 64
    L = np.zeros((nocc, nocc), dtype=LD)
    for k in range(nocc):
        d = M[k, k]
        for j in range(k):
            d = d - L[k, j] * L[k, j]
        if not (d > 0 and np.isfinite(d)):
            return None, k + 1
        L[k, k] = np.sqrt(d)
        for i in range(k + 1, nocc):
            s = M[i, k]
            for j in range(k):
                s = s - L[i, j] * L[k, j]
            L[i, k] = s / L[k, k]
    Zt = np.zeros((nocc, W.shape[0]), dtype=LD)
    for i in range(nocc):
        z = W[:, i].copy()
        for j in range(i):
            z = z - L[i, j] * Zt[j]
        Zt[i] = z / L[i, i]
    return Zt, 0


# ------------------------------------------------------------------------------------------------------------------------------
# The inputs of the grid-kernel tests (host and GPU files use the same ones)
# ------------------------------------------------------------------------------------------------------------------------------
NG_FULL = 1025                                                    # one point past four 256-thread workgroups
NG_EDGES = (1, 255, 256, 257)
AO_TINY, AO_FAR = 5, 6                                            # indices of the two underflow points, after the centres


def ao_points(mol):
    """[NG_FULL][3] points for the AO tests, the special ones first so that every prefix of 255 or more holds them: normal
    points (sigma 2.5 Bohr) around the centroid, then overwritten: point c on centre c (c < natm <= 4), point 4 at 1e-9 Bohr
    off the last centre, point AO_TINY 16 Bohr out in a general direction (every AO of the synthetic molecule lies between
    1e-300 and 1e-30 there) and point AO_FAR 200 Bohr out (every primitive underflows: a r^2 > 745)."""
    R = mol.atom_coords()
    assert R.shape[0] <= 4
    rng = np.random.default_rng(20241021 + mol.nao)
    pts = R.mean(axis=0) + 2.5 * rng.standard_normal((NG_FULL, 3))
    pts[:R.shape[0]] = R
    pts[4] = R[-1] + np.array([6e-10, -7e-10, 3.6e-10]) / np.linalg.norm([6, -7, 3.6]) * 10
    pts[AO_TINY] = R.mean(axis=0) + 16.0 * np.array([0.48, -0.6, 0.64])
    pts[AO_FAR] = R.mean(axis=0) + 200.0 * np.array([-0.6, 0.64, 0.48])
    return np.ascontiguousarray(pts)


BECKE_SPACING = 1.9
BECKE_RADII = (0.35, 0.70, 0.60, 1.45, 1.05, 1.00)               # Bragg radii (Angstrom) of H, C, O, Li, Be, S, dealt in turn
BECKE_CLIP = (3, 7)                                               # a[3][7] = +0.5, a[7][3] = -0.5 by hand
BECKE_ON_PARENT, BECKE_ON_OTHER, BECKE_AXIS, BECKE_PLANE, BECKE_FAR = 0, 1, 2, 3, 4


def becke_lattice(natm):
    """The first natm sites of a 5 x 5 x 4 lattice of spacing 1.9 Bohr (x fastest), jittered by up to 0.15 Bohr except for
    atoms 0, 1, 2, which stay exactly on the x axis."""
    assert 3 <= natm <= 100
    idx = np.arange(100)
    R = BECKE_SPACING * np.stack([idx % 5, (idx // 5) % 5, idx // 25], axis=1).astype(np.float64)
    jit = np.random.default_rng(99).uniform(-0.15, 0.15, (100, 3))
    jit[:3] = 0.0
    return np.ascontiguousarray((R + jit)[:natm])


def becke_adjust(natm):
    """Treutler's a_ij = (chi - 1/chi) / 4 ... in the form the grids use, a = clip((rr^T - rr) / 4, -1/2, 1/2) with
    rr_ij = sqrt(rad_i / rad_j), from mixed radii; no pair of these radii reaches the clip, so one pair is put there by hand."""
    rad = np.sqrt(np.array([BECKE_RADII[i % len(BECKE_RADII)] for i in range(natm)]))
    rr = rad[:, None] / rad[None, :]
    a = np.clip(0.25 * (rr.T - rr), -0.5, 0.5)
    assert np.abs(a).max() < 0.5
    i, j = BECKE_CLIP
    a[i, j], a[j, i] = 0.5, -0.5
    assert np.array_equal(a, -a.T)
    return np.ascontiguousarray(a)


def becke_case(natm):
    """(coords [NG_FULL][3], atom_of int32, vol, R, a) on `becke_lattice(natm)`: points at log-uniform distances of 0.05 to 6
    Bohr from random parents, every second one booked to an arbitrary other atom, and five placed by hand: on its parent
    nucleus (w = vol), on a nucleus that is not its parent (w = 0), on the x axis beyond atom 0 with parent 1 (mu = +-1 for the
    collinear pairs: w = 0), on the plane bisecting atoms 0 and 1 (mu = 0), and about 48 Bohr out."""
    R, a = becke_lattice(natm), becke_adjust(natm)
    rng = np.random.default_rng(7000 + natm)
    par = rng.integers(0, natm, NG_FULL)
    u = rng.standard_normal((NG_FULL, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    dist = np.exp(rng.uniform(np.log(0.05), np.log(6.0), NG_FULL))
    coords = R[par] + dist[:, None] * u
    atom_of = np.where(np.arange(NG_FULL) % 2 == 0, par, rng.integers(0, natm, NG_FULL))
    vol = np.exp(rng.uniform(-6.0, 3.0, NG_FULL))
    coords[BECKE_ON_PARENT], atom_of[BECKE_ON_PARENT] = R[natm - 1], natm - 1
    coords[BECKE_ON_OTHER], atom_of[BECKE_ON_OTHER] = R[natm // 2], 5
    coords[BECKE_AXIS], atom_of[BECKE_AXIS] = (-1.3, 0.0, 0.0), 1
    coords[BECKE_PLANE], atom_of[BECKE_PLANE] = (BECKE_SPACING / 2, 0.4, -0.3), 0
    coords[BECKE_FAR], atom_of[BECKE_FAR] = R[0] - 48.0 * np.array([0.6, 0.48, 0.64]), 0
    return np.ascontiguousarray(coords), atom_of.astype(np.int32), vol, R, a
