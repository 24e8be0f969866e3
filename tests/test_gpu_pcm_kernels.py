"""The C-PCM kernels (`pcm_*` in csrc/mi355scf.hip) one by one against exact FP64 references, at every angular class.

  * `pcm_grad_kernel<LA,LB>` and `pcm_int_kernel<LA,LB>`: a synthetic three-atom molecule with one shell of every l = 0..3 per
    atom, so every class occurs on one centre and across two, against the CPU oracle's McMurchie-Davidson (mn|kk) and
    d/dA (mn|kk) with one s shell of exponent zeta^2 / 2 per point (`_with_points`: (mn|kk) = B_g,mn exactly).  The points are
    the test's own: random ones plus a point on a nucleus, a far one and the two ends of the zeta range.
  * `PCMSolvent.grad` at fixed density on water/cc-pVTZ against four-point differences of `PCMSolvent.energy`.
  * `pcm_pack_kernel`, `pcm_potential_kernel`, `pcm_fock_partial_kernel`, `pcm_fock_finalize_kernel` on synthetic B at the
    column counts and row counts where their loops change branch, against the same contraction in long double with the
    forward-error bound of an FP64 dot product.
Each test prints its figures (pytest -rP shows them)."""
import numpy as np
import pytest
import torch

from test_gpu_dense_kernels import U, assert_guard, guarded
from test_gpu_pcm import _oracle_B, _unpack, _with_points

pytestmark = pytest.mark.gpu

WATER = "O 0 0 0; H 0 -0.757 0.587; H 0 0.757 0.587"
H2CO = "C 0 0 0; O 1.2 0 0; H -0.5 0.9 0; H -0.5 -0.9 0"
SYNTH_ATOMS = "He 0 0 0; Be 0.3 1.1 -0.4; C -0.9 0.2 0.8"          # Bohr, general positions
NPTS = 70
TOL = 1e-11                                                          # test_B_matches_oracle_eris' bound for this integral family
_CACHE = {}


def _mol(atom, basis, **kw):
    from mi355scf.mole import Mole
    return Mole(atom=atom, basis=basis, verbose=0, **kw).build()


def _synthetic():
    """Three atoms, each carrying one two-primitive shell of every l = 0..3 (exponents differ per atom): 12 shells, 48 AOs,
    shell index of (atom a, l) = 4 a + l."""
    if "mol" not in _CACHE:
        mol = _mol(SYNTH_ATOMS, _synthetic_basis(), unit="Bohr")
        assert mol._bas.shape[0] == 12 and mol.nao == 48
        _CACHE["mol"] = mol
    return _CACHE["mol"]


def _synthetic_basis():
    return {el: [[l, [1.3 + 0.2 * a + 0.1 * l, 0.6], [0.45 + 0.05 * a, 0.5]] for l in range(4)]
            for a, el in enumerate(("He", "Be", "C"))}


def _synthetic_with_ghost():
    """`_synthetic` plus a fourth centre, a ghost carrying C's four shells (the one-electron kernels' every-class tests): 16
    shells, 64 AOs, nuclear charges 2, 4, 6, 0."""
    if "ghost" not in _CACHE:
        basis = _synthetic_basis()
        basis["Ghost:C"] = basis["C"]
        mol = _mol(SYNTH_ATOMS + "; Ghost:C 1.4 -0.8 0.5", basis, unit="Bohr")
        assert mol._bas.shape[0] == 16 and mol.nao == 64 and list(mol._atm[:, 0]) == [2, 4, 6, 0]
        _CACHE["ghost"] = mol
    return _CACHE["ghost"]


def _points():
    """(pts [70, 4] = x, y, z, zeta; blocks [3, 3]): random points (sigma 2.5 Bohr, zeta log-uniform in [0.3, 20]) and four
    extremes of the Boys argument x = p theta |PC|^2, theta = zeta^2 / (p + zeta^2): a point on the Be nucleus (x = 0 for the
    one-centre Be pairs), one 56 Bohr away (large-x branch), zeta = 60 (theta -> 1) and zeta = 0.05 (theta -> 0).  Blocks of 1,
    64 and 5 points: a one-lane workgroup, a full wave and a partial one."""
    if "pts" not in _CACHE:
        mol = _synthetic()
        rng = np.random.default_rng(11)
        pts = np.empty((NPTS, 4))
        pts[:, :3] = 2.5 * rng.standard_normal((NPTS, 3))
        pts[:, 3] = np.exp(rng.uniform(np.log(0.3), np.log(20.0), NPTS))
        pts[1, :3] = mol.atom_coords()[1]                  # first lane of the full block: exactly on Be
        pts[64, :3] = [32.0, -36.0, 28.0]                  # last lane of the full block: |s| = 55.7 Bohr
        assert np.linalg.norm(pts[64, :3] - mol.atom_coords(), axis=1).min() > 50.0
        pts[30, 3] = 0.05
        pts[66, 3] = 60.0                                  # in the partial block
        blk = np.array([[0, 1, 0], [1, 64, 1], [65, NPTS - 65, 2]], dtype=np.int32)
        _CACHE["pts"] = (pts, blk)
    return _CACHE["pts"]


def _engine(key, make):
    from mi355scf.engine import Engine
    if ("eng", key) not in _CACHE:
        mol = make()
        _CACHE["eng", key] = (mol, Engine(mol))
    return _CACHE["eng", key]


def _dev(x, eng):
    return torch.as_tensor(np.ascontiguousarray(x), device=eng.device)


def _pair_classes(mol, pairs):
    """{(l_i, l_j): [row, ...]} of a pair list, with the assertion that every class holds a one-centre and a two-centre pair."""
    l, at = mol._bas[:, 1], mol._bas[:, 0]
    cls = {}
    for p, (i, j) in enumerate(pairs):
        cls.setdefault((int(l[i]), int(l[j])), []).append(p)
    for c, rows in cls.items():
        same = [at[pairs[p, 0]] == at[pairs[p, 1]] for p in rows]
        assert any(same) and not all(same), f"class {c}: one-centre and two-centre pairs are not both present"
    return cls


# ---- 1. pcm_grad_kernel<LA,LB> ----------------------------------------------------------------------------------------------
def _derivative_blocks(pairs):
    """dI[p] [npts, 3, d_i, d_j] = d/dA_i (i j | k_g k_g) of the oracle for the ordered pairs `pairs`, computed once."""
    if "dI" not in _CACHE:
        from oracle import oracle as orc
        mol = _synthetic()
        pts, _blk = _points()
        o = orc.Oracle(_with_points(mol, pts[:, :3], pts[:, 3]))
        nb = mol._bas.shape[0]
        dI = [np.stack([o.eri_ip1_shell(i, j, nb + g, nb + g)[:, :, :, 0, 0] for g in range(NPTS)]) for i, j in pairs]
        assert all(np.isfinite(d).all() for d in dI)
        _CACHE["dI"] = (pairs.copy(), dI)
    assert np.array_equal(_CACHE["dI"][0], pairs)
    return _CACHE["dI"][1]


def _grad_ref(mol, pairs, blk, D, q):
    dI = _derivative_blocks(pairs)
    loc = mol.ao_loc_nr()
    ref = np.zeros((len(pairs), blk.shape[0], 3))
    for p, (i, j) in enumerate(pairs):
        Dij = D[loc[i]:loc[i + 1], loc[j]:loc[j + 1]]
        per_point = -2.0 * q[:, None] * np.einsum("gxmn,mn->gx", dI[p], Dij)
        for b, (first, count, _own) in enumerate(blk):
            ref[p, b] = per_point[first:first + count].sum(axis=0)
    return ref


@pytest.mark.parametrize("symmetric", [True, False])
def test_pcm_grad_matches_exact_derivative_integrals_every_class(symmetric):
    """part[pair, block, :] = -2 sum_{g in block} q_g sum_{m in i, n in j} D_mn d/dA_i (mn|kk)_g for all 144 ordered shell pairs
    of the synthetic molecule (16 classes, each on one centre and across two) and the blocks of 1, 64 and 5 points, with a
    symmetric and a non-symmetric D; bound 1e-11 max(1, |ref|max of the class).  The launch repeated gives the same bits.

    Observed on the MI355X, worst |part - ref| / max(1, |ref|max) per class <LA,LB> over both densities (|ref|max 3 .. 64):
      <0,0> 7.6e-15  <0,1> 1.2e-15  <0,2> 1.9e-15  <0,3> 2.0e-15    <1,0> 2.1e-15  <1,1> 2.1e-15  <1,2> 2.0e-15  <1,3> 3.0e-15
      <2,0> 9.7e-16  <2,1> 1.6e-15  <2,2> 1.8e-15  <2,3> 2.8e-15    <3,0> 2.0e-15  <3,1> 1.8e-15  <3,2> 2.8e-15  <3,3> 6.2e-15
    so the starting bound of 1e-11 stands (it was not widened).  With NR one short in the kernel the eight classes of odd LA + LB
    miss by 5e-4 .. 1e-1; without the i gt[i-1] term in the f classes alone, <3,*> miss by 1 .. 3 while the water/6-31G*
    finite-difference test still passes."""
    mol, eng = _engine("synthetic", _synthetic)
    pts, blk = _points()
    pairs = eng.pcm_pairs(ordered=True)
    assert pairs.shape == (144, 2)
    cls = _pair_classes(mol, pairs)
    assert sorted(cls) == [(a, b) for a in range(4) for b in range(4)]
    rng = np.random.default_rng(21 + symmetric)
    A = rng.standard_normal((mol.nao, mol.nao))
    D = A + A.T if symmetric else A
    q = rng.standard_normal(NPTS)
    ref = _grad_ref(mol, pairs, blk, D, q)

    n = len(pairs) * blk.shape[0] * 3
    flat = guarded(n)
    dpts, dblk, dD, dq = _dev(pts, eng), _dev(blk, eng), _dev(D, eng), _dev(q, eng)
    eng.pcm_grad(dpts, dblk, dD, dq, flat[:n])
    torch.cuda.synchronize()
    assert_guard(flat, n, "pcm_grad")
    again = guarded(n)
    eng.pcm_grad(dpts, dblk, dD, dq, again[:n])
    assert torch.equal(flat[:n], again[:n]), "pcm_grad: two launches differ (fixed-order sums promised)"
    got = flat[:n].cpu().numpy().reshape(ref.shape)
    assert np.isfinite(got).all()

    bad, lines = [], []
    for c in sorted(cls):
        rows = cls[c]
        scale = max(1.0, np.abs(ref[rows]).max())
        err = np.abs(got[rows] - ref[rows]).max()
        blk_err = [np.abs(got[rows][:, b] - ref[rows][:, b]).max() for b in range(blk.shape[0])]
        lines.append(f"pcm_grad<{c[0]},{c[1]}> sym={symmetric}: |err|max = {err:.2e}, |ref|max = {scale:.2e}, "
                     f"rel = {err / scale:.2e}, per block = {', '.join(f'{e:.1e}' for e in blk_err)}")
        if not err <= TOL * scale:
            bad.append(lines[-1])
    print("\n".join(lines))
    assert not bad, "classes over 1e-11 max(1, |ref|):\n" + "\n".join(bad)


# ---- 2. pcm_int_kernel<LA,LB> -----------------------------------------------------------------------------------------------
def _B_ref():
    if "Bref" not in _CACHE:
        mol = _synthetic()
        pts, _blk = _points()
        _CACHE["Bref"] = _oracle_B(mol, pts[:, :3], pts[:, 3])
        assert np.isfinite(_CACHE["Bref"]).all()
    return _CACHE["Bref"]


@pytest.mark.parametrize("pad", [0, 32])
def test_pcm_eval_matches_oracle_every_class_and_extreme_points(pad):
    """B of the synthetic molecule at the 70 points against (mn|kk) of the oracle, all rows, with ld = nao (nao + 1) / 2 = 1176
    (even: no padding at all) and ld = 1176 + 32 (padding columns exactly zero); bound 1e-11 max(1, |ref|max of the class).
    What this adds over test_B_matches_oracle_eris: `pcm_int_kernel<3,3>` (and every other class) with its two shells on
    different centres, and the four extreme points -- on a nucleus, 56 Bohr away, zeta = 60 and zeta = 0.05 -- where the
    Boys argument leaves the range a cavity point gives.

    Observed on the MI355X, |B - ref|max per class <LA,LB> (|ref|max 1.0 .. 1.4; the same for both ld):
      <0,0> 4.2e-15  <1,0> 4.7e-15  <1,1> 2.7e-15  <2,0> 5.8e-16  <2,1> 6.9e-16  <2,2> 2.2e-15  <3,0> 6.1e-16  <3,1> 6.1e-16
      <3,2> 9.2e-16  <3,3> 1.2e-15; at the extreme points: on Be 4.2e-15, far 1.7e-17, zeta = 0.05 6.9e-17, zeta = 60 6.1e-16.
    The starting bound of 1e-11 stands."""
    mol, eng = _engine("synthetic", _synthetic)
    pts, blk = _points()
    nao = mol.nao
    npair = nao * (nao + 1) // 2
    ld = npair + pad
    assert npair == 1176 and ld % 2 == 0
    pairs = eng.pcm_pairs(ordered=False)
    assert pairs.shape == (78, 2)
    cls = _pair_classes(mol, pairs)
    assert sorted(cls) == [(a, b) for a in range(4) for b in range(a + 1)]
    ref = _B_ref()

    flat = guarded(NPTS * ld)
    B = flat[:NPTS * ld].view(NPTS, ld)
    eng.pcm_eval(_dev(pts, eng), _dev(blk, eng), ld, B)
    torch.cuda.synchronize()
    assert_guard(flat, NPTS * ld, "pcm_eval")
    Bh = B.cpu().numpy()
    assert np.isfinite(Bh).all()
    assert np.all(Bh[:, npair:] == 0.0), "padding columns are not exactly zero"
    got = np.stack([_unpack(Bh[g], nao) for g in range(NPTS)])

    loc = mol.ao_loc_nr()
    extreme = {"on Be": 1, "far": 64, "zeta 0.05": 30, "zeta 60": 66}
    bad, lines = [], []
    for c in sorted(cls):
        err = scale = 0.0
        worst_g = np.zeros(NPTS)
        for p in cls[c]:
            i, j = pairs[p]
            d = np.abs(got[:, loc[i]:loc[i + 1], loc[j]:loc[j + 1]] - ref[:, loc[i]:loc[i + 1], loc[j]:loc[j + 1]])
            worst_g = np.maximum(worst_g, d.max(axis=(1, 2)))
            scale = max(scale, np.abs(ref[:, loc[i]:loc[i + 1], loc[j]:loc[j + 1]]).max())
        err, scale = worst_g.max(), max(1.0, scale)
        lines.append(f"pcm_int<{c[0]},{c[1]}> ld={ld}: |err|max = {err:.2e} (point {int(worst_g.argmax())}), |ref|max = {scale:.2e}; "
                     + ", ".join(f"{k}: {worst_g[g]:.1e}" for k, g in extreme.items()))
        if not err <= TOL * scale:
            bad.append(lines[-1])
    print("\n".join(lines))
    assert not bad, "classes over 1e-11 max(1, |ref|):\n" + "\n".join(bad)


# ---- 3. the assembled solvent gradient at fixed density ---------------------------------------------------------------------
FD_H = 2e-3          # Bohr: at 4e-3 a point of H2's sphere reaches swf = 0 within the +-4h of the wider stencil and is dropped


def _fixed_density(mol):
    """Core-guess closed-shell density plus a random symmetric perturbation: symmetric, O(1), no SCF."""
    from oracle import oracle as orc
    S, T, V, _ = orc.Oracle(mol).int1e()
    w, U_ = np.linalg.eigh(S)
    X = U_ / np.sqrt(w)
    _e, c = np.linalg.eigh(X.T @ (T + V) @ X)
    C = X @ c[:, :mol.nelectron // 2]
    A = np.random.default_rng(41).standard_normal(S.shape)
    return 2.0 * C @ C.T + 0.02 * (A + A.T)


def _solvent(mol):
    from mi355scf.engine import Engine
    from mi355scf.pcm import PCMSolvent
    return PCMSolvent(mol).build(Engine(mol), mol)


def _water_tz():
    if "wtz" not in _CACHE:
        mol = _mol(WATER, "cc-pVTZ")
        assert mol._bas[:, 1].max() == 3 and mol.nao == 58
        D = _fixed_density(mol)
        ws = _solvent(mol)
        _CACHE["wtz"] = (mol, D, ws, ws.grad(D))
    return _CACHE["wtz"]


@pytest.mark.parametrize("ia,x", [(0, 2), (1, 1), (2, 0)])
def test_solvent_gradient_matches_four_point_differences_with_f_shells(ia, x):
    """`PCMSolvent.grad(D)` on water/cc-pVTZ (f on O, d on H, deep s contractions) against the four-point central difference of
    `PCMSolvent.energy(D)` with the same D at every displaced geometry: besides the AO-centre share of `pcm_grad` this is the
    only check of the points' share (-per_blk to the owner), `grad_vnuc` and `grad_s` inside `grad()`.  One component per atom.
    Bound: max(1e-8, 10 |fd4(h) - fd4(2h)|), h = 2e-3 Bohr -- the difference of the two stencils is 15x the h^4 truncation
    error of fd4(h), the reference's own error.  The surface keeps its point count at every displaced geometry (no point
    crosses SWF_DROP), so the energy is smooth along the path.

    Observed on the MI355X: |analytic - fd4(h)| = 2.8e-11, 1.7e-12, 7.3e-12 for (O, z), (H1, y), (H2, x) with
    |fd4(h) - fd4(2h)| = 4.2e-10, 2.5e-11, 1.1e-10: the floor of 1e-8 is the bound in all three."""
    mol, D, ws, g = _water_tz()
    npts = ws.surface.npts
    E = {}
    for k in (-4, -2, -1, 1, 2, 4):
        R = mol.atom_coords().copy()
        R[ia, x] += k * FD_H
        md = mol.set_geom_(R, unit="Bohr", inplace=False)
        wd = _solvent(md)
        assert wd.surface.npts == npts, (k, wd.surface.npts, npts)
        E[k] = wd.energy(D)
    fd_h = (-E[2] + 8 * E[1] - 8 * E[-1] + E[-2]) / (12 * FD_H)
    fd_2h = (-E[4] + 8 * E[2] - 8 * E[-2] + E[-4]) / (24 * FD_H)
    tol = max(1e-8, 10 * abs(fd_h - fd_2h))
    print(f"PCM grad water/cc-pVTZ atom {ia} dir {x}: analytic {g[ia, x]:.12f}, fd4(h) {fd_h:.12f}, fd4(2h) {fd_2h:.12f}, "
          f"|an - fd4(h)| = {abs(g[ia, x] - fd_h):.2e}, tol = {tol:.2e}")
    assert abs(g[ia, x] - fd_h) < tol, (ia, x, g[ia, x], fd_h, fd_2h, tol)


def test_solvent_gradient_is_translationally_invariant_with_f_shells():
    """The three atoms' solvent gradients sum to zero within 1e-9 (observed 5e-16 at |g|max = 3.5e-2)."""
    _mol_, _D, _ws, g = _water_tz()
    print(f"PCM grad water/cc-pVTZ: sum over atoms = {g.sum(axis=0)}, |g|max = {np.abs(g).max():.3e}")
    assert np.abs(g).max() > 1e-4
    assert np.abs(g.sum(axis=0)).max() < 1e-9


# ---- 4. the per-cycle passes at their edge shapes ---------------------------------------------------------------------------
# nao -> n2 = ld / 2 at the smallest even ld: the branch of pcm_potential_kernel's loop `for (; c + 256 < n2; c += 512)` + tail
CONTEXTS = {
    "h2/sto-3g": (lambda: _mol("H 0 0 0; H 0 0 0.74", "sto-3g"), 2, 2),            # two threads of one wave hold a column pair
    "water/cc-pvdz": (lambda: _mol(WATER, "cc-pVDZ"), 24, 150),                    # tail only, part of the workgroup
    "h2co/6-31g(d)": (lambda: _mol(H2CO, "6-31G(d)"), 32, 264),                    # unrolled body for 8 threads only
    "synthetic": (_synthetic, 48, 588),                                            # one unrolled trip, tail for 76 threads
    "water/cc-pvtz": (lambda: _mol(WATER, "cc-pVTZ"), 58, 856),                    # second trip partial; one padding column
}
ROWS = (1, 2, 3, 65, 131, 1001)


def _chunks(npts, ld):
    from mi355scf.engine import Engine
    nchunk = Engine.pcm_fock_chunks(npts, ld)
    return nchunk, -(-npts // nchunk)


def _min_ld(nao):
    npair = nao * (nao + 1) // 2
    return npair, npair + (npair & 1)


def test_per_cycle_case_list_reaches_every_branch():
    """The (context, npts) grid of the two tests below holds: n2 <= 256, 256 < n2 <= 512, n2 > 512 with a partial second trip;
    a padded and an unpadded ld; an odd rows_per (tail only, and loop body plus tail), an even one, a chunk that starts at or
    beyond npts, a last chunk shorter than rows_per, nchunk = 1 and npts = 1."""
    n2s = []
    for name, (_make, nao, n2) in CONTEXTS.items():
        npair, ld = _min_ld(nao)
        assert ld // 2 == n2, (name, ld)
        n2s.append(n2)
    assert any(n <= 256 for n in n2s) and any(256 < n <= 512 for n in n2s) and any(512 < n < 1024 and n % 512 for n in n2s)
    assert any(_min_ld(nao)[0] & 1 for _m, nao, _n in CONTEXTS.values()) and any(not _min_ld(nao)[0] & 1 for _m, nao, _n in CONTEXTS.values())
    seen = set()
    for _make, nao, _n2 in CONTEXTS.values():
        ld = _min_ld(nao)[1]
        for npts in ROWS:
            nchunk, rp = _chunks(npts, ld)
            assert 1 <= nchunk <= 64 and nchunk * rp >= npts
            seen.add("nchunk 1" if nchunk == 1 else "nchunk > 1")
            seen.add("rows_per 1" if rp == 1 else ("odd rows_per > 1" if rp & 1 else "even rows_per"))
            if (nchunk - 1) * rp >= npts:
                seen.add("empty chunk")
            if npts % rp:
                seen.add("short last chunk")
    assert seen >= {"nchunk 1", "nchunk > 1", "rows_per 1", "odd rows_per > 1", "even rows_per", "empty chunk", "short last chunk"}, seen
    assert 1 in ROWS


def _synthetic_B(npts, npair, ld, seed):
    rng = np.random.default_rng(seed)
    B = np.zeros((npts, ld))
    B[:, :npair] = rng.standard_normal((npts, npair)) * np.exp(rng.uniform(-2, 2, npair))
    return B, rng


def _pack_ref(D):
    """d_c = D_mn + D_nm (one FP64 addition: the same bits on any IEEE machine), D_mm on the diagonal."""
    m, n = np.tril_indices(D.shape[0])
    return np.where(m == n, D[m, n], D[m, n] + D[n, m])


@pytest.mark.parametrize("context", list(CONTEXTS))
def test_pcm_potential_within_rounding_bound(context):
    """v = vn - B d and v = B d on random B with exactly zero padding, symmetric and non-symmetric D, for every row count.
    `dpack` must equal the packed D bit for bit (padding untouched: zero); v is compared with the long-double contraction of the
    unpadded columns with that d: |v - ref| <= 2 n u sum|terms|, u = 2^-53, n = the number of terms (the packed pairs, plus
    vn) -- the forward-error bound of a length-n FP64 dot product, doubled for the split accumulators (s0, s1, the wave and
    workgroup trees).  The long-double reference itself is good to n 2^-64.  Repeated calls give the same bits.
    Observed worst |err| / bound: 0.31 at n2 = 2, below 2e-3 for the four larger contexts."""
    make, nao, n2 = CONTEXTS[context]
    mol, eng = _engine(context, make)
    assert mol.nao == nao
    npair, ld = _min_ld(nao)
    worst = 0.0
    for npts in ROWS:
        B, rng = _synthetic_B(npts, npair, ld, 1000 * nao + npts)
        dB = _dev(B, eng)
        for symmetric in (True, False):
            A = rng.standard_normal((nao, nao))
            D = A + A.T if symmetric else A
            vn = rng.standard_normal(npts)
            d = _pack_ref(D)
            Bl, dl = B[:, :npair].astype(np.longdouble), d.astype(np.longdouble)
            dot = Bl @ dl
            mag = np.abs(Bl) @ np.abs(dl)
            for use_vn in (True, False):
                fd, fv = guarded(ld, np.zeros(ld)), guarded(npts)
                eng.pcm_potential(dB, ld, _dev(D, eng), fd[:ld], _dev(vn, eng) if use_vn else None, fv[:npts])
                torch.cuda.synchronize()
                assert_guard(fd, ld, "dpack")
                assert_guard(fv, npts, "v")
                dp = fd[:ld].cpu().numpy()
                assert np.array_equal(dp[:npair], d), (context, npts, symmetric, "dpack")
                assert np.all(dp[npair:] == 0.0), "dpack padding written"
                fv2 = guarded(npts)
                eng.pcm_potential(dB, ld, _dev(D, eng), fd[:ld], _dev(vn, eng) if use_vn else None, fv2[:npts])
                assert torch.equal(fv[:npts], fv2[:npts])
                got = fv[:npts].cpu().numpy().astype(np.longdouble)
                ref = vn - dot if use_vn else dot
                n = npair + int(use_vn)
                bound = 2.0 * n * U * (mag + (np.abs(vn) if use_vn else 0.0))
                ratio = float(np.max(np.abs(got - ref) / bound))
                worst = max(worst, ratio)
                assert ratio <= 1.0, (context, npts, symmetric, use_vn, ratio)
    print(f"[rounding] pcm_potential {context} (n2 = {n2}): worst |err| / bound = {worst:.3g}")


@pytest.mark.parametrize("context", list(CONTEXTS))
def test_pcm_fock_within_rounding_bound(context):
    """V = scale unpack(q^T B) and V += scale unpack(q^T B) on random B for every row count (nchunk and rows_per from
    mi_pcm_fock_chunks: odd and even rows_per, empty chunks, one chunk), against the long-double sum over the points:
    |V - ref| <= 2 n u sum|terms|, n = npts (+ 1 for the accumulated V), the forward-error bound of a length-n FP64 sum doubled
    for the split accumulators of the row-pair loop (the scales are powers of two: no rounding of their own).  V is exactly
    symmetric and a repeated call gives the same bits.  Observed worst |err| / bound: 0.34 .. 0.49 (npts = 1: one rounding
    against a bound of two)."""
    make, nao, n2 = CONTEXTS[context]
    mol, eng = _engine(context, make)
    npair, ld = _min_ld(nao)
    m, k = np.tril_indices(nao)
    worst = 0.0
    for npts in ROWS:
        B, rng = _synthetic_B(npts, npair, ld, 2000 * nao + npts)
        q = rng.standard_normal(npts)
        V0 = rng.standard_normal((nao, nao))
        V0 = V0 + V0.T
        nchunk, _rp = _chunks(npts, ld)
        Bl = B[:, :npair].astype(np.longdouble)
        s = q.astype(np.longdouble) @ Bl
        mag = np.abs(q).astype(np.longdouble) @ np.abs(Bl)
        dB, dq = _dev(B, eng), _dev(q, eng)
        for scale, acc in ((-1.0, False), (0.5, True)):
            fp, fV = guarded(nchunk * ld), guarded(nao * nao, V0 if acc else None)
            V = fV[:nao * nao].view(nao, nao)
            eng.pcm_fock(dB, ld, dq, scale, acc, fp[:nchunk * ld], V)
            torch.cuda.synchronize()
            assert_guard(fp, nchunk * ld, "part")
            assert_guard(fV, nao * nao, "V")
            assert torch.equal(V, V.T), (context, npts, "V not symmetric")
            fV2 = guarded(nao * nao, V0 if acc else None)
            eng.pcm_fock(dB, ld, dq, scale, acc, fp[:nchunk * ld], fV2[:nao * nao].view(nao, nao))
            assert torch.equal(fV[:nao * nao], fV2[:nao * nao])
            got = V.cpu().numpy().astype(np.longdouble)
            ref = np.zeros((nao, nao), dtype=np.longdouble)
            ref[m, k] = scale * s
            ref[k, m] = ref[m, k]
            tot = np.zeros((nao, nao), dtype=np.longdouble)
            tot[m, k] = abs(scale) * mag
            tot[k, m] = tot[m, k]
            if acc:
                ref += V0
                tot += np.abs(V0)
            bound = 2.0 * (npts + int(acc)) * U * tot
            ratio = float(np.max(np.abs(got - ref) / bound))
            worst = max(worst, ratio)
            assert ratio <= 1.0, (context, npts, scale, acc, ratio)
    print(f"[rounding] pcm_fock {context} (n2 = {n2}): worst |err| / bound = {worst:.3g}")
