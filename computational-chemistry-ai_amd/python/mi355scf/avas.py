"""Atomic valence active space (AVAS; Sayfutyarova, Sun, Chan, Knizia, JCTC 13, 4063 (2017)) behind `pyscf.mcscf.avas.avas`
(`templates/calculate_casscf.py:86`) for closed-shell RHF references.

    P      = S12 S22^-1 S21                 projector on the selected reference AOs, in the AO basis of the calculation
    occupied space: eigenvectors of Co^T P Co with eigenvalue > threshold become active, the rest inactive; the same in the
    virtual space.  Orbitals are returned as [inactive occupied | active occupied | active virtual | inactive virtual];
    with `canonicalize` each of the four blocks diagonalises the reference Fock matrix within the block.
    ncas = kept occupied + kept virtual,  nelecas = 2 x kept occupied.

The reference AO set is the molecule's own atoms in STO-3G (`minao="sto-3g"`); PySCF's default is its MINAO set, which this
package does not carry, so selections near the threshold can differ from PySCF's.  The cross overlap S12 is the off-diagonal block
of the ordinary overlap matrix of one molecule that carries both basis sets on every atom (the engine's `int1e`): no integral
code of its own.  `avas_algebra` is the linear algebra alone, a function of arrays.
"""
import re

import numpy as np

from .reference import require


def avas_algebra(C, mo_occ, S, S12, S22, F=None, threshold=0.2, canonicalize=True):
    """-> (ncas, nelecas, mo_coeff, (n_occ_kept, n_vir_kept)).  C [N, nmo]: orbitals with occupations mo_occ (2 / 0);
    S [N, N]: AO overlap; S12 [N, M]: overlap with the M selected reference AOs; S22 [M, M]: their own overlap;
    F [N, N]: the reference Fock matrix (needed with `canonicalize`)."""
    C, S12, S22 = np.asarray(C, dtype=np.float64), np.asarray(S12, dtype=np.float64), np.asarray(S22, dtype=np.float64)
    mo_occ = np.asarray(mo_occ)
    if np.any((mo_occ != 0) & (mo_occ != 2)):
        raise NotImplementedError("avas: closed-shell references only (occupations 2 and 0)")
    P = S12 @ np.linalg.solve(S22, S12.T)
    P = 0.5 * (P + P.T)
    blocks = []
    kept = []
    for sel, active_last in ((mo_occ > 0, True), (mo_occ == 0, False)):
        Cs = C[:, sel]
        w, U = np.linalg.eigh(Cs.T @ P @ Cs)               # ascending
        act = w > threshold
        kept.append(int(act.sum()))
        inactive, active = Cs @ U[:, ~act], Cs @ U[:, act]
        blocks += [inactive, active] if active_last else [active, inactive]
    if canonicalize:
        if F is None:
            raise ValueError("avas: canonicalize needs the Fock matrix")
        for i, B in enumerate(blocks):
            if B.shape[1] > 1:
                fb = B.T @ np.asarray(F) @ B
                _, U = np.linalg.eigh(0.5 * (fb + fb.T))
                blocks[i] = B @ U
    mo = np.hstack(blocks)
    return kept[0] + kept[1], 2 * kept[0], mo, tuple(kept)


def _reference_overlaps(mol, ao_labels, minao):
    """(S12, S22) between the AOs of `mol` and the reference AOs of `minao` that `ao_labels` selects."""
    from .mole import Mole
    ref = Mole(atom=mol._atom, unit="Bohr", basis=minao, charge=mol.charge, spin=mol.spin, verbose=0).build()
    idx = ref.search_ao_label(ao_labels) if not _is_index_list(ao_labels) else np.asarray(ao_labels, dtype=int)
    if len(idx) == 0:
        raise ValueError(f"avas: no {minao} reference AO matches {ao_labels!r}")
    # one molecule with both sets on every atom: shells are grouped by atom, the calculation's first, so AO rows are mapped back
    both = Mole(atom=mol._atom, unit="Bohr", charge=mol.charge, spin=mol.spin, verbose=0)
    both.basis = {sym: _merged_shells(mol, ref, sym) for sym in {s for s, _ in mol._atom}}
    both.build()
    Sb = both.intor("int1e_ovlp")
    i1, i2 = _split_index(mol, ref, both)
    return Sb[np.ix_(i1, i2[idx])], Sb[np.ix_(i2[idx], i2[idx])]


def _is_index_list(x):
    return not isinstance(x, str) and len(x) > 0 and all(isinstance(i, (int, np.integer)) for i in x)


def _shell_list(m, sym):
    """PySCF-format basis list of element `sym` as `m` holds it (its own shell order)."""
    return [[l, *[[e, c] for e, c in zip(exps, coefs)]] for (l, exps, coefs) in m._basis_for(sym)]


def _merged_shells(mol, ref, sym):
    return _shell_list(mol, sym) + _shell_list(ref, sym)


def _split_index(mol, ref, both):
    """AO indices in `both` of the AOs of `mol` (in mol's order) and of `ref` (in ref's order).  `Mole._basis_for` sorts an
    explicit shell list by angular momentum (a stable sort), so within an atom and an l the calculation's shells precede the
    reference's."""
    loc = both.ao_loc_nr()
    i1, i2 = [], []
    for ia in range(mol.natm):
        for l in range(5):
            n1 = int(np.sum((mol._bas[:, 0] == ia) & (mol._bas[:, 1] == l)))
            sh = np.where((both._bas[:, 0] == ia) & (both._bas[:, 1] == l))[0]
            for k, s in enumerate(sh):
                (i1 if k < n1 else i2).append((ia, l, k, np.arange(loc[s], loc[s + 1])))
    # both lists are in (atom, l, shell) order; mol and ref order their shells by atom, then as their basis tables list them
    def order(m, items):
        want = [(int(a), int(l)) for a, l in zip(m._bas[:, 0], m._bas[:, 1])]
        pool = {}
        for ia, l, _k, ao in items:
            pool.setdefault((ia, l), []).append(ao)
        return np.concatenate([pool[key].pop(0) for key in want])
    return order(mol, i1), order(ref, i2)


def avas(mf, ao_labels, threshold=0.2, minao="sto-3g", with_iao=False, openshell_option=2, canonicalize=True, ncore=0, verbose=None):
    """-> (ncas, nelecas, mo_coeff) for a converged closed-shell RHF `mf`; `ao_labels`: label patterns ("C 2pz", ["C 2p", "N 2p"])
    or indices of reference AOs."""
    if with_iao or ncore:
        raise NotImplementedError("avas: with_iao and ncore are not implemented")
    require(mf, "avas")
    if int(getattr(mf.mol, "spin", 0)):
        raise NotImplementedError("avas: closed-shell RHF references only")
    if mf.mo_coeff is None:
        raise NotImplementedError("avas: the reference has no orbitals; run mf.kernel() first")
    if isinstance(ao_labels, np.ndarray):
        ao_labels = [int(i) for i in ao_labels]
    mol = mf.mol
    S12, S22 = _reference_overlaps(mol, ao_labels, minao)
    S = np.asarray(mf.get_ovlp())
    F = None
    if canonicalize:
        # the converged reference's Fock matrix from its own orbitals and energies: F = S C eps C^T S
        SC = S @ np.asarray(mf.mo_coeff)
        F = (SC * np.asarray(mf.mo_energy)[None, :]) @ SC.T
    ncas, nelecas, mo, kept = avas_algebra(np.asarray(mf.mo_coeff), np.asarray(mf.mo_occ), S, S12, S22, F, threshold, canonicalize)
    if getattr(mf, "verbose", 0) >= 4:
        print(f"AVAS: {S22.shape[0]} reference AOs, threshold {threshold}: {kept[0]} occupied + {kept[1]} virtual active orbitals")
    return ncas, nelecas, mo


kernel = avas


class AVAS:
    """Object form: `AVAS(mf, ao_labels, ...).kernel()`."""

    def __init__(self, mf, aolabels, threshold=0.2, minao="sto-3g", canonicalize=True, **kw):
        self._scf, self.aolabels, self.threshold, self.minao, self.canonicalize = mf, aolabels, threshold, minao, canonicalize
        self.ncas = self.nelecas = self.mo_coeff = None

    def kernel(self):
        self.ncas, self.nelecas, self.mo_coeff = avas(self._scf, self.aolabels, self.threshold, self.minao,
                                                       canonicalize=self.canonicalize)
        return self.ncas, self.nelecas, self.mo_coeff
