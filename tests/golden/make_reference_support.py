"""Which SCF references every method built on top of one accepts, recorded as a table: tests/golden/reference_support.json.

    python tests/golden/make_reference_support.py        (writes the file; run on the commit whose behaviour is to be kept)

`build_table()` makes every reference of the grid with the package's own classes (8 kinds x 5 flavours), hands a fresh copy to every
consumer and records "refused: <message>" for a NotImplementedError and "passed" for anything else (a normal return or another
exception: the reference gate comes first in every consumer).  A reference that cannot be built itself (`solvent.PCM(UHF)`) puts
its refusal into its whole row.  The last column is the coordinate system `geomopt.optimize` picks.  Nothing here opens the GPU:
the references carry made-up orbitals, `avas` is stopped right after its reference check and `optimize` right before its first
step.  tests/test_reference_support_host.py rebuilds the table and compares every cell."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "reference_support.json")

H2O = "O 0 0 0; H 0 -0.757 0.587; H 0 0.757 0.587"
OH = "O 0 0 0; H 0 0 0.97"
SITE, CHARGE = np.array([[0.0, 0.0, 6.0]]), np.array([0.4])       # Bohr

# kind -> (module, class, xc, spin of the molecule)
KINDS = {
    "RHF": ("scf", "RHF", None, 0),
    "RKS b3lyp": ("dft", "RKS", "b3lyp", 0),
    "RKS camb3lyp": ("dft", "RKS", "camb3lyp", 0),
    "RKS tpss": ("dft", "RKS", "tpss", 0),
    "UHF": ("scf", "UHF", None, 0),
    "UKS b3lyp": ("dft", "UKS", "b3lyp", 0),
    "ROHF": ("scf", "ROHF", None, 1),
    "ROKS b3lyp": ("dft", "ROKS", "b3lyp", 1),
}
FLAVOURS = ("plain", "density_fit", "PCM", "mm_charge", "two ranks")
OPTIMIZE = "optimize coordsys"
# what a reference of the grid is: the test asserts a refused and a passed cell for every one of these
TRAITS = {
    "restricted": lambda kind, flavour: kind[0] == "R" and not kind.startswith("RO"),
    "unrestricted": lambda kind, flavour: kind[0] == "U",
    "rohf": lambda kind, flavour: kind.startswith("RO"),
    "Hartree-Fock": lambda kind, flavour: kind.endswith("HF"),
    "Kohn-Sham": lambda kind, flavour: "KS" in kind,
    "range-separated": lambda kind, flavour: "camb3lyp" in kind,
    "meta-GGA": lambda kind, flavour: "tpss" in kind,
    **{f: (lambda kind, flavour, f=f: flavour == f) for f in FLAVOURS},
}

_MOLS = {}


def _mol(spin):
    from pyscf import gto
    if spin not in _MOLS:
        m = gto.Mole()
        m.atom, m.basis, m.spin, m.verbose = (OH if spin else H2O), "sto-3g", spin, 0
        m.build()
        _MOLS[spin] = m
    return _MOLS[spin]


def make_reference(kind, flavour):
    """A fresh reference; NotImplementedError when the package refuses to build it."""
    import pyscf
    from pyscf import qmmm, solvent
    module, name, xc, spin = KINDS[kind]
    mol = _mol(spin)
    mf = getattr(getattr(pyscf, module), name)(mol)
    if xc is not None:
        mf.xc = xc
    # made-up orbitals, so that the consumers that ask for a reference that has been run get past that question
    n = mol.nao
    c, e, occ = np.eye(n), np.arange(n, dtype=float), np.zeros(n)
    na, nb = mol.nelec
    occ[:na] += 1.0
    occ[:nb] += 1.0
    if kind[0] == "U":
        c, e, occ = np.stack([c, c]), np.stack([e, e]), np.stack([(occ > 0) * 1.0, (occ > 1) * 1.0])
    mf.mo_coeff, mf.mo_energy, mf.mo_occ, mf.converged = c, e, occ, True
    if flavour == "density_fit":
        mf = mf.density_fit()
    elif flavour == "PCM":
        mf = solvent.PCM(mf)
    elif flavour == "mm_charge":
        mf = qmmm.mm_charge(mf, SITE, CHARGE, unit="Bohr")
    elif flavour == "two ranks":
        mf._rank, mf._nranks = 0, 2
    return mf


class _Stop(Exception):
    pass


def _stop(*a, **kw):
    raise _Stop


def _avas(mf):
    from mi355scf import avas
    return avas.avas(mf, ["O 2p"])


def _optimize(mf):
    """`optimize` with a gradient scanner that is never called: `build_table` notes which of its two drivers gets the molecule."""
    from mi355scf import geomopt

    class Scanner:
        base = mf

        def __call__(self, mol):
            raise _Stop

    geomopt.optimize(Scanner(), maxsteps=1)


def consumers():
    import pyscf.tdscf
    from pyscf import cc, mcscf, mp, qmmm, solvent
    from mi355scf import grad, hessian, infrared, tdscf
    return {
        "MP2": lambda mf: mp.MP2(mf),
        "TDA": lambda mf: tdscf.TDA(mf),
        "TDHF": lambda mf: tdscf.TDHF(mf),
        "CCSD": lambda mf: cc.CCSD(mf),
        "CASCI": lambda mf: mcscf.CASCI(mf, 2, 2),
        "CASSCF": lambda mf: mcscf.CASSCF(mf, 2, 2),
        "Hessian": lambda mf: hessian.Hessian(mf),
        "Infrared": lambda mf: infrared.Infrared(mf),
        "FDGradients": lambda mf: grad.FDGradients(mf),
        "pyscf.tdscf.TDA": lambda mf: pyscf.tdscf.TDA(mf),
        "nuc_grad_method": lambda mf: mf.nuc_grad_method(),
        "solvent.PCM": lambda mf: solvent.PCM(mf),
        "qmmm.mm_charge": lambda mf: qmmm.mm_charge(mf, SITE, CHARGE, unit="Bohr"),
        "density_fit": lambda mf: mf.density_fit(),
        "shard": lambda mf: mf.shard(0, 2),
        "avas": _avas,
    }


def build_table():
    """{"<kind> / <flavour>": {consumer: outcome}}."""
    from mi355scf import avas, geomopt, parallel
    cons = consumers()
    picked = []
    patches = [(avas, "_reference_overlaps", _stop),                                  # the step after avas's reference check
               (parallel, "blas_atomics_off", lambda: False),                         # shard(0, 2) would open the GPU for it
               (geomopt, "optimize_internal", lambda gs, mol, *a: picked.append("internal") or (mol, True, 0)),
               (geomopt, "optimize_cartesian", lambda gs, mol, *a: picked.append("cart") or (mol, True, 0))]
    saved = [(mod, name, getattr(mod, name)) for mod, name, _new in patches]
    for mod, name, new in patches:
        setattr(mod, name, new)
    table = {}
    try:
        for kind in KINDS:
            for flavour in FLAVOURS:
                row = table[f"{kind} / {flavour}"] = {}
                for who, call in cons.items():
                    try:
                        call(make_reference(kind, flavour))
                        row[who] = "passed"
                    except NotImplementedError as err:
                        row[who] = f"refused: {err}"
                    except Exception:
                        row[who] = "passed"
                try:
                    del picked[:]
                    _optimize(make_reference(kind, flavour))
                    row[OPTIMIZE] = ",".join(picked)
                except NotImplementedError as err:
                    row[OPTIMIZE] = f"refused: {err}"
    finally:
        for mod, name, old in saved:
            setattr(mod, name, old)
    return table


if __name__ == "__main__":
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(HERE)), "computational-chemistry-ai_amd", "python"))
    with open(OUT, "w") as f:
        json.dump(build_table(), f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"wrote {OUT}: {os.path.getsize(OUT)} bytes")
