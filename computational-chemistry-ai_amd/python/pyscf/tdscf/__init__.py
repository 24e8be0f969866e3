"""`pyscf.tdscf` (templates/calculate_uv_spectrum.py:92-158): closed-shell TDA / TDHF / TDDFT on the MI355X engine.
Imported on its own (`from pyscf import tdscf`), not by `import pyscf`."""
from mi355scf.reference import require
from . import rhf, rks  # noqa: F401


def _check(mf):
    require(mf, "tdscf")
    return mf


def TDA(mf):
    return rhf.TDA(_check(mf))


def TDHF(mf):
    return rhf.TDHF(_check(mf))


def TDDFT(mf):
    """TDHF for an RHF reference, TDDFT for an RKS one (the same full-response solver)."""
    return rhf.TDHF(_check(mf))


RPA = TDDFT
CIS = TDA
