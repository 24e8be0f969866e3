"""`pyscf.tdscf` (templates/calculate_uv_spectrum.py:92-158): closed-shell TDA / TDHF / TDDFT on the MI355X engine.
Imported on its own (`from pyscf import tdscf`), not by `import pyscf`."""
from . import rhf, rks  # noqa: F401


def _check(mf):
    if not getattr(mf, "_spin_restricted", True):
        raise NotImplementedError("tdscf: UHF/UKS references are not supported (closed-shell RHF/RKS only)")
    if getattr(mf, "_pcm", False):
        raise NotImplementedError("tdscf: excited states with PCM solvation are not implemented")
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
