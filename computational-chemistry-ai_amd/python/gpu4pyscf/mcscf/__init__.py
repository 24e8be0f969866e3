"""`gpu4pyscf.mcscf`: the same `CASCI` as `pyscf.mcscf`."""
from mi355scf import casci  # noqa: F401
from mi355scf.casci import CASCI, CASSCF  # noqa: F401
