"""`gpu4pyscf.mcscf`: the same `CASCI`, `CASSCF` and `avas` as `pyscf.mcscf`."""
from mi355scf import casci  # noqa: F401
from mi355scf.casci import CASCI, CASSCF  # noqa: F401
from pyscf.mcscf import avas  # noqa: F401,E402
