"""`pyscf.mcscf` (`templates/calculate_casscf.py:15,126`): `CASCI` on the MI355X engine (`mi355scf.casci`).  `CASSCF` exists but
raises NotImplementedError: orbital optimisation, state averaging and `mcscf.avas` are not implemented.
Imported on its own (`from pyscf import mcscf`), not by `import pyscf`."""
from mi355scf import casci  # noqa: F401
from mi355scf.casci import CASCI, CASSCF  # noqa: F401
