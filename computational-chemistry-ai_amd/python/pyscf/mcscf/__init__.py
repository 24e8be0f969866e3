"""`pyscf.mcscf` (`templates/calculate_casscf.py:15-16,86,98-111,126`): `CASCI` and `CASSCF` (orbital optimisation, state
averaging) on the MI355X engine (`mi355scf.casci`, `mi355scf.casscf`) and the `avas` active-space selection (`mi355scf.avas`,
STO-3G reference AOs instead of MINAO).  Closed-shell RHF references for CASSCF; nuclear gradients (`mc.nuc_grad_method()`,
`mi355scf.casscf_grad`) for the state-specific CASSCF wavefunction; ROHF-based CASSCF, state-averaged and CASCI gradients are not
implemented.  Imported on its own (`from pyscf import mcscf`), not by `import pyscf`."""
from mi355scf import casci  # noqa: F401
from mi355scf.casci import CASCI, CASSCF  # noqa: F401
from . import avas  # noqa: F401,E402
