"""`pyscf.fci` (`templates/calculate_casscf.py:15`): the determinant FCI solver of the MI355X engine (`mi355scf.fci`).
`fci.FCI(mf_or_mol)`, `fci.direct_spin1.FCI()` / `FCISolver`, `fci.cistring`.  Imported on its own (`from pyscf import fci`)."""
from . import cistring, direct_spin1  # noqa: F401
from mi355scf.fci import FCI, FCISolver  # noqa: F401
