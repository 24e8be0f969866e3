"""`pyscf.tools` (`templates/calculate_casscf.py:15,216-221`): only the `molden` names the template touches exist, and they
raise NotImplementedError -- writing Molden files is not implemented."""
from . import molden  # noqa: F401
