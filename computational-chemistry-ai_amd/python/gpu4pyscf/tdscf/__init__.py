"""`gpu4pyscf.tdscf`: the same closed-shell response classes as `pyscf.tdscf`."""
from pyscf.tdscf import TDA, TDHF, TDDFT, RPA, CIS, rhf, rks  # noqa: F401
