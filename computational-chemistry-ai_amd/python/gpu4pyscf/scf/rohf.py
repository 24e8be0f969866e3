"""`gpu4pyscf.scf.rohf`: the same `ROHF` as `pyscf.scf.rohf`."""
from mi355scf.rohf import ROHF  # noqa: F401
