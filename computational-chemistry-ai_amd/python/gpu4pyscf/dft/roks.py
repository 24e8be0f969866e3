"""`gpu4pyscf.dft.roks`: the same `ROKS` as `pyscf.dft.roks`."""
from mi355scf.rohf import ROKS  # noqa: F401
