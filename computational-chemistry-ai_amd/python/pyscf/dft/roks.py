"""`pyscf.dft.roks`: `ROKS`, restricted open-shell Kohn-Sham (`mi355scf.rohf`)."""
from mi355scf.rohf import ROKS  # noqa: F401
