"""`gpu4pyscf.cc`: the same `CCSD` as `pyscf.cc`."""
from mi355scf import ccsd  # noqa: F401
from mi355scf.ccsd import CCSD, RCCSD  # noqa: F401
