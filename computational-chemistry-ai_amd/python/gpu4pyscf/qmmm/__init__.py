"""`gpu4pyscf.qmmm`: the same embedding as `pyscf.qmmm` (mi355scf/qmmm.py)."""
from mi355scf.qmmm import mm_charge, mm_charge_grad  # noqa: F401
