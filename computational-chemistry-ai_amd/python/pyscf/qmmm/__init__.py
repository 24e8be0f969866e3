"""`pyscf.qmmm`: `mm_charge(mf, coords, charges)` / `mm_charge_grad` -- point-charge embedding on the MI355X engine
(mi355scf/qmmm.py)."""
from mi355scf.qmmm import mm_charge, mm_charge_grad  # noqa: F401
