"""`pyscf.mcscf.avas` (`templates/calculate_casscf.py:16,86`): `avas.avas(mf, ao_labels, threshold=0.2, ...)` from
`mi355scf.avas`."""
from mi355scf.avas import avas, kernel, AVAS  # noqa: F401
