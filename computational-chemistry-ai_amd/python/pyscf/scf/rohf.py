"""`pyscf.scf.rohf`: `ROHF` (reference call sites `templates/calculate_casscf.py:61-64`; named in the isinstance check at
`templates/calculate_reaction_energy.py:167`)."""
from mi355scf.rohf import ROHF  # noqa: F401
