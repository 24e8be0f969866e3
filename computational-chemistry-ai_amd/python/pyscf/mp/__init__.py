"""`pyscf.mp`: `MP2` (`templates/calculate_interaction.py:19,118`).  Conventional MP2 streamed from the engine's resident ERI tiles
(`mi355scf.mp2`); `mp.mp2.MP2` resolves as in PySCF."""
from mi355scf import mp2  # noqa: F401
from mi355scf.mp2 import MP2, RMP2, UMP2  # noqa: F401
