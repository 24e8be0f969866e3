"""`pyscf.solvent` (templates/calculate_solvent_effect.py:15,114): `solvent.PCM(mf)` -- C-PCM for RHF / RKS on the MI355X
engine (mi355scf/pcm.py)."""
from mi355scf.pcm import PCM  # noqa: F401
from mi355scf import pcm  # noqa: F401
