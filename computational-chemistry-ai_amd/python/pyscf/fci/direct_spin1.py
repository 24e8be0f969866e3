"""`pyscf.fci.direct_spin1`: `FCISolver` / `FCI()` and the module-level helpers that need no solver state."""
from mi355scf.fci import FCISolver, absorb_h1e  # noqa: F401


def FCI(mol=None, **kw):
    return FCISolver(mol)
