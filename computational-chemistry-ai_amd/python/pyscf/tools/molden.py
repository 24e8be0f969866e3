"""`pyscf.tools.molden`: `header` and `orbital_coeff` exist so that `templates/calculate_casscf.py` imports unchanged; both raise
NotImplementedError (the template calls them only under `--save-molden`)."""


def header(mol, fout, ignore_h=False):
    raise NotImplementedError("tools.molden is not implemented")


def orbital_coeff(mol, fout, mo_coeff, spin="Alpha", symm=None, ene=None, occ=None, ignore_h=False):
    raise NotImplementedError("tools.molden is not implemented")
