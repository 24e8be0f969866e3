from mi355scf.tdscf import TDA, TDDFT  # noqa: F401
