from mi355scf.tdscf import TDA, TDHF, CIS, RPA, oscillator_strengths  # noqa: F401
