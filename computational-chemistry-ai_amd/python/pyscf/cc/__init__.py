"""`pyscf.cc` (the reference README's "adding a new method": `cc.CCSD(mf).kernel()`, `.ccsd_t()`): closed-shell CCSD and CCSD(T)
on the MI355X engine (`mi355scf.ccsd`).  `RCCSD` is the same class; UCCSD, density-fitted CCSD, gradients and lambda equations
are not implemented."""
from mi355scf import ccsd  # noqa: F401
from mi355scf.ccsd import CCSD, RCCSD  # noqa: F401
