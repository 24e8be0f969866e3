from . import hf, uhf, rohf  # noqa: F401
RHF = hf.RHF
UHF = uhf.UHF
ROHF = rohf.ROHF
