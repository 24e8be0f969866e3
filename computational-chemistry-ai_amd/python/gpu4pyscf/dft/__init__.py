from . import rks, uks, roks  # noqa: F401
RKS = rks.RKS
UKS = uks.UKS
ROKS = roks.ROKS
