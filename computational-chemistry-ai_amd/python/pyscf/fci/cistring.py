"""`pyscf.fci.cistring`: strings as occupation bit masks in ascending integer order."""
from mi355scf.fci import num_strings, make_strings, addr2str, str2addr, link_table  # noqa: F401

gen_strings4orblist = make_strings
