"""What an SCF object handed to a method IS (`traits`), which of those every method accepts (`SUPPORT`, `require`), and the
run-time subclass idiom of the wrappers (`wrap`).  Imports no method module, so every one of them can import this.

A method refuses a reference instead of silently dropping a term (K_LR, V_pcm, the embedding potential): `require(mf, who)` asks
its row, which lists, in the order they are asked, the traits the method does not take and the words of each refusal.  A new method
adds a row, a new flavour of reference a field of `Traits` and a condition of `_IS`; tests/golden/make_reference_support.py then
lists every (reference, method) cell that has to be decided.  Not here: what is known only after the set-up
(direct mode: `ao2mo.resident_engine`, `dft.check_rsh_scf`), what concerns the method's own object (active space, memory, triplets)
and the per-cycle reads of `with_df`, `with_solvent`, `_nranks` that choose a path of the Fock build."""
from collections import namedtuple


class Traits(namedtuple("Traits", "scf spin xc df pcm qmmm nranks cls")):
    """scf: an SCF object of this engine at all; spin: "restricted" | "unrestricted" | "rohf"; xc: the functional, None = HF;
    df, pcm, qmmm: density-fitted, PCM-solvated, embedded in point charges; nranks: ranks of the sharded store; cls: class name."""
    __slots__ = ()

    @property
    def rsh(self):
        """A range-separated hybrid (needs K_LR)."""
        from .dft import is_rsh
        return is_rsh(self.xc)


def traits(mf):
    """The `Traits` of `mf`, read from its attributes without touching the GPU (`engine`, a property that opens it, is asked of
    the type).  PCM is either spelling: the `_pcm` of the wrapper class or a `with_solvent`."""
    t = type(mf)
    return Traits(scf=all(hasattr(t, a) for a in ("_jk", "_setup", "_setup_once", "engine", "energy_nuc")) and hasattr(mf, "mo_coeff"),
                  spin="rohf" if getattr(mf, "_rohf", False) else "restricted" if getattr(mf, "_spin_restricted", True) else "unrestricted",
                  xc=getattr(mf, "xc", None), df=getattr(mf, "with_df", None) is not None,
                  pcm=bool(getattr(mf, "_pcm", False)) or getattr(mf, "with_solvent", None) is not None,
                  qmmm=bool(getattr(mf, "_qmmm", False)), nranks=int(getattr(mf, "_nranks", 1)), cls=t.__name__)


_IS = {"rohf": lambda t: t.spin == "rohf", "unrestricted": lambda t: t.spin == "unrestricted", "open-shell": lambda t: t.spin != "restricted",
       "Kohn-Sham": lambda t: t.xc is not None, "rsh": lambda t: t.rsh, "df": lambda t: t.df, "pcm": lambda t: t.pcm,
       "qmmm": lambda t: t.qmmm, "sharded": lambda t: t.nranks > 1, "foreign": lambda t: not t.scf}
# the wording most rows share; {who} is the row's name, {xc} and {cls} come from the reference
_ROHF = "{who}: restricted open-shell (ROHF / ROKS) references are not supported"
_DF = "{who}: density-fitted references are not supported"
_QMMM = ("{who}: point-charge-embedded references (qmmm.mm_charge) are not supported: the method was not verified with an "
         "embedded core Hamiltonian")
_NO_KLR = "{who}: not implemented for the range-separated hybrid {xc} (no long-range exchange integrals on this path)"
_ONE_RANK = "qmmm.mm_charge runs on one rank"
_ROHF_SCF = "{who}: density fitting and PCM solvation are not implemented"


def _rhf_only(*first, unrestricted="{who}: UHF / UKS references are not supported (closed-shell RHF only)"):
    """The row of a method on the resident, unsharded store of one closed-shell RHF (`first`: what it asks before that)."""
    return first + (("unrestricted", unrestricted),
                    ("Kohn-Sham", "{who}: Kohn-Sham references (xc = {xc!r}) are not supported (closed-shell RHF only)"),
                    ("df", _DF), ("pcm", "{who}: PCM-solvated references are not supported"), ("qmmm", _QMMM),
                    ("sharded", "{who}: sharded references are not supported (one GPU, unsharded ERI store)"),
                    ("foreign", "{who}: {cls} is not an RHF object of this engine"))


SUPPORT = {
    "MP2": (("rohf", _ROHF + " (RHF -> RMP2, UHF -> UMP2)"),),
    "TDA/TDDFT": (("qmmm", _QMMM), ("open-shell", "{who}: only closed-shell RHF/RKS references are supported (UHF/UKS are not)"), ("df", _DF)),
    "tdscf": (("open-shell", "{who}: UHF/UKS references are not supported (closed-shell RHF/RKS only)"),        # pyscf.tdscf's entry points
              ("pcm", "{who}: excited states with PCM solvation are not implemented")),
    "TDA/TDDFT gradients": (("rsh", "{who}: not implemented for the range-separated hybrid {xc} (no long-range derivative integrals)"),
                            ("pcm", "{who}: PCM-wrapped references are not implemented")),
    "CASCI": _rhf_only(),                                                   # an ROHF (one orbital set, occupations 2 / 1 / 0) passes
    "CASSCF": _rhf_only(("rohf", _ROHF + " yet: ROHF-based CASSCF is not implemented (mcscf.CASCI takes an ROHF reference)")),
    "CCSD": _rhf_only(("rohf", _ROHF), unrestricted="{who}: UCCSD is not implemented (UHF / UKS references; closed-shell RHF only)"),
    "avas": (("open-shell", "{who}: closed-shell RHF references only"),),
    "Hessian": (("rsh", _NO_KLR), ("qmmm", _QMMM)),
    "infrared spectrum": (("rsh", _NO_KLR), ("qmmm", _QMMM)),
    "nuclear gradients": (("rsh", _NO_KLR),),
    "PCM": (("qmmm", "solvent.PCM on a point-charge-embedded SCF (qmmm.mm_charge) is not supported"),
            ("open-shell", "PCM with UHF / UKS is not implemented (closed-shell RHF / RKS only)"), ("sharded", "PCM runs on one rank"),
            ("rsh", _NO_KLR)),
    "qmmm.mm_charge": (("foreign", "{who}: {cls} is not an SCF object of this engine"), ("pcm", "{who} on a PCM-solvated SCF is not supported"),
                       ("df", "{who}: density-fitted SCF objects are not supported"), ("sharded", _ONE_RANK)),
    "embedded SCF": (("sharded", _ONE_RANK), ("df", "qmmm.mm_charge: density-fitted SCF objects are not supported"),   # switched on after `mm_charge`
                     ("pcm", "qmmm.mm_charge: PCM solvation on top of the embedding is not supported")),
    "density_fit()": (("qmmm", "qmmm.mm_charge: density fitting of an embedded SCF is not supported"),
                      ("rohf", "ROHF / ROKS: density fitting is not implemented"), ("rsh", _NO_KLR)),
    "shard()": (("qmmm", _ONE_RANK), ("pcm", "PCM runs on one rank"),       # asked when more than one rank is requested
                ("rohf", "ROHF / ROKS: sharded runs are not implemented")),
    "ROHF / ROKS": (("rsh", "ROKS: the range-separated hybrid {xc} is not implemented (RKS / UKS only)"), ("df", _ROHF_SCF), ("pcm", _ROHF_SCF)),
    "RSH SCF": (("df", "{xc}: density fitting is not implemented for range-separated hybrids"),
                ("pcm", "{xc}: PCM solvation is not implemented for range-separated hybrids"),
                ("sharded", "{xc}: sharded runs are not implemented for range-separated hybrids")),
}


def require(mf, who):
    """NotImplementedError with the words of row `who` for the first trait of `mf` the row does not take; else `traits(mf)`."""
    t = traits(mf)
    for trait, message in SUPPORT[who]:
        if _IS[trait](t):
            raise NotImplementedError(message.format(who=who, xc=t.xc, cls=t.cls))
    return t


def wrap(obj, mixin, prefix, cache, **attrs):
    """`obj` as an instance of the class `prefix + its class's name` with bases (mixin, its class), made once per class and kept in
    `cache`; the new object shares obj's state (a copy of its `__dict__`) and gets `attrs` on top."""
    base = obj.__class__
    cls = cache.get(base) or cache.setdefault(base, type(prefix + base.__name__, (mixin, base), {}))
    new = cls.__new__(cls)
    new.__dict__.update(obj.__dict__, **attrs)
    return new
