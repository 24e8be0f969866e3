"""Which reference every method accepts, cell by cell against tests/golden/reference_support.json (recorded by
tests/golden/make_reference_support.py before `mi355scf/reference.py` replaced the hand-written gates): no combination may move
between accepted and refused, no message may change, and where several traits fail the same refusal wins.  No GPU."""
import importlib.util
import json
import os

import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _load_generator():
    spec = importlib.util.spec_from_file_location("make_reference_support", os.path.join(GOLDEN, "make_reference_support.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def gen():
    return _load_generator()


@pytest.fixture(scope="module")
def recorded():
    with open(os.path.join(GOLDEN, "reference_support.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def rebuilt(gen):
    return gen.build_table()


def test_every_cell_matches_the_recorded_table(gen, recorded, rebuilt):
    rows = [f"{kind} / {flavour}" for kind in gen.KINDS for flavour in gen.FLAVOURS]
    columns = sorted(list(gen.consumers()) + [gen.OPTIMIZE])
    assert sorted(recorded) == sorted(rows) == sorted(rebuilt)
    differ = []
    for r in rows:
        assert sorted(recorded[r]) == columns == sorted(rebuilt[r]), r
        differ += [f"{r} | {c}: recorded {recorded[r][c]!r}, now {rebuilt[r][c]!r}" for c in columns if recorded[r][c] != rebuilt[r][c]]
    print(f"{len(rows)} references x {len(columns)} consumers = {len(rows) * len(columns)} cells, {len(differ)} differ")
    assert not differ, "\n".join(differ)


def test_the_grid_holds_a_refused_and_a_passed_cell_for_every_consumer_and_trait(gen, recorded):
    """A gate that stops firing, or a consumer the grid cannot get past, would otherwise hide in a column of equal cells."""
    refused = lambda cell: cell.startswith("refused: ")
    for who in gen.consumers():
        cells = [row[who] for row in recorded.values()]
        assert any(refused(c) for c in cells) and any(c == "passed" for c in cells), who
    picked = {row[gen.OPTIMIZE] for row in recorded.values()}
    assert {"internal", "cart"} <= picked and all(p in ("internal", "cart") or refused(p) for p in picked)
    for trait, has in gen.TRAITS.items():
        cells = [c for kind in gen.KINDS for flavour in gen.FLAVOURS if has(kind, flavour)
                 for who, c in recorded[f"{kind} / {flavour}"].items() if who != gen.OPTIMIZE]
        assert any(refused(c) for c in cells) and any(c == "passed" for c in cells), trait


def test_traits_and_wrap():
    """One reading of every trait, the union where the old spellings differed, nothing of it touching the GPU."""
    from mi355scf import reference
    make = _load_generator().make_reference
    t = reference.traits(make("RHF", "plain"))
    assert (t.scf, t.spin, t.xc, t.rsh, t.df, t.pcm, t.qmmm, t.nranks) == (True, "restricted", None, False, False, False, False, 1)
    with pytest.raises(AttributeError):
        t.df = True
    t = reference.traits(make("UKS b3lyp", "two ranks"))
    assert (t.spin, t.xc, t.rsh, t.nranks) == ("unrestricted", "b3lyp", False, 2)
    t = reference.traits(make("ROKS b3lyp", "mm_charge"))
    assert (t.spin, t.qmmm, t.pcm, t.df) == ("rohf", True, False, False)
    t = reference.traits(make("RKS camb3lyp", "plain"))
    assert t.rsh and not reference.traits(make("RKS tpss", "density_fit")).rsh and reference.traits(make("RKS tpss", "density_fit")).df
    assert reference.traits(make("RHF", "PCM")).pcm
    for name, value in (("_pcm", True), ("with_solvent", object())):        # either spelling alone marks a hand-made object
        mf = make("RHF", "plain")
        setattr(mf, name, value)
        assert reference.traits(mf).pcm
    assert not reference.traits(object()).scf and reference.traits(object()).spin == "restricted"
    # wrap: one class per (purpose, base), the name, the shared state
    cache = {}

    class Mixin:
        pass

    mf = make("RHF", "plain")
    a, b = reference.wrap(mf, Mixin, "X", cache, tag=1), reference.wrap(mf, Mixin, "X", cache)
    assert type(a) is type(b) and type(a).__name__ == "X" + type(mf).__name__ and isinstance(a, type(mf)) and isinstance(a, Mixin)
    assert a.mol is mf.mol and a.tag == 1 and not hasattr(b, "tag") and not hasattr(mf, "tag") and list(cache) == [type(mf)]
