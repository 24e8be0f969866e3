"""The extended-precision XC reference (tests/golden/xc_edge_reference.npz, made by tests/golden/make_xc_edge_reference.py)
checked on the CPU: its shapes, its reproducibility, its agreement with the independent FP64 restatement in oracle/dft.py
where FP64 is comfortable, and the host mirror of the ITYH factor (tests/test_rsh_host.py) against mpmath.  No GPU."""
import importlib.util
import os

import numpy as np
import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CLOSED = {"tail": 42, "zerograd": 16, "ityh": 64, "mgga": 46, "cutoff": 8}
SPIN = {"pol": 111, "cutoff_spin": 12}
NAMES = {1: "slater", 2: "b88", 3: "vwn_rpa", 4: "vwn5", 5: "lyp", 6: "pbe_x", 7: "pbe_c", 8: "tpss_x", 9: "tpss_c", 10: "m062x_x",
         11: "m062x_c"}
ITYH_LADDER = (0.3, 1.0, 1.5, 2.0, 3.0, 3.9, 3.999, 4.0, 4.001, 5.0, 10.0, 50.0, 100.0, 300.0)


@pytest.fixture(scope="module")
def fix():
    with np.load(os.path.join(GOLDEN, "xc_edge_reference.npz")) as z:
        return {k: z[k] for k in z.files}


def _generator():
    pytest.importorskip("mpmath")
    spec = importlib.util.spec_from_file_location("make_xc_edge_reference", os.path.join(GOLDEN, "make_xc_edge_reference.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_fixture_shapes(fix):
    from mi355scf import dft
    assert sorted(dft.XC_IDS.values()) == list(range(1, 13))
    for name, n in CLOSED.items():
        assert n <= 256
        for key in ("rho", "g", "tau", "omega"):
            assert fix[f"{name}_{key}"].shape == (n,) and fix[f"{name}_{key}"].dtype == np.float64
        assert fix[f"{name}_e"].shape == (12, n) and fix[f"{name}_d"].shape == (12, 3, n)
        assert fix[f"{name}_fs"].shape == (12, 4, n) and fix[f"{name}_ft"].shape == (12, 4, n)
        assert fix[f"{name}_ye"].shape == (12, n) and fix[f"{name}_yd"].shape == (12, 3, n)
        assert np.all(np.isfinite(fix[f"{name}_e"])) and np.all(np.isfinite(fix[f"{name}_d"]))
        for k in (1, 2, 3, 4, 5, 6, 7, 12):       # second derivatives for the kinds the response kernel takes
            assert np.all(np.isfinite(fix[f"{name}_fs"][k - 1])) and np.all(np.isfinite(fix[f"{name}_ft"][k - 1]))
        assert np.all(np.isnan(fix[f"{name}_ye"][11]))      # no yardstick for the short-range B88
    for name, n in SPIN.items():
        assert n <= 256
        assert fix[f"{name}_ga"].shape == (3, n) and fix[f"{name}_gb"].shape == (3, n)
        assert fix[f"{name}_e"].shape == (12, n) and fix[f"{name}_d"].shape == (12, 7, n)
        assert np.all(np.isfinite(fix[f"{name}_e"]))
        # derivatives are NaN exactly for the variables of an empty channel
        empty_b = np.maximum(fix[f"{name}_rb"], 0) == 0
        empty_a = np.maximum(fix[f"{name}_ra"], 0) == 0
        live = np.maximum(fix[f"{name}_ra"], 0) + np.maximum(fix[f"{name}_rb"], 0) > 1e-10
        d = fix[f"{name}_d"]
        assert np.all(np.isfinite(d[:, 0][:, ~empty_a])) and np.all(np.isfinite(d[:, 1][:, ~empty_b]))
        assert np.all(np.isnan(d[:, 1][:, empty_b & live])) and np.all(np.isnan(d[:, 0][:, empty_a & live]))
    # the designed edges are there
    assert np.nextafter(1e-10, 1) in fix["tail_rho"] and 0.0 in fix["zerograd_g"] and 0.0 in fix["pol_rb"]
    assert set(np.unique(fix["ityh_omega"])) == {0.2, 0.33}
    tw = fix["mgga_g"] ** 2 / (8 * fix["mgga_rho"])
    assert (fix["mgga_tau"] < tw).any() and (fix["mgga_tau"] == tw).any()
    assert os.path.getsize(os.path.join(GOLDEN, "xc_edge_reference.npz")) < 400 * 1024


def test_every_eighth_point_regenerates(fix):
    gen = _generator()

    def same(got, ref, what):
        got = float(got) if not gen.mp.isnan(got) else float("nan")
        if np.isnan(ref):
            assert np.isnan(got), what
        else:
            assert abs(got - ref) <= 1e-15 * abs(ref), (what, got, ref)
    for name, t in gen.closed_tables().items():
        for key in ("rho", "g", "tau", "omega"):
            assert np.array_equal(t[key], fix[f"{name}_{key}"]), (name, key)
        for i in range(0, len(t["rho"]), 8):
            if gen.is_zero_closed(t, i):
                assert not fix[f"{name}_e"][:, i].any() and not fix[f"{name}_d"][:, :, i].any()
                continue
            for kind in range(1, 13):
                p = gen.closed_point(kind, t["rho"][i], t["g"][i], t["tau"][i], t["omega"][i])
                same(p["e"], fix[f"{name}_e"][kind - 1, i], (name, i, kind, "e"))
                for k in range(3):
                    same(p["d"][k], fix[f"{name}_d"][kind - 1, k, i], (name, i, kind, "d", k))
                for k in range(4 if "fs" in p else 0):
                    same(p["fs"][k], fix[f"{name}_fs"][kind - 1, k, i], (name, i, kind, "fs", k))
                    same(p["ft"][k], fix[f"{name}_ft"][kind - 1, k, i], (name, i, kind, "ft", k))
    for name, t in gen.spin_tables().items():
        for key in ("ra", "rb", "ga", "gb", "ta", "tb"):
            assert np.array_equal(t[key], fix[f"{name}_{key}"]), (name, key)
        for i in range(0, len(t["ra"]), 8):
            if gen.is_zero_spin(t, i):
                assert not fix[f"{name}_e"][:, i].any()
                continue
            for kind in range(1, 13):
                p = gen.spin_point(kind, t["ra"][i], t["rb"][i], t["ga"][:, i], t["gb"][:, i], t["ta"][i], t["tb"][i], t["omega"][i])
                same(p["e"], fix[f"{name}_e"][kind - 1, i], (name, i, kind, "e"))
                for k in range(7):
                    same(p["d"][k], fix[f"{name}_d"][kind - 1, k, i], (name, i, kind, "d", k))


def test_reference_agrees_with_the_fp64_oracle_in_the_interior(fix):
    """Kinds 1-11 on the interior points of the tables (rho 1e-4 .. 10, reduced gradient at most 10, tau at least tau_W,
    both spin channels filled): the oracle's complex-step FP64 values agree with the reference to 1e-10, energy-weighted.  The
    two share no code, so a typo in either restatement shows here."""
    from oracle import dft as od
    seen = 0
    for name in CLOSED:
        rho, g, tau = fix[f"{name}_rho"], fix[f"{name}_g"], fix[f"{name}_tau"]
        with np.errstate(all="ignore"):
            ok = (rho >= 1e-4) & (rho <= 10) & (g <= 10 * np.abs(rho) ** (4.0 / 3)) & (tau >= g * g / (8 * rho))
        if not ok.any():
            continue
        rho, g, tau = rho[ok], g[ok], tau[ok]
        for kind, kname in NAMES.items():
            if kind >= 8:
                e, *d = od.eval_xc_mgga([(1.0, kname)], rho, g * g, tau)
            else:
                e, *d = od.eval_xc([(1.0, kname)], rho, g * g)
            e_ref, d_ref = fix[f"{name}_e"][kind - 1][ok], fix[f"{name}_d"][kind - 1][:, ok]
            scale = np.abs(e_ref)
            assert np.all(np.abs(e - e_ref) <= 1e-10 * scale), (name, kind, "e")
            for k, (dv, wt) in enumerate(zip(d, (rho, g * g, tau))):
                assert np.all(np.abs(dv - d_ref[k]) * wt <= 1e-10 * scale), (name, kind, k, (np.abs(dv - d_ref[k]) * wt / scale).max())
            seen += len(rho)
    ra, rb, ga, gb, ta, tb = (fix[f"pol_{k}"] for k in ("ra", "rb", "ga", "gb", "ta", "tb"))
    ok = (ra >= 1e-4) & (ra <= 10) & (rb >= 0.5 * ra)
    assert ok.sum() >= 6
    saa, sab, sbb = (ga * ga).sum(axis=0)[ok], (ga * gb).sum(axis=0)[ok], (gb * gb).sum(axis=0)[ok]
    for kind, kname in NAMES.items():
        if kind >= 8:
            e, d = od.eval_xc_mgga_spin([(1.0, kname)], ra[ok], rb[ok], saa, sab, sbb, ta[ok], tb[ok])
        else:
            e, d = od.eval_xc_spin([(1.0, kname)], ra[ok], rb[ok], saa, sab, sbb)
        e_ref, d_ref = fix["pol_e"][kind - 1][ok], fix["pol_d"][kind - 1][:, ok]
        scale = np.abs(e_ref)
        assert np.all(np.abs(e - e_ref) <= 1e-10 * scale), (kind, "e")
        for k, (dv, wt) in enumerate(zip(d, (ra[ok], rb[ok], saa, np.abs(sab), sbb, ta[ok], tb[ok]))):
            assert np.all(np.abs(dv - d_ref[k]) * wt <= 1e-10 * scale), (kind, k, (np.abs(dv - d_ref[k]) * wt / scale).max())
    assert seen >= 12 * 11


def test_ityh_host_mirror_against_mpmath():
    """F(a) and G(a) = F + a F'/2 (the factor of de/dsigma, 2e-3 .. 1e-2 of F and less) of the host mirror of the kernel's ITYH
    factor against the closed form at 60 digits, over the a-ladder: F to 1e-12, G to 2e-9, the project's vsigma bound.  A
    four-term series switched in at a = 4 misses the bound on G by truncation alone (2.1e-6 at a = 2, 3.3e-8 at a = 4)."""
    mpmath = pytest.importorskip("mpmath")
    from test_rsh_host import ityh
    mp, mpf = mpmath.mp, mpmath.mpf
    mp.dps = 60

    def closed(a):
        return 1 - mpf(8) / 3 * a * (mp.sqrt(mp.pi) * mp.erf(1 / (2 * a)) + (2 * a - 4 * a ** 3) * mp.exp(-1 / (4 * a * a)) - 3 * a + 4 * a ** 3)
    h = 1e-30
    for a in ITYH_LADDER:
        F = float(np.real(ityh(np.array(a + 0j))))
        G = F + 0.5 * a * float(np.imag(ityh(np.array(a + 1j * h)))) / h
        F_ref = closed(mpf(a))
        G_ref = F_ref + mpf(a) / 2 * mp.diff(closed, mpf(a))
        assert abs(F - F_ref) <= 1e-12 * abs(F_ref), (a, F, float(F_ref))
        assert abs(G - G_ref) <= 2e-9 * abs(G_ref), (a, G, float(G_ref), float(abs(G - G_ref) / abs(G_ref)))
