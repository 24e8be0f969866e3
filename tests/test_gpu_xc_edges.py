"""The exchange-correlation functional kernels (xc_eval_kernel, xc_eval_spin_kernel, xc_eval_mgga_kernel, xc_fxc_prep_kernel)
against the 60-digit reference of tests/golden/xc_edge_reference.npz (made by tests/golden/make_xc_edge_reference.py with
mpmath; this module reads the fixture only) at the edges of their argument space: density tails with reduced gradients up to
1e4, zero and tiny gradients, spin polarisation down to an empty channel, the ITYH factor across its closed-form/series
switch, tau at and below tau_W, and the density cut-off.  Every term kind runs alone with coefficient 1, then the composites.

Scale and bounds.  scale = max(|e_kind|, 0.7386 rho^(4/3)) (the local LDA exchange energy density; a correlation term's own
|e| cancels to nothing in the tail).  e to 1e-11 scale; first derivatives |dv| rho, |dv| sigma, |dv| tau to 1e-9 scale; the
short-range B88 (kind 12) to 2e-9 of each of e, vrho and vsigma themselves at every a; second derivatives to
1e-6 (|f_ref| + 1e-3 |v_ref| / den) with den = rho (f_rr, f_rs) and sigma (f_ss), sigma not below the kernel's floor of 1e-40.
No masks.  The reference is the bare formula; what the kernels add is checked as a convention:
  * every output is exactly 0.0 at rho <= 1e-10 (rho_a + rho_b for the spin kernels), negative densities count as zero;
  * every output at every other point is finite;
  * where the minority channel is emptier than MINORITY_REL of the density (the zeta clip of TPSS correlation at 1 - 1e-15
    bites below 5e-16) or holds no more than CHANNEL_FLOOR (the kernels' XC_CHANNEL_FLOOR), the energy and the majority
    channel's derivatives are still compared with the bare formula, while the minority channel's own outputs only have to be
    finite: the clipped or dropped channel has no meaningful derivative and nothing multiplies it.  Everywhere else, down to
    rho_b / rho_a = 1e-13 and rho_b = 1e-14, the minority channel is compared like the majority one.

Regimes whose bound comes from the FP64 yardstick (the fixture stores, per point, what oracle/dft.py reaches in FP64 against
the same reference; a bound set this way is 16 x the largest yardstick error of the regime, never the kernel's own error):

    YARDSTICK_REGIMES below; empty means every regime meets the plain bounds.

Measured on the MI355X when the tests were written: worst kernel error / worst yardstick error of the table, both as
fractions of the bound, over every entry point and quantity of the kind (first and second derivatives included; the yardstick
of the spin tables includes minority-channel derivatives, where the oracle's own guards dominate it):

    kind  tail             zerograd         ityh             mgga             cutoff           pol              cutoff_spin
    1     1.8e-4 / 2.0e-4  1.4e-4 / 1.6e-4  1.7e-4 / 1.9e-4  1.7e-4 / 2.0e-4  1.8e-4 / 1.8e-4  1.7e-4 / 2.1e-4  1.8e-4 / 3.1e-4
    2     1.7e-4 / 4.0e-3  1.4e-4 / 1.6e-4  1.7e-4 / 3.9e-4  1.7e-4 / 2.0e-4  1.8e-4 / 3.4e-3  1.7e-4 / 6.7e+6  1.9e-4 / 3.8e+8
    3     5.5e-4 / 6.0e-4  5.8e-5 / 7.7e-5  4.6e-4 / 2.0e-4  2.4e-4 / 2.2e-4  2.1e-4 / 2.0e-4  1.8e-4 / 3.1e-4  3.2e-4 / 1.7e-4
    4     8.1e-4 / 6.8e-4  1.9e-4 / 6.1e-5  6.4e-4 / 4.5e-4  7.0e-4 / 6.8e-4  8.1e-4 / 2.6e-4  4.7e-4 / 5.1e-4  8.1e-4 / 1.5e-4
    5     1.4e-5 / 1.1e-5  7.6e-6 / 7.6e-6  1.3e-5 / 1.3e-5  1.2e-5 / 9.0e-6  1.4e-5 / 9.2e-6  4.4e-6 / 1.5e-5  1.4e-5 / 1.0e-5
    6     1.9e-4 / 5.5e-4  1.4e-4 / 1.4e-4  1.7e-4 / 1.5e-4  1.7e-4 / 1.7e-4  1.8e-4 / 2.5e-4  1.7e-4 / 3.0e+3  1.7e-4 / 7.1e-4
    7     6.5e-4 / 3.9e-1  1.7e-4 / 2.2e-2  8.0e-4 / 3.3e-1  3.6e-5 / 2.6e-1  4.0e-4 / 4.6e-2  2.4e-4 / 5.6e-2  7.3e-4 / 4.9e-1
    8     1.6e-2 / 2.3e-2  4.2e-3 / 2.6e-4  1.2e-2 / 1.9e-3  5.0e-3 / 1.1e-4  4.4e-4 / 3.5e-3  1.5e-4 / 9.1e+3  1.8e-4 / 2.2e-2
    9     1.1e-3 / 6.2e-1  1.7e-4 / 2.6e-2  8.1e-4 / 3.3e-1  1.3e-4 / 2.6e-1  3.9e-4 / 4.6e-2  2.5e-4 / 6.8e+1  7.5e-4 / 4.9e-1
    10    4.5e-4 / 1.4e-3  7.1e-5 / 1.3e-4  1.6e-4 / 2.2e-4  6.8e-4 / 8.4e-4  8.3e-5 / 3.6e-4  1.0e-4 / 2.0e+3  1.6e-4 / 1.0e-3
    11    5.0e-4 / 2.5e+0  9.1e-5 / 3.3e-2  3.9e-4 / 4.5e-1  1.9e-4 / 6.6e-2  2.4e-4 / 1.3e+0  1.1e-3 / 1.4e+6  2.7e-4 / 1.2e+1
    12    1.7e-6 / -       1.1e-5 / -       1.9e-3 / -       1.9e-6 / -       1.3e-5 / -       5.1e-6 / -       7.6e-7 / -
"""
import os

import numpy as np
import pytest

from conftest import MOLECULES

pytestmark = pytest.mark.gpu

W = 0.7
U = np.array([0.6, 0.0, 0.8])           # direction of the closed-shell tables' gradients
CLOSED = ("tail", "zerograd", "ityh", "mgga", "cutoff")
SPIN = ("pol", "cutoff_spin")
GGA_KINDS = (1, 2, 3, 4, 5, 6, 7, 12)
MGGA_KINDS = (8, 9, 10, 11)
LDA_X = 0.7385587663820224
MINORITY_REL = 5e-16
CHANNEL_FLOOR = 1e-24
# (entry point, kind, table, quantity) -> (largest yardstick error / scale in the regime, bound = 16 x that)
YARDSTICK_REGIMES = {}
COMPOSITES = {"B3LYP": [(0.08, 1), (0.72, 2), (0.19, 3), (0.81, 5)], "PBE0": [(0.75, 6), (1.0, 7)],
              "CAM-B3LYP": [(0.35, 2), (0.46, 12), (0.19, 4), (0.81, 5)], "TPSS": [(1.0, 8), (1.0, 9)],
              "M06-2X": [(1.0, 10), (1.0, 11)]}
_CACHE = {}


def _fix():
    if "fix" not in _CACHE:
        path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "xc_edge_reference.npz")
        with np.load(path) as z:
            _CACHE["fix"] = {k: z[k] for k in z.files}
    return _CACHE["fix"]


def _engine():
    if "eng" not in _CACHE:
        from pyscf import gto
        from mi355scf import engine
        _CACHE["eng"] = engine.Engine(gto.M(atom=MOLECULES["h2o"], basis="sto-3g", verbose=0))
    return _CACHE["eng"]


def _dev(eng, a):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64), device=eng.device).contiguous()


def _np(t):
    return t.cpu().numpy()


class Report:
    """Collects every figure of a test (printed, for the measurement scripts) and fails at the end with all misses."""

    def __init__(self, what):
        self.what, self.bad = what, []

    def check(self, label, err, bound, yard=None):
        err, bound = np.asarray(err, dtype=np.float64), np.asarray(bound, dtype=np.float64)
        if err.size == 0:
            return
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = np.where(err == 0, 0.0, err / bound)
        ratio = np.where(np.isfinite(err), ratio, np.inf)
        i = int(np.argmax(ratio))
        line = f"{self.what} {label}: worst error/bound {ratio.flat[i]:.3g} at point {i}"
        if yard is not None:
            with np.errstate(divide="ignore", invalid="ignore"):
                yr = np.where(yard == 0, 0.0, np.asarray(yard) / bound)
            worst = np.nanmax(yr) if np.isfinite(yr).any() else np.nan
            line += f"; yardstick/bound there {yr.flat[i]:.3g}, worst {worst:.3g}"
        print(line)
        if not ratio.flat[i] <= 1.0:
            self.bad.append(line)

    def exact_zero(self, label, arrays, where):
        for k, a in enumerate(arrays):
            if not np.all(a[..., where] == 0.0):
                self.bad.append(f"{self.what} {label}: output {k} is not exactly 0.0 at the cut-off points")

    def finite(self, label, arrays):
        for k, a in enumerate(arrays):
            if not np.all(np.isfinite(a)):
                self.bad.append(f"{self.what} {label}: output {k} is not finite at points {np.nonzero(~np.isfinite(a))[-1][:8]}")

    def done(self):
        assert not self.bad, "\n".join(self.bad)


def _bound(key, default):
    return YARDSTICK_REGIMES[key][1] if key in YARDSTICK_REGIMES else default


def _closed_table(name):
    f = _fix()
    rho, g, tau, om = (f[f"{name}_{k}"] for k in ("rho", "g", "tau", "omega"))
    R = np.vstack([rho, g * U[0], g * U[1], g * U[2]])
    grad = R[1:]
    sigma = (grad * grad).sum(axis=0)
    return {"rho": rho, "R": R, "grad": grad, "sigma": sigma, "tau": tau, "omega": om, "zero": rho <= 1e-10,
            "lda": LDA_X * np.maximum(rho, 0.0) ** (4.0 / 3), "e": f[f"{name}_e"], "d": f[f"{name}_d"], "fs": f[f"{name}_fs"],
            "ft": f[f"{name}_ft"], "ye": f[f"{name}_ye"], "yd": f[f"{name}_yd"]}


def _spin_table(name):
    f = _fix()
    ra, rb, ga, gb, ta, tb, om = (f[f"{name}_{k}"] for k in ("ra", "rb", "ga", "gb", "ta", "tb", "omega"))
    pa, pb = np.maximum(ra, 0.0), np.maximum(rb, 0.0)
    rho = pa + pb
    lo = np.minimum(pa, pb)
    return {"ra": ra, "rb": rb, "pa": pa, "pb": pb, "Ra": np.vstack([ra, ga]), "Rb": np.vstack([rb, gb]), "ga": ga, "gb": gb, "ta": ta,
            "tb": tb, "omega": om, "rho": rho, "zero": rho <= 1e-10, "lda": LDA_X * rho ** (4.0 / 3),
            "exempt_a": (pa < pb) & ((lo < MINORITY_REL * rho) | (lo <= CHANNEL_FLOOR)),
            "exempt_b": (pb <= pa) & ((lo < MINORITY_REL * rho) | (lo <= CHANNEL_FLOOR)),
            "e": f[f"{name}_e"], "d": f[f"{name}_d"], "ye": f[f"{name}_ye"], "yd": f[f"{name}_yd"]}


def _combine(terms, arr):
    """sum_t coef_t arr[kind_t - 1]"""
    return sum(c * arr[k - 1] for c, k in terms)


def _omega_groups(t, terms):
    """Point subsets that share the runtime parameter: one launch per omega where a short-range B88 term is present."""
    if not any(k == 12 for _c, k in terms):
        return [(np.arange(len(t["omega"])), None)]
    return [(np.nonzero(t["omega"] == om)[0], [float(om) if k == 12 else 0.0 for _c, k in terms]) for om in np.unique(t["omega"])]


def _mul0(a, b):
    """a * b with 0 wherever b is 0 (a reference derivative of an empty channel is NaN and multiplies a zero gradient)."""
    return np.where(b == 0, 0.0, np.where(b == 0, 0.0, a) * b)


def _check_closed(rep, entry, name, t, terms, e, vr, vs, vt=None, kind=None):
    """e and the raw derivatives of a closed-shell evaluation against the reference of `terms`."""
    live = ~t["zero"]
    e_ref, d_ref = _combine(terms, t["e"]), _combine(terms, t["d"])
    scale = np.maximum(np.abs(e_ref), t["lda"])
    single = kind is not None and kind != 12
    ye = t["ye"][kind - 1] if single else None
    yd = t["yd"][kind - 1] if single else None
    outs = [e, vr, vs] + ([vt] if vt is not None else [])
    rep.exact_zero(f"{entry} {name}", outs, t["zero"])
    rep.finite(f"{entry} {name}", outs)
    if kind == 12:     # relative to each quantity itself, at every a
        for what, got, ref in (("e", e, e_ref), ("vrho", vr, d_ref[0]), ("vsigma", vs, d_ref[1])):
            rep.check(f"{entry} {name} {what} (relative)", np.abs(got - ref)[live], (2e-9 * np.abs(ref))[live])
        return
    for what, got, ref, wt, tol, y in (("e", e, e_ref, 1.0, 1e-11, ye), ("vrho", vr, d_ref[0], t["rho"], 1e-9, None if yd is None else yd[0]),
                                       ("vsigma", vs, d_ref[1], t["sigma"], 1e-9, None if yd is None else yd[1]),
                                       ("vtau", vt, d_ref[2], t["tau"], 1e-9, None if yd is None else yd[2])):
        if got is None:
            continue
        b = _bound((entry, kind, name, what), tol) * scale
        rep.check(f"{entry} {name} {what}", (np.abs(got - ref) * wt)[live], b[live], None if y is None else (y * wt)[live])


def _raw_from_wv(t, wv):
    """vrho, vsigma (and vtau) back out of wv = (w/2 vrho, 2 w vsigma grad rho, w/4 vtau); vsigma from the largest gradient
    component, and the rows must be parallel to the gradient."""
    vr = wv[0] / (0.5 * W)
    gz = t["grad"][2]
    with np.errstate(divide="ignore", invalid="ignore"):
        vs = np.where(gz != 0, wv[3] / (2 * W * np.where(gz != 0, gz, 1.0)), 0.0)
    vt = wv[4] / (0.25 * W) if wv.shape[0] == 5 else None
    return vr, vs, vt


def _check_wv_rows(rep, label, t, wv, vs):
    """wv[1..3] = 2 w vsigma grad rho to rounding (the closed-shell kernels form exactly this product), exactly 0 where the
    gradient is 0."""
    ref = 2 * W * vs[None, :] * t["grad"]
    rep.check(f"{label} wv rows against 2 w vsigma grad rho", np.abs(wv[1:4] - ref), 1e-15 * np.abs(ref) + 1e-300 * (t["grad"] != 0))


def _check_spin_rows(rep, entry, name, t, wv, terms, kind):
    """Rows 1..3 of a spin kernel at rho_a = rho_b against 2 w vsigma grad rho of the reference, as |dv| sigma: the kernel
    adds 2 de/dsigma_ss grad rho_s and de/dsigma_ab grad rho_s', which are not parallel to rounding."""
    d_ref, e_ref = _combine(terms, t["d"]), _combine(terms, t["e"])
    ref = 2 * W * d_ref[1][None, :] * t["grad"]
    err = (np.abs(wv[1:4] - ref) * np.abs(t["grad"])).sum(axis=0) / (2 * W)
    live = ~t["zero"]
    if kind == 12:
        tol = 2e-9 * np.abs(d_ref[1]) * t["sigma"]
    else:
        tol = _bound((entry, kind, name, "vsigma"), 1e-9) * np.maximum(np.abs(e_ref), t["lda"])
    rep.check(f"{entry} {name} gradient rows (|dv| sigma)", err[live], tol[live])


# ---------------------------------------------------------------------------------------------
# closed shell
# ---------------------------------------------------------------------------------------------
def _run_closed_gga(rep, label, terms, kind=None):
    eng = _engine()
    for name in CLOSED:
        t = _closed_table(name)
        n = len(t["rho"])
        e, vr, vs, wv = np.empty(n), np.empty(n), np.empty(n), np.empty((4, n))
        for idx, prm in _omega_groups(t, terms):
            out = eng.xc_eval(terms, _dev(eng, t["R"][:, idx]), _dev(eng, np.full(len(idx), W)), True, want_raw=True, params=prm)
            e[idx], wv[:, idx], vr[idx], vs[idx] = (_np(x) for x in out)
        _check_closed(rep, "xc_eval", name, t, terms, e, vr, vs, kind=kind)
        rep.exact_zero(f"xc_eval {name} wv", [wv], t["zero"])
        rep.finite(f"xc_eval {name} wv", [wv])
        rep.check(f"xc_eval {name} wv[0] against w/2 vrho", np.abs(wv[0] - 0.5 * W * vr), 4e-16 * np.abs(vr))
        _check_wv_rows(rep, f"xc_eval {name}", t, wv, vs)


@pytest.mark.parametrize("kind", GGA_KINDS)
def test_closed_shell_kernel_at_the_edges(kind):
    rep = Report(f"kind {kind}")
    _run_closed_gga(rep, f"kind {kind}", [(1.0, kind)], kind)
    rep.done()


def _run_closed_mgga(rep, terms, kind=None):
    eng = _engine()
    for name in CLOSED:
        t = _closed_table(name)
        e, wv = eng.xc_eval_mgga(terms, _dev(eng, t["R"]), _dev(eng, t["tau"]), _dev(eng, np.full(len(t["rho"]), W)))
        e, wv = _np(e), _np(wv)
        vr, vs, vt = _raw_from_wv(t, wv)
        rep.exact_zero(f"xc_eval_mgga {name} wv", [wv], t["zero"])
        rep.finite(f"xc_eval_mgga {name} wv", [wv])
        _check_closed(rep, "xc_eval_mgga", name, t, terms, e, vr, vs, vt, kind=kind)
        _check_wv_rows(rep, f"xc_eval_mgga {name}", t, wv, vs)


@pytest.mark.parametrize("kind", MGGA_KINDS)
def test_closed_shell_meta_gga_kernel_at_the_edges(kind):
    rep = Report(f"kind {kind}")
    _run_closed_mgga(rep, [(1.0, kind)], kind)
    rep.done()


@pytest.mark.parametrize("name", list(COMPOSITES))
def test_composite_functionals_at_the_edges(name):
    rep = Report(name)
    if any(k in MGGA_KINDS for _c, k in COMPOSITES[name]):
        _run_closed_mgga(rep, COMPOSITES[name])
    else:
        _run_closed_gga(rep, name, COMPOSITES[name])
    rep.done()


# ---------------------------------------------------------------------------------------------
# spin-polarised
# ---------------------------------------------------------------------------------------------
def _spin_call(eng, kind, Ra, Rb, ta, tb, omega):
    """(e, wva, wvb) of one term: mi_xc_eval_spin for the GGA kinds, mi_xc_eval_mgga_spin for the meta-GGAs."""
    n = Ra.shape[1]
    w = _dev(eng, np.full(n, W))
    if kind in MGGA_KINDS:
        out = eng.xc_eval_mgga_spin([(1.0, kind)], _dev(eng, Ra), _dev(eng, Rb), _dev(eng, ta), _dev(eng, tb), w)
        return [_np(x) for x in out]
    e, wva, wvb = np.empty(n), np.empty((4, n)), np.empty((4, n))
    groups = [(np.arange(n), None)] if kind != 12 else [(np.nonzero(omega == om)[0], [float(om)]) for om in np.unique(omega)]
    for idx, prm in groups:
        out = eng.xc_eval_spin([(1.0, kind)], _dev(eng, Ra[:, idx]), _dev(eng, Rb[:, idx]), w[: len(idx)], True, params=prm)
        e[idx], wva[:, idx], wvb[:, idx] = (_np(x) for x in out)
    return e, wva, wvb


def _run_spin(kind):
    eng = _engine()
    entry = "xc_eval_mgga_spin" if kind in MGGA_KINDS else "xc_eval_spin"
    rep = Report(f"kind {kind}")
    # the closed-shell tables at rho_a = rho_b = rho / 2: both channels return the closed-shell wv
    for name in CLOSED:
        t = _closed_table(name)
        e, wva, wvb = _spin_call(eng, kind, 0.5 * t["R"], 0.5 * t["R"], 0.5 * t["tau"], 0.5 * t["tau"], t["omega"])
        rep.exact_zero(f"{entry} {name} wv", [wva, wvb], t["zero"])
        rep.finite(f"{entry} {name} wv", [wva, wvb])
        for s, wv in (("a", wva), ("b", wvb)):
            vr, vs, vt = _raw_from_wv(t, wv)
            if kind == 12:      # vsigma itself cannot be read off wv where the gradient vanishes: the rows below carry it
                vs = np.where(t["grad"][2] != 0, vs, t["d"][kind - 1][1])
            _check_closed(rep, f"{entry}[{s}]", name, t, [(1.0, kind)], e, vr, vs, vt, kind=kind)
            _check_spin_rows(rep, f"{entry}[{s}]", name, t, wv, [(1.0, kind)], kind)
    # polarised points: wv_s[0] = w/2 de/drho_s, wv_s[1..3] = w (2 de/dsigma_ss grad rho_s + de/dsigma_ab grad rho_s'),
    # wv_s[4] = w/4 de/dtau_s, built from the reference partials (ra, rb, saa, sab, sbb, ta, tb)
    for name in SPIN:
        t = _spin_table(name)
        e, wva, wvb = _spin_call(eng, kind, t["Ra"], t["Rb"], t["ta"], t["tb"], t["omega"])
        live = ~t["zero"]
        e_ref, d = t["e"][kind - 1], t["d"][kind - 1]
        scale = np.maximum(np.abs(e_ref), t["lda"])
        rep.exact_zero(f"{entry} {name}", [e, wva, wvb], t["zero"])
        rep.finite(f"{entry} {name}", [e, wva, wvb])
        if kind == 12:
            rep.check(f"{entry} {name} e (relative)", np.abs(e - e_ref)[live], (2e-9 * np.abs(e_ref))[live])
        else:
            rep.check(f"{entry} {name} e", np.abs(e - e_ref)[live], (_bound((entry, kind, name, "e"), 1e-11) * scale)[live], t["ye"][kind - 1][live])
        for s, wv, dr, dss, g_own, g_oth, dens, dt, tau, exempt in (("a", wva, d[0], d[2], t["ga"], t["gb"], t["pa"], d[5], t["ta"], t["exempt_a"]),
                                                                  ("b", wvb, d[1], d[4], t["gb"], t["ga"], t["pb"], d[6], t["tb"], t["exempt_b"])):
            # an exempt (clipped or dropped) minority channel only has to be finite, which is checked above; so does an
            # empty one, whose reference derivatives are NaN
            ok = live & ~exempt & (dens > 0)
            yd = t["yd"][kind - 1]
            iy = {"a": (0, 2, 5), "b": (1, 4, 6)}[s]
            tol = 2e-9 * np.abs(dr) if kind == 12 else _bound((entry, kind, name, f"vrho_{s}"), 1e-9) * scale
            wt = 1.0 if kind == 12 else dens
            rep.check(f"{entry} {name} vrho_{s}", (np.abs(wv[0] / (0.5 * W) - dr) * wt)[ok], (tol * np.ones_like(scale))[ok], (yd[iy[0]] * wt)[ok])
            ref = W * (2 * _mul0(dss[None, :], g_own) + _mul0(d[3][None, :], g_oth))
            err = (np.abs(wv[1:4] - ref) * np.abs(g_own)).sum(axis=0) / W
            if kind == 12:
                tol = 2e-9 * (np.abs(ref) * np.abs(g_own)).sum(axis=0) / W
            else:
                tol = _bound((entry, kind, name, f"vsigma_{s}"), 1e-9) * scale
            rep.check(f"{entry} {name} gradient rows of channel {s} (|dv| sigma)", err[ok], tol[ok], (2 * yd[iy[1]] * (g_own * g_own).sum(axis=0))[ok])
            if kind in MGGA_KINDS:
                rep.check(f"{entry} {name} vtau_{s}", (np.abs(wv[4] / (0.25 * W) - dt) * tau)[ok],
                          (_bound((entry, kind, name, f"vtau_{s}"), 1e-9) * scale)[ok], (yd[iy[2]] * tau)[ok])
    rep.done()


@pytest.mark.parametrize("kind", GGA_KINDS)
def test_spin_kernel_at_the_edges(kind):
    _run_spin(kind)


@pytest.mark.parametrize("kind", MGGA_KINDS)
def test_spin_meta_gga_kernel_at_the_edges(kind):
    _run_spin(kind)


# ---------------------------------------------------------------------------------------------
# second derivatives
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("triplet", [False, True], ids=["singlet", "triplet"])
@pytest.mark.parametrize("kind", GGA_KINDS)
def test_response_coefficients_at_the_edges(kind, triplet):
    """coef / w = {f_rr, f_rs, f_ss, v_sigma} (singlet) or the spin-difference {g_xx, g_xy, g_yy, g_z} (triplet) of
    engine.xc_fxc_prep against the reference's second derivatives: 1e-6 (|f_ref| + 1e-3 |v_ref| / den), v_ref the closed-shell
    vrho for f_rr and vsigma for the others (for the triplet the larger of the closed-shell vsigma and |g_z|), den = rho, rho,
    sigma, 1.  No finite-difference uncertainty and no mask: the reference is exact."""
    eng = _engine()
    rep = Report(f"kind {kind} {'triplet' if triplet else 'singlet'}")
    for name in CLOSED:
        t = _closed_table(name)
        n = len(t["rho"])
        coef = np.empty((4, n))
        for idx, prm in _omega_groups(t, [(1.0, kind)]):
            coef[:, idx] = _np(eng.xc_fxc_prep([(1.0, kind)], _dev(eng, t["R"][:, idx]), _dev(eng, np.full(len(idx), W)), True,
                                               triplet=triplet, params=prm)) / W
        ref = (t["ft"] if triplet else t["fs"])[kind - 1]
        live = ~t["zero"]
        rep.exact_zero(f"xc_fxc_prep {name}", [coef], t["zero"])
        rep.finite(f"xc_fxc_prep {name}", [coef])
        vr, vs = np.abs(t["d"][kind - 1][0]), np.abs(t["d"][kind - 1][1])
        if triplet:
            vs = np.maximum(vs, np.abs(ref[3]))
        rho, sig = t["rho"], np.maximum(t["sigma"], 1e-40)
        for k, (what, v, den) in enumerate((("f_rr", vr, rho), ("f_rs", vs, rho), ("f_ss", vs, sig), ("v_sigma", vs, 1.0))):
            with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
                tol = 1e-6 * (np.abs(ref[k]) + 1e-3 * v / den)
            rep.check(f"xc_fxc_prep {name} {what}", np.abs(coef[k] - ref[k])[live], tol[live])
    rep.done()
