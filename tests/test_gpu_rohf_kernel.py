"""`mi_rohf_fock` against a few lines of numpy on random symmetric Fa, Fb: F_eff and G are selections and one half-sum, so they
must agree to 1e-14 max|F|; the finished |G|^2 sum to 1e-12 relative and the maximum exactly (a maximum of the same FP64 numbers);
elements beyond `nmo` of a padded row must keep their sentinel."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SENTINEL = -7.25


def _classes(nmo, ncore, nopen):
    return np.repeat([0, 1, 2], [ncore, nopen, nmo - ncore - nopen])


def ref_rohf_fock(fa, fb, ncore, nopen):
    """(F_eff, G): Fb between closed and open, Fa between open and virtual, (Fa + Fb) / 2 elsewhere; G = sgn(class_i - class_j) F_eff."""
    cls = _classes(fa.shape[0], ncore, nopen)
    lo, hi = np.minimum.outer(cls, cls), np.maximum.outer(cls, cls)
    f = np.where((lo == 0) & (hi == 1), fb, np.where((lo == 1) & (hi == 2), fa, 0.5 * (fa + fb)))
    return f, np.sign(np.subtract.outer(cls, cls)) * f


def _pairs(nmo):
    cand = [(0, 0), (0, 1), (0, nmo), (3, 0), (3, 2), (nmo, 0), (nmo - 1, 1)]
    return sorted({(c, o) for c, o in cand if c >= 0 and o >= 0 and c + o <= nmo})


CASES = [(nmo, pad, c, o) for nmo in (1, 7, 8, 9, 33, 65) for pad in (0, 3) for c, o in _pairs(nmo)]


@pytest.mark.parametrize("nmo,pad,ncore,nopen", CASES)
def test_rohf_fock_matches_numpy(nmo, pad, ncore, nopen):
    import torch
    from mi355scf import engine, rohf
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(1000 * nmo + 10 * ncore + nopen + pad)
    fa, fb = (rng.normal(size=(nmo, nmo)) for _ in range(2))
    fa, fb = fa + fa.T, fb + fb.T
    ld = nmo + pad
    bufs = []
    for m in (fa, fb):
        b = torch.full((nmo, ld), SENTINEL, dtype=torch.float64, device=dev)
        b[:, :nmo] = torch.as_tensor(m, device=dev)
        bufs.append(b)
    L = engine.lib()
    nb = int(L.mi_rohf_fock_blocks())
    out_f = torch.full((nmo, ld), SENTINEL, dtype=torch.float64, device=dev)
    out_g = torch.full((nmo, ld), SENTINEL, dtype=torch.float64, device=dev)
    part = torch.full((2 * nb,), SENTINEL, dtype=torch.float64, device=dev)
    engine._check(L.mi_rohf_fock(bufs[0].data_ptr(), bufs[1].data_ptr(), ld, ncore, nopen, nmo, out_f.data_ptr(), out_g.data_ptr(),
                                 part.data_ptr(), None))
    torch.cuda.synchronize()
    f, g, p = out_f.cpu().numpy(), out_g.cpu().numpy(), part.cpu().numpy()
    f_ref, g_ref = ref_rohf_fock(fa, fb, ncore, nopen)
    scale = max(np.abs(fa).max(), np.abs(fb).max())
    err_f, err_g = np.abs(f[:, :nmo] - f_ref).max(), np.abs(g[:, :nmo] - g_ref).max()
    g2, g2_ref = p[:nb].sum(), np.sum(g_ref * g_ref)
    print(f"nmo {nmo} ld {ld} (ncore, nopen) ({ncore}, {nopen}): F_eff error {err_f:.1e}, G error {err_g:.1e}, |G|^2 {g2:.6e} vs {g2_ref:.6e}, "
          f"max |G| {p[nb:].max():.6e}")
    assert err_f <= 1e-14 * scale and err_g <= 1e-14 * scale
    assert abs(g2 - g2_ref) <= 1e-12 * max(g2_ref, 1e-300) and p[nb:].max() == np.abs(g_ref).max()
    assert np.all(g[:, :nmo] == -g[:, :nmo].T)                                  # antisymmetric, bit for bit (symmetric input)
    assert np.all(f[:, nmo:] == SENTINEL) and np.all(g[:, nmo:] == SENTINEL)    # padding untouched
    assert np.all(bufs[0].cpu().numpy()[:, :nmo] == fa) and np.all(bufs[1].cpu().numpy()[:, :nmo] == fb)     # inputs untouched
    # the Python wrapper takes the same padded views
    f2, g2w, p2 = rohf.rohf_fock(bufs[0][:, :nmo], bufs[1][:, :nmo], ncore, nopen)
    assert torch.equal(f2, out_f[:, :nmo]) and torch.equal(g2w, out_g[:, :nmo]) and torch.equal(p2, part)


def test_rohf_fock_refuses_bad_sizes():
    import torch
    from mi355scf import engine
    L = engine.lib()
    x = torch.zeros(16, dtype=torch.float64, device="cuda:0")
    p = torch.zeros(2 * int(L.mi_rohf_fock_blocks()), dtype=torch.float64, device="cuda:0")
    for ld, ncore, nopen, nmo in ((4, 3, 2, 4), (3, 1, 1, 4), (4, -1, 1, 4), (4, 0, 0, 0)):
        assert L.mi_rohf_fock(x.data_ptr(), x.data_ptr(), ld, ncore, nopen, nmo, x.data_ptr(), x.data_ptr(), p.data_ptr(), None) != 0
