"""A float64 NumPy model of the prime-factor chunk entries (tike_pfa_*), written
from include/tike_amd.h and the header comment of csrc/pfa.hip -- the layouts
and the contract of every stage, not the kernels.  test_pfa_entries_cpu.py pins
it to np.fft and to the oracle; test_pfa_entries_gpu.py holds every entry to it.

Layouts.  A det x det tile is p x p sub-tiles of M x M, (p, p, M, M) in memory.
  det = p M, p in {3, 5, 7}, M = 2^k in 32 .. 512 (prime factor, no twiddles):
    tile coordinate v lives in sub-tile v qM mod p at element v qp mod M
    (qM = M^-1 mod p, qp = p^-1 mod M), i.e. sub-tile n1, element n2 holds
    coordinate (M n1 + p n2) mod det; on the far side sub-tile k1, element k2
    is frequency (M qM k1 + p qp k2) mod det.
  det = 1024, 2048 (p = 4, M = det / 4, one Cooley-Tukey step): sub-tile n1,
    element n2 holds coordinate n1 + 4 n2; sub-tile k1, element k2 is frequency
    k2 + M k1; the sub-tile transforms are plain and the twiddle w_det^(n1 k2)
    belongs to the combine entry.
"""
import numpy as np

F8, C16 = np.float64, np.complex128


# ------------------------------------------------------------------ layouts
class Geom:
    """p, M and the two index maps of a supported detector size."""

    def __init__(self, det):
        self.det = det
        self.ct = det in (1024, 2048)
        if self.ct:
            self.p, self.M = 4, det // 4
        else:
            for p in (3, 5, 7):
                M = det // p
                if det % p == 0 and 32 <= M <= 512 and M & (M - 1) == 0:
                    self.p, self.M = p, M
                    break
            else:
                raise ValueError(f"no prime-factor layout for {det}")
        p, M = self.p, self.M
        n1, n2 = np.arange(p)[:, None], np.arange(M)[None, :]
        if self.ct:
            self.coord = n1 + p * n2
            self.freq = n2 + M * n1
        else:
            qM, qp = pow(M, -1, p), pow(p, -1, M)
            self.coord = (M * n1 + p * n2) % det
            self.freq = (M * qM * n1 + p * qp * n2) % det
            v = np.arange(det)  # the other statement of the same input map
            assert np.array_equal(self.coord[v * qM % p, v * qp % M], v)
        for m in (self.coord, self.freq):  # both are permutations of 0 .. det-1
            assert np.array_equal(np.sort(m.ravel()), np.arange(det))


def _to(tiles, m):
    return tiles[..., m[:, None, :, None], m[None, :, None, :]]


def _from(sub, m):
    out = np.empty((*sub.shape[:-4], m.size, m.size), sub.dtype)
    out[..., m[:, None, :, None], m[None, :, None, :]] = sub
    return out


def tile_to_subtiles(tiles, g):
    """(..., det, det) in tile coordinates -> (..., p, p, M, M), input side."""
    return _to(tiles, g.coord)


def subtiles_to_tile(sub, g):
    return _from(sub, g.coord)


def far_to_subtiles(far, g):
    """(..., det, det) indexed by frequency -> (..., p, p, M, M), far side."""
    return _to(far, g.freq)


def subtiles_to_far(sub, g):
    return _from(sub, g.freq)


def pad_tile(x, det):
    """Zero padding of (..., pw, pw) to (..., det, det), window at (det - pw) // 2."""
    pw = x.shape[-1]
    pad = (det - pw) // 2
    out = np.zeros((*x.shape[:-2], det, det), x.dtype)
    out[..., pad:pad + pw, pad:pad + pw] = x
    return out


def crop_tile(x, pw):
    pad = (x.shape[-1] - pw) // 2
    return x[..., pad:pad + pw, pad:pad + pw]


# ------------------------------------------------------------ bilinear gather
def patches_of(psi, scan, pw):
    """The convention of oracle/operators.py (patch_fwd) in float64: corner =
    floor(scan), also of negative coordinates; weights ((1-fx)(1-fy), fx(1-fy),
    (1-fx)fy, fx fy); a pixel whose leading tap is outside the image is zero;
    the trailing taps are addressed linearly (ii+1, ii+W, ii+W+1) and a tap
    beyond the allocation weighs zero.  psi (H, W), scan (N, 2) f32 (y, x)."""
    psi = np.asarray(psi, C16)
    H, W = psi.shape
    flat, total = psi.ravel(), psi.size
    scan = np.asarray(scan, np.float32).astype(F8).reshape(-1, 2)
    corner = np.floor(scan)
    fy, fx = (scan - corner).T
    sy, sx = corner.astype(np.int64).T
    w = np.stack([(1 - fx) * (1 - fy), fx * (1 - fy), (1 - fx) * fy, fx * fy], -1)
    yy = sy[:, None, None] + np.arange(pw)[:, None]
    xx = sx[:, None, None] + np.arange(pw)[None, :]
    valid = (yy >= 0) & (yy < H) & (xx >= 0) & (xx < W)
    ii = yy * W + xx
    out = np.zeros((len(scan), pw, pw), C16)
    for k, off in enumerate((0, 1, W, W + 1)):
        idx = ii + off
        ok = valid & (idx < total)
        out += np.where(ok, flat[np.clip(idx, 0, total - 1)], 0) * w[:, k, None, None]
    return out


# -------------------------------------------------------- probe of a position
FORMS = ("shared", "per_scan", "weights", "eigen", "unique")


def probe_of_positions(form, nscan, probe, weights=None, eigen=None, unique=None):
    """(nscan, S, pw, pw) c128, the probe of every position.
      shared    probe (S, pw, pw)
      per_scan  probe (nscan, S, pw, pw)
      weights   probe x weights[n][0][s]; weights (nscan, C + 1, S), no eigen probes
      eigen     ... + sum_c weights[n][c + 1][s] eigen[c][s] on modes s < Sm;
                eigen (C, Sm, pw, pw)
      unique    modes s < Sm from unique (nscan, Sm, pw, pw), already
                synthesised; the others probe x weights[n][0][s]"""
    probe = np.asarray(probe, C16)
    if form == "shared":
        return np.broadcast_to(probe, (nscan, *probe.shape)).copy()
    if form == "per_scan":
        assert probe.shape[0] == nscan
        return probe.copy()
    w = np.asarray(weights, F8)
    out = w[:, 0, :, None, None] * probe[None]
    if form == "eigen":
        e = np.asarray(eigen, C16)
        C, Sm = e.shape[:2]
        for c in range(C):
            out[:, :Sm] += w[:, c + 1, :Sm, None, None] * e[c][None]
    elif form == "unique":
        u = np.asarray(unique, C16)
        out[:, :u.shape[1]] = u
    else:
        assert form == "weights", form
    return out


# ------------------------------------------------------------------ the stages
def fwd_gather(psi, scan, probes, det):
    """tike_pfa_fwd_gather: (subtiles (N, S, p, p, M, M), patches (N, pw, pw))."""
    g = Geom(det)
    pw = probes.shape[-1]
    patches = patches_of(psi, scan, pw)
    return tile_to_subtiles(pad_tile(patches[:, None] * probes, det), g), patches


def subtile_fft(sub, inverse=False):
    """tike_pfa_fft2: the unscaled M x M transform of every sub-tile."""
    if inverse:
        return np.fft.ifft2(sub) * (sub.shape[-1] * sub.shape[-2])
    return np.fft.fft2(sub)


def _across(sub, g, inverse):
    """The p x p DFT across the sub-tiles, unscaled; at 1024 / 2048 with the
    twiddle w_det^(n1y k2y + n1x k2x) in front of it (its conjugate behind the
    inverse)."""
    p, M = g.p, g.M
    sign = 2j if inverse else -2j
    D = np.exp(sign * np.pi * np.outer(np.arange(p), np.arange(p)) / p)
    tw = 1.0
    if g.ct:
        w1 = np.exp(sign * np.pi * np.outer(np.arange(p), np.arange(M)) / g.det)
        tw = w1[:, None, :, None] * w1[None, :, None, :]  # (n1y, n1x, k2y, k2x)
    if not inverse:
        return np.einsum("ka,lb,...abyx->...klyx", D, D, sub * tw)
    return np.einsum("ak,bl,...klyx->...abyx", D, D, sub) * tw


def far_plane(sub_hat, det, fwd_scale):
    """F (N, S, det, det), indexed by frequency, from the transformed sub-tiles."""
    g = Geom(det)
    return subtiles_to_far(fwd_scale * _across(np.asarray(sub_hat, C16), g, False), g)


def cost_terms(I, data, model):
    """Per-pixel cost and gradient factor (objective.py:11-124)."""
    with np.errstate(invalid="ignore", divide="ignore"):
        if model == 0:
            sI, sd = np.sqrt(I), np.sqrt(data)
            return np.square(sI - sd), -(1 - sd / (sI + I.dtype.type(1e-9)))
        return (I - data * np.log(I + I.dtype.type(1e-9)),
                -(1 - data / (I + I.dtype.type(1e-9))))


def costs_and_factor(F, data, mask, model, unmeasured_scaling, num_measured,
                     dtype=F8):
    """costs (N,), the mean over measured pixels; factor (N, det, det).  In
    `dtype` throughout: float32 restates what a float32 implementation of the
    same formula may be off by (the bar of the costs)."""
    F = np.asarray(F, np.complex64 if dtype == np.float32 else C16)
    I = np.sum(np.square(F.real) + np.square(F.imag), axis=1, dtype=dtype)
    data = np.asarray(data, dtype)
    ms = np.ones(I.shape[-2:], bool) if mask is None else np.asarray(mask) != 0
    term, gg = cost_terms(I, data, model)
    costs = np.sum(np.where(ms, term, 0), axis=(-2, -1), dtype=dtype) / dtype(num_measured)
    factor = np.where(ms, gg, dtype(unmeasured_scaling) - dtype(1))
    mean_abs = np.sum(np.where(ms, np.abs(term), 0), axis=(-2, -1),
                      dtype=F8) / num_measured
    return costs, factor, I, mean_abs


def combine_gradient(sub_hat, data, mask, det, fwd_scale, model,
                     unmeasured_scaling, num_measured):
    """tike_pfa_combine_gradient: (what it leaves in place, costs, F, I)."""
    g = Geom(det)
    F = far_plane(sub_hat, det, fwd_scale)
    costs, factor, I, _ = costs_and_factor(F, data, mask, model,
                                           unmeasured_scaling, num_measured)
    G = far_to_subtiles(F * factor[:, None], g)
    return _across(G, g, True), costs, F, I


def inv_products(sub, patches, probes, det, inv_scale, scale=1.0, m_probe_update=None):
    """tike_pfa_inv_products on the inverse sub-tile transforms' output:
    (objproj (N, pw, pw), chi0 (N, pw, pw), m_probe_update (S, pw, pw), chi)."""
    g = Geom(det)
    pw = probes.shape[-1]
    chi = inv_scale * crop_tile(subtiles_to_tile(np.asarray(sub, C16), g), pw)
    objproj = np.sum(np.conj(probes) * chi, axis=1)
    mpu = scale * np.sum(np.conj(np.asarray(patches, C16))[:, None] * chi, axis=0)
    if m_probe_update is not None:
        mpu = mpu + np.asarray(m_probe_update, C16)
    return objproj, chi[:, 0].copy(), mpu, chi


# ------------------------------------------------- inputs with a chosen far plane
def subtiles_from_far(F, det, fwd_scale):
    """The transformed sub-tiles (input of the combine entry) whose far plane is
    F (N, S, det, det), rounded to complex64."""
    g = Geom(det)
    return (_across(far_to_subtiles(np.asarray(F, C16), g), g, True) /
            (g.p * g.p * fwd_scale)).astype(np.complex64)


def combine_case(det, nscan, S, seed, mask_fraction=0.15):
    """Inputs of the combine entry from a chosen far plane: |F| uniform in
    [0.5, 2] with random phase per mode, so the intensity is never dark;
    non-negative counts with exact zeros on at least 1 % of the measured
    pixels; a random mask of `mask_fraction` with NaN counts under it (the
    `data_nan` / `mask` pair; `data` is the same without NaN for mask NULL)."""
    rng = np.random.default_rng(seed)
    shape = (nscan, S, det, det)
    F = rng.uniform(0.5, 2.0, shape) * np.exp(2j * np.pi * rng.random(shape))
    fwd_scale = 1.0 / det
    sub = subtiles_from_far(F, det, fwd_scale)
    I0 = np.sum(np.abs(F)**2, axis=1)
    data = (I0 * rng.uniform(0.3, 1.7, I0.shape)).astype(np.float32)
    data[rng.random(data.shape) < 0.02] = 0.0
    mask = (rng.random((det, det)) >= mask_fraction).astype(np.uint8)
    data_nan = data.copy()
    data_nan[:, mask == 0] = np.nan
    return dict(sub=sub, data=data, data_nan=data_nan, mask=mask,
                fwd_scale=fwd_scale, det=det, nscan=nscan, S=S)


def check_combine_case(c):
    """The input conditions, on the float64 model of the ROUNDED sub-tiles."""
    F = far_plane(c["sub"], c["det"], c["fwd_scale"])
    I = np.sum(np.abs(F)**2, axis=1)
    for mask, data in ((None, c["data"]), (c["mask"], c["data_nan"])):
        ms = np.ones(I.shape[-2:], bool) if mask is None else mask != 0
        assert I[:, ms].min() >= 0.25, I[:, ms].min()
        d = data[:, ms]
        assert np.all(d >= 0) and np.mean(d == 0) >= 0.01
        assert np.isfinite(d).all()
    assert np.isnan(c["data_nan"][:, c["mask"] == 0]).all()
    assert 0.05 < np.mean(c["mask"] == 0) < 0.25
    return F, I
