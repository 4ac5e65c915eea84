"""One launch past 4 GiB / past 65 536 positions: the model, the replica
construction and the per-position comparison the large-launch tests share.

* A float64 / complex128 model of ONE chunk of the lstsq minibatch
  (`chunk_model`) and of the operators (`ptycho_fwd`, `ptycho_adj`, `fft2`,
  `ifft2`), in plain NumPy, written from the formulas of the reference
  (lstsq.py:367-602, convolution.cu:35-134, objective.py:11-124,
  exitwave.py:122-184, position.py:779-810) -- not from oracle/, which is
  float32, and not from the kernels.
* The replica construction: a base problem of `n0` distinct positions repeated
  R times ON THE DEVICE.  Every per-position output of replica r must equal
  the float64 result of base position i; every accumulated output R x the
  base accumulation.  An index that wrapped at 32 bits reads a position a
  fixed distance away; `assert_no_aliasing` computes that this distance is
  never a whole number of replicas, so the position it lands on differs.
* `positions_for`: the number of positions that carries an array past a
  threshold by at least one whole replica.
* `position_errors` / `accumulated_error`: the comparison, on the device, in
  slabs (no temporary above `SLAB_BYTES`, no big array on the host).

No GPU import at module level: the CPU tests use the model and the helpers."""
import numpy as np

F8, C16 = np.float64, np.complex128
EPS32 = 2.0 ** -24  # unit roundoff of float32
SLAB_BYTES = 1 << 28  # of one temporary of the device comparison

# what a 32-bit slip can wrap by: bytes ...
WRAP_BYTES = {
    "2^32 bytes": 1 << 32,
    "2^31 floats": 4 << 31,
    "2^32 floats": 4 << 32,
    "2^31 complex elements": 8 << 31,
}
# ... and positions or tiles (a launch dimension, a 24-bit multiply)
WRAP_COUNTS = {"2^16": 1 << 16, "2^24": 1 << 24}


# ---------------------------------------------------------------- replicas
def positions_for(span_bytes_per_position, n0, threshold):
    """The smallest multiple of n0 positions whose span (positions x
    span_bytes_per_position) exceeds `threshold` by at least one whole
    replica (n0 positions)."""
    span = int(span_bytes_per_position)
    assert span >= 1 and n0 >= 1 and threshold >= 0
    rep = n0 * span
    return n0 * (-(-(int(threshold) + rep) // rep))


def aliasing_distances(strides, tiles_per_position, n0, counts=()):
    """[(array, wrap, positions)] for every wrap distance that is a WHOLE
    number of positions of an array.  strides: {array: bytes per position};
    tiles_per_position: the counts a launch indexes per position (1: the
    positions themselves, S: tiles); counts: further count distances (the
    device's grid limit as read at run time)."""
    out = []
    for name, stride in strides.items():
        for wrap, nbytes in WRAP_BYTES.items():
            if nbytes % stride == 0:
                out.append((name, wrap, nbytes // stride))
    for per in sorted(set(tiles_per_position)):
        for wrap, count in list(WRAP_COUNTS.items()) + [
                (str(c), int(c)) for c in counts]:
            if count % per == 0:
                out.append((f"{per} tile(s) per position", wrap, count // per))
    return out


def assert_no_aliasing(strides, tiles_per_position, n0, counts=()):
    """A wrapped access must land on a position of ANOTHER base index: no wrap
    distance may be a whole number of replicas.  (A distance that is no whole
    number of positions lands inside a position, off its first element, and
    is not listed.)"""
    assert n0 % 2 == 1 and n0 >= 5, n0
    bad = [(a, w, d) for a, w, d in aliasing_distances(
        strides, tiles_per_position, n0, counts) if d % n0 == 0]
    assert not bad, f"a wrapped access lands on an identical replica: {bad}"


# --------------------------------------------------------------- transforms
def fft2(x):
    """Ortho 2-D DFT over the last two axes, complex128."""
    return np.fft.fft2(np.asarray(x, C16), norm="ortho")


def ifft2(x):
    return np.fft.ifft2(np.asarray(x, C16), norm="ortho")


# --------------------------------------------------------- patches, probes
def _corners(scan):
    """Integer corner and the four bilinear weights of every position
    (convolution.cu:101-134); scan (n, 2) = (y, x)."""
    scan = np.asarray(scan, F8)
    c = np.floor(scan)
    f = scan - c
    fy, fx = f[:, 0], f[:, 1]
    w = np.stack([(1 - fx) * (1 - fy), fx * (1 - fy), (1 - fx) * fy, fx * fy],
                 1)
    return c.astype(np.int64), w


_TAPS = ((0, 0), (0, 1), (1, 0), (1, 1))


def patches_of(psi, scan, pw):
    """Bilinear gather of (n, pw, pw) patches from psi (H, W)."""
    psi = np.asarray(psi, C16)
    corner, w = _corners(scan)
    out = np.zeros((len(corner), pw, pw), C16)
    for n, (sy, sx) in enumerate(corner):
        for t, (dy, dx) in enumerate(_TAPS):
            out[n] += w[n, t] * psi[sy + dy:sy + dy + pw, sx + dx:sx + dx + pw]
    return out


def scatter(proj, scan, H, W):
    """The adjoint of `patches_of`: (image, sum of |terms|, number of terms)
    per pixel, for proj (n, pw, pw)."""
    proj = np.asarray(proj, C16)
    pw = proj.shape[-1]
    corner, w = _corners(scan)
    img = np.zeros((H, W), C16)
    mag = np.zeros((H, W), F8)
    cnt = np.zeros((H, W), F8)
    for n, (sy, sx) in enumerate(corner):
        for t, (dy, dx) in enumerate(_TAPS):
            sl = (slice(sy + dy, sy + dy + pw), slice(sx + dx, sx + dx + pw))
            img[sl] += w[n, t] * proj[n]
            mag[sl] += w[n, t] * np.abs(proj[n])
            cnt[sl] += 1
    return img, mag, cnt


def varying_probe(probe, eigen, weights, n):
    """(n, S, pw, pw): weights[n][0][s] probe_s + sum_c weights[n][c+1][s]
    eigen[c][s] for the modes that own eigen probes (probe.py:272-303); the
    shared probe for every position when there are no weights."""
    probe = np.asarray(probe, C16).reshape(probe.shape[-3:])
    if weights is None:
        return np.broadcast_to(probe, (n, *probe.shape)).copy()
    weights = np.asarray(weights, F8)
    u = weights[:, 0, :, None, None] * probe
    if eigen is not None:
        eigen = np.asarray(eigen, C16)
        eigen = eigen.reshape(eigen.shape[-4:])
        for c in range(eigen.shape[0]):
            m = eigen.shape[1]
            u[:, :m] += weights[:, c + 1, :m, None, None] * eigen[c]
    return u


def _pad(x, det):
    pw = x.shape[-1]
    pad = (det - pw) // 2
    out = np.zeros((*x.shape[:-2], det, det), C16)
    out[..., pad:pad + pw, pad:pad + pw] = x
    return out


def _crop(x, pw):
    pad = (x.shape[-1] - pw) // 2
    return x[..., pad:pad + pw, pad:pad + pw]


# ------------------------------------------------------------- operators
def ptycho_fwd(probe, scan, psi, det, eigen=None, weights=None):
    """Far-plane waves (n, S, det, det) of the positions."""
    pw = probe.shape[-1]
    u = varying_probe(probe, eigen, weights, len(scan))
    return fft2(_pad(patches_of(psi, scan, pw)[:, None] * u, det))


def ptycho_adj(farplane, probe, scan, psi):
    """(psi_adj (H, W), probe_adj (n, S, pw, pw)) for far planes (n, S, det,
    det) and ONE probe per position (n, S, pw, pw): the adjoint of the
    forward operator with respect to the object and to the probe."""
    probe = np.asarray(probe, C16)
    pw = probe.shape[-1]
    H, W = psi.shape[-2:]
    near = _crop(ifft2(farplane), pw)
    psi_adj = scatter(np.sum(np.conj(probe) * near, 1), scan, H, W)[0]
    probe_adj = np.conj(patches_of(psi, scan, pw))[:, None] * near
    return psi_adj, probe_adj


# --------------------------------------------------- position shift terms
def _derivative_taps(sigma=0.333, truncate=6.0):
    r = int(truncate * sigma + 0.5)
    d = np.arange(-r, r + 1)
    phi = np.exp(-0.5 / (sigma * sigma) * d ** 2)
    return -(d / (sigma * sigma)) * (phi / phi.sum())


def _derivative(x, axis):
    """sum_d taps[d] x[i + d] along `axis`, edges repeated."""
    taps = _derivative_taps()
    r = len(taps) // 2
    n = x.shape[axis]
    out = np.zeros_like(x)
    for k, t in enumerate(taps):
        idx = np.clip(np.arange(n) + k - r, 0, n - 1)
        out += t * np.take(x, idx, axis=axis)
    return out


def position_terms(patches, unique0, chi0):
    """Numerator / denominator (n, 2) of the shift estimate (lstsq.py:545-579):
    chi of mode 0 on the two derivative exit waves, central half."""
    pw = patches.shape[-1]
    c = slice(pw // 4, pw - pw // 4)
    num = np.zeros((len(patches), 2))
    den = np.zeros((len(patches), 2))
    for k, axis in enumerate((-2, -1)):
        gp = _derivative(patches, axis)[:, c, c] * unique0[:, c, c]
        num[:, k] = np.sum((np.conj(gp) * chi0[:, c, c]).real, axis=(-2, -1))
        den[:, k] = np.sum(np.abs(gp) ** 2, axis=(-2, -1))
    return num, den


# ----------------------------------------------------- one lstsq chunk
def chunk_model(psi, scan, probe, eigen, weights, data, mask, det, *,
                noise_model="gaussian", unmeasured=1.0, num_batch=1,
                step_start=0.5, step_weight=0.5):
    """Everything one chunk of `_get_nearplane_gradients` produces, for the n
    positions given, in float64.  psi (H, W); probe (S, pw, pw); eigen (C, Sm,
    pw, pw) or None; weights (n, C + 1, S) or None; data (n, det, det); mask
    (det, det) bool.  Poisson: the per-mode step lengths of 'all_modes'."""
    psi = np.asarray(psi, C16).reshape(psi.shape[-2:])
    H, W = psi.shape
    n = len(scan)
    pw = probe.shape[-1]
    d = np.asarray(data, F8)
    mask = np.asarray(mask, bool)
    patches = patches_of(psi, scan, pw)
    unique = varying_probe(probe, eigen, weights, n)
    far = fft2(_pad(patches[:, None] * unique, det))
    abs2 = np.abs(far) ** 2
    inten = abs2.sum(1)
    dm = np.where(mask, d, 0.0)  # unmeasured counts (NaN, garbage): never read
    if noise_model == "gaussian":
        term = (np.sqrt(inten) - np.sqrt(dm)) ** 2
        g = -(1 - np.sqrt(dm) / (np.sqrt(inten) + 1e-9))
        g = np.broadcast_to(g[:, None], far.shape)
    else:
        term = inten - dm * np.log(inten + 1e-9)
        xi = (1 - dm / (inten + 1e-9))[:, None]
        xa = xi * abs2
        m = np.broadcast_to(mask, abs2.shape)
        den_final = np.sum(xi * xa, axis=(-2, -1), where=m)
        step = np.full((n, far.shape[1], 1, 1), float(step_start))
        for _ in range(2):
            xam1 = xi * step - 1
            den = np.where(m, abs2 * xam1 ** 2 + inten[:, None] - abs2, 1.0)
            numer = np.sum(xa * (1 + dm[:, None] * xam1 / den), axis=(-2, -1),
                           where=m)
            step = (step * (1 - step_weight) +
                    (numer / den_final)[..., None, None] * step_weight)
        g = -step * xi
    costs = np.sum(term, axis=(-2, -1),
                   where=np.broadcast_to(mask, term.shape)) / mask.sum()
    g = np.where(mask[None, None], g, unmeasured - 1.0)
    chi = _crop(ifft2(far * g), pw)
    objproj = np.sum(np.conj(unique) * chi, 1)
    obj, obj_mag, obj_cnt = scatter(objproj, scan, H, W)
    mpu_terms = np.conj(patches)[:, None] * chi
    pos_num, pos_den = position_terms(patches, unique[:, 0], chi[:, 0])
    return dict(
        patches=patches, unique=unique, far=far, intensity=inten, costs=costs,
        gscale=g, chi=chi, chi0=chi[:, 0], objproj=objproj,
        object_upd_sum=obj, object_abs=obj_mag, object_terms=obj_cnt,
        m_probe_update=mpu_terms.sum(0) / num_batch,
        m_probe_abs=np.abs(mpu_terms).sum(0) / num_batch,
        position_numerator=pos_num, position_denominator=pos_den)


# ------------------------------------------------------- the base problem
def base_problem(det, S, n0, seed, *, pw=None, eigen=True, margin=24):
    """n0 distinct random positions on a small object, float32 / complex64 as
    the device gets them: dict(scan, psi, psi_true, probe, eigen, weights,
    data).  data = the model's intensity at psi_true (float32); psi = psi_true
    with 10 % noise, so the patterns are nearly fitted -- the hard case for
    the costs."""
    pw = pw or det
    rng = np.random.default_rng(seed)
    HW = pw + margin
    scan = (1 + (margin - 3) * rng.random((n0, 2))).astype(np.float32)
    assert len({tuple(r) for r in scan}) == n0
    psi_true = ((0.75 + 0.25 * rng.random((1, HW, HW))) * np.exp(
        1j * np.pi * (rng.random((1, HW, HW)) - 0.5))).astype(np.complex64)
    y = (np.arange(pw) - (pw - 1) / 2) / (pw / 2)
    window = np.exp(-0.5 * (y[:, None] ** 2 + y[None, :] ** 2) / 0.3 ** 2)
    probe = np.stack([window * np.exp(1j * np.pi * rng.random((pw, pw))) /
                      (m + 1) for m in range(S)])[None, None].astype(
                          np.complex64)
    ep = ew = None
    if eigen:
        ep = (window * np.exp(2j * np.pi * rng.random((pw, pw))))[
            None, None, None].astype(np.complex64)
        ep /= np.sqrt(np.mean(np.abs(ep) ** 2))
        ew = np.zeros((n0, 2, S), np.float32)
        ew[:, 0] = 1 + 0.02 * rng.standard_normal((n0, S))
        ew[:, 1, 0] = 0.05 * rng.standard_normal(n0)
    data = (np.abs(ptycho_fwd(probe, scan, psi_true[0], det, ep, ew)) ** 2
            ).sum(1).astype(np.float32)
    psi = (psi_true * (1 + 0.1 * rng.standard_normal(psi_true.shape))).astype(
        np.complex64)
    probe0 = (probe * (1 + 0.05 * rng.standard_normal(probe.shape))).astype(
        np.complex64)
    return dict(scan=scan, psi=psi, psi_true=psi_true, probe=probe0, eigen=ep,
                weights=ew, data=data, det=det, pw=pw, S=S, n0=n0)


# -------------------------------------------- cases (shapes of the issue)
FOUR_GIB = 1 << 32
N0_BYTES, N0_COUNT = 5, 7


def _case(name, route, det, S, axis="bytes", **kw):
    n0 = kw.pop("n0", N0_BYTES if axis == "bytes" else N0_COUNT)
    if axis == "bytes":
        N = positions_for(S * det * det * 8, n0, FOUR_GIB)
    else:
        N = positions_for(1, n0, 1 << 16)
    return dict(name=name, route=route, det=det, S=S, n0=n0, N=N, axis=axis,
                **kw)


CHUNK_CASES = [
    # (one_launch: `tike_fwd_grad_ifft2_pass1`, the kernel of record)
    _case("no_farplane-256x8", "no_farplane", 256, 8,
          expect=dict(one_launch=True)),
    _case("no_farplane-256x8-u16-mask", "no_farplane", 256, 8, u16_mask=True,
          expect=dict(one_launch=True)),
    _case("no_farplane-256x8-u16-mask-deterministic", "no_farplane", 256, 8,
          u16_mask=True, deterministic=True, expect=dict(one_launch=True)),
    _case("no_farplane-256x8-poisson", "no_farplane", 256, 8,
          noise_model="poisson", expect=dict(steps_in_pass2=True)),
    _case("no_farplane-512x4-positions", "no_farplane", 512, 4,
          positions=True),
    _case("mode-groups-256x12", "no_farplane", 256, 12,
          expect=dict(groups=True)),
    _case("pos_major-128x8", "pos_major", 128, 8),
    _case("pfa-384x4", "pfa", 384, 4),
    _case("general-300x2", "general", 300, 2,
          switches=dict(GENERAL_FUSED="always", PFA_ROUTE=False)),
    _case("unfused-100x8", "unfused", 100, 8),
    _case("split_kept-256x2-poisson", "split_kept", 256, 2,
          noise_model="poisson", switches=dict(POISSON_FROM_HANDOFF=False)),
    _case("unfused-16x1-count", "unfused", 16, 1, axis="count"),
    _case("unfused-32x3-count", "unfused", 32, 3, axis="count"),
]
ROUTES = ("pfa", "general", "no_farplane", "split_kept", "pos_major",
          "unfused")


def case_strides(case):
    """Bytes per position of every array one chunk of the case indexes by
    position, and the tile counts per position its launches use."""
    det, S = case["det"], case["S"]
    pw = case.get("pw") or det
    u16 = bool(case.get("u16_mask"))
    strides = {
        "far / mid": 8 * S * det * det,
        "one mode of far": 8 * det * det,
        "chi": 8 * S * pw * pw,
        "patches / chi0 / objproj": 8 * pw * pw,
        "data": (2 if u16 else 4) * det * det,
        "intensity / gscale": 4 * det * det,
        "scan": 8,
        "costs": 4,
        "weights": 4 * 2 * S,
        "steps": 4 * S,
    }
    return strides, (1, S)


# ------------------------------------------------- comparison on the device
def position_errors(got, want, n0):
    """Per-position normwise error ||got_n - want_i|| / ||want_i|| (i = n mod
    n0) of a device tensor got (N, ...) against the host model want (n0, ...),
    as a float64 device tensor (N,).  Reduced slab by slab over (R, n0, ...)
    views: nothing larger than SLAB_BYTES is formed."""
    import torch
    N = got.shape[0]
    assert N % n0 == 0 and tuple(got.shape[1:]) == tuple(want.shape[1:]), (
        got.shape, want.shape)
    cplx = got.is_complex()
    w = torch.from_numpy(np.ascontiguousarray(
        want, dtype=C16 if cplx else F8)).to(got.device).reshape(n0, -1)
    den = torch.linalg.vector_norm(w, dim=1)
    den = torch.where(den > 0, den, torch.ones_like(den))
    R = N // n0
    view = got.reshape(R, n0, -1)
    step = max(1, SLAB_BYTES // (w.numel() * w.element_size()))
    out = torch.empty((R, n0), dtype=torch.float64, device=got.device)
    for lo in range(0, R, step):
        diff = view[lo:lo + step].to(w.dtype)
        diff -= w
        out[lo:lo + step] = torch.linalg.vector_norm(diff, dim=2) / den
        del diff
    return out.reshape(N)


def worst(errors, n0):
    """(largest error -- NaN counts as infinite --, its position, its base
    index) of a per-position error tensor."""
    import torch
    e = torch.nan_to_num(errors, nan=float("inf"))
    k = int(torch.argmax(e))
    return float(e[k]), k, k % n0


def accumulation_bound(abs_terms, additions):
    """What float32 accumulation may add to an entry: (number of float32
    additions into it) x 2^-24 x sum |terms|, entrywise, from the float64
    model."""
    return np.asarray(additions, F8) * EPS32 * np.asarray(abs_terms, F8)


def accumulated_error(got, want, bound):
    """(||got - want||, ||want||, ||bound||) of an accumulated output: the
    bar of the per-position outputs applies to the first against the second,
    plus the third."""
    import torch
    cplx = got.is_complex()
    w = torch.from_numpy(np.ascontiguousarray(
        want, dtype=C16 if cplx else F8)).to(got.device).reshape(got.shape)
    assert bool(torch.isfinite(torch.view_as_real(got) if cplx else got
                               ).all()), "non-finite accumulated output"
    return (float(torch.linalg.vector_norm(got.to(w.dtype) - w)),
            float(torch.linalg.vector_norm(w)),
            float(np.linalg.norm(np.ravel(bound))))


def entrywise_excess(got, want, bound, bar):
    """max over the entries of |got - want| / (bar x max|want| + bound): the
    accumulated output entry by entry -- an entry with few contributions
    cannot borrow from the bound of a deep one.  <= 1 passes."""
    import torch
    cplx = got.is_complex()
    w = torch.from_numpy(np.ascontiguousarray(
        want, dtype=C16 if cplx else F8)).to(got.device).reshape(got.shape)
    b = torch.from_numpy(np.ascontiguousarray(bound, dtype=F8)).to(
        got.device).reshape(got.shape)
    tol = bar * float(w.abs().max()) + b
    ratio = torch.nan_to_num((got.to(w.dtype) - w).abs() / tol,
                             nan=float("inf"))
    return float(ratio.max())


# ------------------------------------------- rpie on an object of slices
def multislice_rpie_model(psi, scan, probe, data, propagator):
    """The numerators one minibatch of rpie forms for an object of D slices
    (rpie.py:367-495, multislice.py:69-141, fresnelspectprop.py:52-113),
    gaussian model, every pixel measured, probe window = detector, in
    float64.  psi (D, H, W); probe (S, pw, pw); propagator (pw, pw).  The
    wave behind slice t reaches slice t + 1 as IFFT2(FFT2(.) H); on the way
    back the exit-wave update goes to the slice in front as IFFT2(FFT2(.)
    conj(H)).  psi_num[t] = scatter(sum_s conj(incident_t) diff) / S and
    probe_num[t] = sum_n conj(patch_t) diff, with their sums of |terms| and
    term counts; chi0 = mode 0 of the update at the first slice."""
    psi = np.asarray(psi, C16)
    D, H, W = psi.shape
    Hp = np.asarray(propagator, C16)
    d = np.asarray(data, F8)
    n = len(scan)
    pw = probe.shape[-1]
    S = probe.shape[-3]
    incident = [varying_probe(probe, None, None, n)]
    patches = []
    for t in range(D):
        patches.append(patches_of(psi[t], scan, pw))
        wave = patches[t][:, None] * incident[t]
        if t < D - 1:
            incident.append(ifft2(fft2(wave) * Hp))
    far = fft2(wave)
    inten = (np.abs(far) ** 2).sum(1)
    costs = ((np.sqrt(inten) - np.sqrt(d)) ** 2).mean((-2, -1))
    g = -(1 - np.sqrt(d) / (np.sqrt(inten) + 1e-9))
    diff = ifft2(far * g[:, None])
    out = dict(costs=costs, psi_num=np.zeros((D, H, W), C16),
               psi_abs=np.zeros((D, H, W)), psi_terms=np.zeros((D, H, W)),
               probe_num=np.zeros((D, S, pw, pw), C16),
               probe_abs=np.zeros((D, S, pw, pw)))
    for t in range(D - 1, -1, -1):
        img, mag, cnt = scatter(np.sum(np.conj(incident[t]) * diff, 1), scan,
                                H, W)
        out["psi_num"][t], out["psi_abs"][t] = img / S, mag / S
        out["psi_terms"][t] = cnt
        terms = np.conj(patches[t])[:, None] * diff
        out["probe_num"][t] = terms.sum(0)
        out["probe_abs"][t] = np.abs(terms).sum(0)
        if t == 0:
            break
        diff = ifft2(fft2(diff) * np.conj(Hp))
    out["chi0"] = diff[:, 0]
    return out
