"""Float64 NumPy model of the difference-map solver (`tike_amd.ptycho.solvers
.dm`) and of its two C-ABI entries, `tike_dm_reflect` and `tike_dm_update`.
There is no reference counterpart: this model and the solver's docstring
define the algorithm.  Everything here is plain NumPy in float64 /
complex128 and shares no code with the package."""
import numpy as np


def _corner(scan):
    y, x = np.asarray(scan[0], np.float64), np.asarray(scan[1], np.float64)
    sy, sx = int(np.floor(y)), int(np.floor(x))
    fy, fx = float(y - sy), float(x - sx)
    return sy, sx, ((1 - fx) * (1 - fy), fx * (1 - fy), (1 - fx) * fy,
                    fx * fy)


def patches(obj, scan, pw):
    """(N, pw, pw): the bilinear patch of obj (H, W) at every position; a tap
    outside the object counts as zero."""
    obj = np.pad(np.asarray(obj, np.complex128), ((0, 1), (0, 1)))
    out = np.empty((len(scan), pw, pw), np.complex128)
    for n, pos in enumerate(scan):
        sy, sx, (w00, w01, w10, w11) = _corner(pos)
        out[n] = (w00 * obj[sy:sy + pw, sx:sx + pw]
                  + w01 * obj[sy:sy + pw, sx + 1:sx + pw + 1]
                  + w10 * obj[sy + 1:sy + pw + 1, sx:sx + pw]
                  + w11 * obj[sy + 1:sy + pw + 1, sx + 1:sx + pw + 1])
    return out


def scatter(values, scan, shape):
    """The adjoint of `patches`: (H, W) sum of the (N, pw, pw) values."""
    H, W = shape
    pw = values.shape[-1]
    out = np.zeros((H + 1, W + 1), values.dtype)
    for n, pos in enumerate(scan):
        sy, sx, (w00, w01, w10, w11) = _corner(pos)
        out[sy:sy + pw, sx:sx + pw] += w00 * values[n]
        out[sy:sy + pw, sx + 1:sx + pw + 1] += w01 * values[n]
        out[sy + 1:sy + pw + 1, sx:sx + pw] += w10 * values[n]
        out[sy + 1:sy + pw + 1, sx + 1:sx + pw + 1] += w11 * values[n]
    return out[:H, :W]


def pad(x, det):
    """The (…, pw, pw) planes centred in (…, det, det) ones, as
    tike_conv_fwd places them."""
    pw = x.shape[-1]
    p = (det - pw) // 2
    out = np.zeros((*x.shape[:-2], det, det), x.dtype)
    out[..., p:p + pw, p:p + pw] = x
    return out


def crop(x, pw):
    p = (x.shape[-1] - pw) // 2
    return x[..., p:p + pw, p:p + pw]


def products(obj, scan, probe):
    """P_s O_n: (N, S, pw, pw); probe (S, pw, pw)."""
    return patches(obj, scan, probe.shape[-1])[:, None] * probe[None]


def reflect(obj, scan, probe, waves, relaxation, det):
    """tike_dm_reflect: pad((1 + a) P O - a waves); waves None: pad(P O)."""
    po = products(obj, scan, probe)
    if waves is None:
        return pad(po, det)
    return pad((1 + relaxation) * po - relaxation * waves, det)


def update(waves, chi, obj, scan, probe, relaxation):
    """tike_dm_update: (the new waves, change (N))."""
    po = products(obj, scan, probe)
    new = ((1 - relaxation) * waves + relaxation * po
           + crop(chi, probe.shape[-1]))
    return new, np.sum(np.abs(new - waves)**2, axis=(1, 2, 3))


def project(near, data, mask=None, unmeasured=1.0):
    """The middle of the exit-wave step (norm='ortho'): (chi (N, S, det, det)
    before the crop, cost (N)).  NaN counts under the mask are never read."""
    far = np.fft.fft2(near, norm="ortho")
    inten = np.sum(np.abs(far)**2, axis=1)
    if mask is None:
        mask = np.ones(near.shape[-2:], bool)
    d = np.where(mask, data, 0.0).astype(np.float64)
    factor = np.where(mask, np.sqrt(d) / (np.sqrt(inten) + 1e-9) - 1.0,
                      unmeasured - 1.0)
    cost = (np.sum(np.where(mask, (np.sqrt(inten) - np.sqrt(d))**2, 0.0),
                   axis=(-2, -1)) / np.count_nonzero(mask))
    return np.fft.ifft2(far * factor[:, None], norm="ortho"), cost


def exit_wave_step(obj, probe, waves, scan, data, *, relaxation=1.0,
                   mask=None, unmeasured=1.0):
    """Step 1 for the given positions: (new waves, cost (N))."""
    det = data.shape[-1]
    chi, cost = project(reflect(obj, scan, probe, waves, relaxation, det),
                        data, mask, unmeasured)
    return update(waves, chi, obj, scan, probe, relaxation)[0], cost


def epoch(obj, probe, waves, scan, data, *, relaxation=1.0, overlap_iter=2,
          object_inertia=1e-4, probe_inertia=1e-9, mask=None, unmeasured=1.0,
          recover_psi=True, recover_probe=True, batches=None):
    """One epoch: obj (H, W), probe (S, pw, pw), waves (N, S, pw, pw) -> (obj,
    probe, waves, cost).  batches: lists of positions that partition the
    work; every sum over the positions is formed batch by batch."""
    N = len(scan)
    pw = probe.shape[-1]
    if batches is None:
        batches = [np.arange(N)]
    new = np.empty_like(waves)
    cost = 0.0
    for b in batches:
        if len(b) == 0:
            continue
        new[b], c = exit_wave_step(obj, probe, waves[b], scan[b], data[b],
                                   relaxation=relaxation, mask=mask,
                                   unmeasured=unmeasured)
        cost += np.sum(c)
    waves = new
    for _ in range(overlap_iter):
        if recover_psi:
            num = sum(scatter(np.sum(np.conj(probe)[None] * waves[b], axis=1),
                              scan[b], obj.shape) for b in batches if len(b))
            amp = np.sum(np.abs(probe)**2, axis=0)
            den = sum(scatter(np.repeat(amp[None], len(b), 0), scan[b],
                              obj.shape) for b in batches if len(b))
            c = object_inertia * den.max()
            obj = (c * obj + num) / (c + den)
        if recover_probe:
            num = sum(np.sum(np.conj(patches(obj, scan[b], pw))[:, None]
                             * waves[b], axis=0) for b in batches if len(b))
            den = sum(np.sum(np.abs(patches(obj, scan[b], pw))**2, axis=0)
                      for b in batches if len(b))
            c = probe_inertia * den.max()
            probe = (c * probe + num) / (c + den)
    return obj, probe, waves, cost / N


def binomial(x):
    """One pass of the separable (1, 2, 1) / 4 filter over the last two axes,
    edges repeated."""
    for axis in (-2, -1):
        p = np.concatenate([np.take(x, [0], axis), x, np.take(x, [-1], axis)],
                           axis)
        n = x.shape[axis]
        x = (np.take(p, range(0, n), axis) + 2 * np.take(p, range(1, n + 1),
                                                         axis)
             + np.take(p, range(2, n + 2), axis)) / 4
    return x


def model_cost(obj, probe, scan, data, mask=None):
    """The cost of the other solvers: the Fourier error of P O itself."""
    return float(np.mean(project(reflect(obj, scan, probe, None, 1.0,
                                         data.shape[-1]), data, mask)[1]))


def problem(det=32, pw=32, S=1, grid=(4, 4), step=5.0, seed=0, pad_obj=2,
            amplitude=100.0, integer=False, smooth=0):
    """A small synthetic problem: (obj (H, W), probe (S, pw, pw), scan (N, 2)
    float32, data (N, det, det) noise-free intensities of the model).
    amplitude: the peak of the first probe mode (100: some 1e6 counts per
    pattern); integer: positions without a fractional part; smooth: passes
    of a 3 x 3 binomial filter over the (otherwise white) object."""
    rng = np.random.default_rng(seed)
    ij = np.stack(np.meshgrid(np.arange(grid[0]), np.arange(grid[1]),
                              indexing="ij"), -1).reshape(-1, 2)
    jitter = rng.random((len(ij), 2))
    scan = (1.0 + pad_obj + step * ij
            + (np.round(2 * jitter) if integer else jitter)).astype(np.float32)
    H = int(np.ceil(scan.max())) + pw + 2 + pad_obj
    obj = ((0.6 + 0.4 * rng.random((H, H)))
           * np.exp(1j * np.pi * (rng.random((H, H)) - 0.5)))
    for _ in range(smooth):
        obj = binomial(obj)
    y =(np.arange(pw) - (pw - 1) / 2) / pw
    r2 = y[:, None]**2 + y[None, :]**2
    probe = np.stack([
        np.exp(-r2 / (2 * 0.18**2)) * np.exp(1j * 8 * r2 * (m + 1))
        * (y[None, :] if m % 2 else 1.0) * (y[:, None] if m // 2 else 1.0)
        * amplitude * (4.0**m) / (m + 1) for m in range(S)])
    near = reflect(obj, scan, probe, None, 1.0, det)
    data = np.sum(np.abs(np.fft.fft2(near, norm="ortho"))**2, axis=1)
    return obj, probe, scan, data
