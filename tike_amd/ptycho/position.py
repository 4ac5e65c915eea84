"""Scan-position helpers and position correction
(reference src/tike/ptycho/position.py).

On the accelerated path: ``check_allowed_positions``, ``PositionOptions``
(state of the position correction inside ``lstsq_grad``), the affine
regularisation of updated positions (host-side, a few hundred flops per epoch)
and the Gaussian-derivative taps handed to ``tike_position_sums``.
"""
from __future__ import annotations

import dataclasses

import numpy as np
import torch

from .. import _arrays as A
from .. import linalg, precision
from .._lib import check, lib
from .. import random as trandom


def check_allowed_positions(scan, psi, probe_shape):
    """Raise ValueError unless every patch lies inside the object with one
    pixel to spare: 1 <= floor(scan) <= psi.shape - probe_shape - 1 on both
    axes (the kernels read the pixel after a patch's last one; the rule and
    the message of the reference, position.py:600-628)."""
    corner = np.floor(A.to_host(scan))
    lowest, highest = corner.min(axis=-2), corner.max(axis=-2)
    room = np.subtract(psi.shape[-2:], probe_shape[-2:]) - 1
    if np.any(lowest[:2] < 1) or np.any(highest[:2] > room):
        raise ValueError(
            "Scan positions must be >= 1 and "
            "scan positions + 1 + probe.shape must be <= psi.shape. "
            "psi may be too small or the scan positions may be scaled wrong. "
            f"The span of scan is {lowest} to {highest}, and "
            f"the shape of psi is {psi.shape}.")


# ------------------------------------------------------------------ transform
@dataclasses.dataclass
class AffineTransform:
    """A 2-D affine transformation scale @ shear @ rotate + translate
    (position.py:137-249)."""

    scale0: float = 1.0
    scale1: float = 1.0
    shear1: float = 0.0
    angle: float = 0.0
    t0: float = 0.0
    t1: float = 0.0

    def resample(self, factor: float) -> "AffineTransform":
        return AffineTransform(self.scale0, self.scale1, self.shear1,
                               self.angle, self.t0 * factor, self.t1 * factor)

    @classmethod
    def frombuffer(cls, buffer) -> "AffineTransform":
        return AffineTransform(*buffer)

    def asbuffer(self) -> np.ndarray:
        return np.array(self.astuple())

    @classmethod
    def fromarray(cls, T) -> "AffineTransform":
        """The transform whose `asarray()` (and, for a 3 x 2 input,
        translation) is T.  The rows of the 2 x 2 part are orthogonalised in
        order (a QR factorisation of its transpose with a positive diagonal:
        the decomposition of Graphics Gems II 7.1 that the reference uses,
        position.py:166-193): the diagonal holds the scales, the off-diagonal
        term over scale1 the shear, and the angle is arccos of the first
        component of the first unit row.  A rank-deficient matrix gives the
        identity transform."""
        T = np.asarray(T, dtype=np.float64)
        basis, factor = np.linalg.qr(T[:2, :2].T)
        flip = np.where(np.diag(factor) < 0, -1.0, 1.0)
        basis, factor = basis * flip, factor * flip[:, None]
        tiny = 1e-12 * np.abs(factor).max()  # rows on one line: no rotation
        if not (factor[0, 0] > tiny and factor[1, 1] > tiny):
            return cls()
        shift = T[2] if len(T) > 2 else (0.0, 0.0)
        return cls(scale0=float(factor[0, 0]), scale1=float(factor[1, 1]),
                   shear1=float(factor[0, 1] / factor[1, 1]),
                   angle=float(np.arccos(np.clip(basis[0, 0], -1.0, 1.0))),
                   t0=float(shift[0]), t1=float(shift[1]))

    def asarray(self, xp=np) -> np.ndarray:
        """The 2 x 2 matrix diag(scale0, scale1) @ [[1, 0], [shear1, 1]] @
        rotation(angle), multiplied out (position.py:195-220); row vectors
        are transformed as x @ matrix."""
        c, s = np.cos(self.angle), np.sin(self.angle)
        sheared = (self.shear1 * c + s, c - self.shear1 * s)
        return np.array([[self.scale0 * c, -self.scale0 * s],
                         [self.scale1 * sheared[0], self.scale1 * sheared[1]]],
                        dtype=precision.floating)

    @classmethod
    def fit(cls, positions0, positions1, weights=None) -> "AffineTransform":
        """Least-squares transform with positions0 -> positions1 (rows may be
        weighted): the normal equations of [positions0, 1] @ X = positions1,
        solved in the positions' own precision and the reference's evaluation
        order (see `linalg.lstsq`).  Positions on one line make them singular:
        the identity transform is returned."""
        ones = np.ones_like(positions0[..., :1])
        try:
            return cls.fromarray(
                linalg.lstsq(np.concatenate([positions0, ones], axis=-1),
                             positions1, weights))
        except np.linalg.LinAlgError:
            return cls()

    def asarray3(self, xp=np) -> np.ndarray:
        T = np.empty((3, 2), dtype=precision.floating)
        T[2] = (self.t0, self.t1)
        T[:2, :2] = self.asarray()
        return T

    def astuple(self) -> tuple:
        return (self.scale0, self.scale1, self.shear1, self.angle, self.t0,
                self.t1)

    def __call__(self, x, gpu=False, shift=True):
        if A.is_device(x):
            M = torch.as_tensor(self.asarray(), device=x.device, dtype=x.dtype)
            r = x @ M
            if shift:
                r = r + torch.tensor((self.t0, self.t1), device=x.device,
                                     dtype=x.dtype)
            return r
        r = x @ self.asarray()
        if shift:
            r = r + np.array((self.t0, self.t1))
        return r


def estimate_global_transformation(positions0, positions1, weights=None,
                                   transform=None):
    """The affine transformation that maps positions0 onto positions1 in the
    (weighted) least-squares sense (`AffineTransform.fit`) and the residual
    norm over these positions (position.py:252-270).  Host arrays."""
    fitted = AffineTransform.fit(positions0, positions1, weights)
    # (the Frobenius norm written out: numpy hands the flattened float64
    # residual to BLAS ddot, whose threaded start-up costs 10-35 ms per call
    # on many-core hosts -- 40 calls per RANSAC fit, 0.5 s per epoch of a
    # position-correcting run of 10 000 positions, three GPU epochs' worth)
    residual = fitted(positions0) - positions1
    return fitted, np.sqrt(np.sum(np.square(residual)))


def ransac_subsets(n, min_sample=4, max_iter=20):
    """The random subsets of one RANSAC fit over n positions
    (position.py:296-300), from the library's generator."""
    return trandom.randomizer_np.choice(a=n, size=(max_iter, min_sample),
                                        replace=True)


def _consensus_fits(positions0, positions1, weights, subsets, max_error,
                    min_consensus):
    """(fitness, model) of every random subset whose rough fit explains at
    least `min_consensus` of all positions to within `max_error` pixels; the
    model is refitted on those inliers."""
    for rows in subsets:
        rough, _ = estimate_global_transformation(positions0[rows],
                                                  positions1[rows], weights)
        miss = np.linalg.norm(rough(positions0) - positions1, axis=-1)
        inliers = miss <= max_error
        if inliers.mean() >= min_consensus:
            model, fitness = estimate_global_transformation(
                positions0[inliers], positions1[inliers], weights)
            yield fitness, model


def estimate_global_transformation_ransac(positions0, positions1, weights=None,
                                          transform=None, min_sample=4,
                                          max_error=32, min_consensus=0.75,
                                          max_iter=20, subsets=None):
    """RANSAC estimate of the global affine transformation
    (position.py:273-327): the consensus fit with the smallest residual (the
    first of equals), or `transform` unchanged with fitness inf when no
    subset reaches consensus.  The subsets come from ``tike_amd.random.
    randomizer_np`` exactly as the reference draws them (`subsets`: drawn
    earlier by `ransac_subsets`, for a fit that is carried out later)."""
    if subsets is None:
        subsets = ransac_subsets(len(positions0), min_sample, max_iter)
    best = (np.inf, AffineTransform() if transform is None else transform)
    for fitness, model in _consensus_fits(positions0, positions1, weights,
                                          subsets, max_error, min_consensus):
        if fitness < best[0]:
            best = (fitness, model)
    return best[1], best[0]


def gaussian_derivative_taps(sigma=0.333, truncate=6.0):
    """Taps t[d], d = -r..r, of ``gaussian_gradient`` (position.py:779-810):
    g[i] = sum_d t[d] x[i + d], i.e. scipy's ``gaussian_filter1d(-x, sigma,
    order=1)``: a normalised Gaussian times -d / sigma^2, reversed."""
    r = int(truncate * float(sigma) + 0.5)
    d = np.arange(-r, r + 1)
    phi = np.exp(-0.5 / (sigma * sigma) * d**2)
    phi = phi / phi.sum()
    return (-(d / (sigma * sigma)) * phi).astype(np.float32), r


def gaussian_gradient(x, sigma=0.333):
    """First-order Gaussian derivatives of `x` along its last two axes
    (position.py:779-810): ``gaussian_filter1d(-x, sigma, order=1,
    mode='nearest', truncate=6)`` per axis.  The solver applies the same taps
    inside ``tike_position_sums``; this is the array-level form."""
    t, was_numpy = (x, False) if isinstance(x, torch.Tensor) else (
        torch.from_numpy(np.ascontiguousarray(x)), True)
    taps, r = gaussian_derivative_taps(sigma)
    taps = torch.from_numpy(taps).to(t.device)
    out = []
    for axis in (-2, -1):
        n = t.shape[axis]
        g = torch.zeros_like(t)
        for d in range(-r, r + 1):
            idx = torch.clamp(torch.arange(n, device=t.device) + d, 0, n - 1)
            g = g + taps[d + r] * t.index_select(axis % t.ndim, idx)
        out.append(g.cpu().numpy() if was_numpy else g)
    return tuple(out)


# -------------------------------------------------------------------- options
@dataclasses.dataclass
class PositionOptions:
    """Data and settings of the position correction (position.py:330-598)."""

    initial_scan: np.ndarray
    use_adaptive_moment: bool = False
    vdecay: float = 0.999
    mdecay: float = 0.9
    use_position_regularization: bool = False
    update_magnitude_limit: float = 0
    transform: AffineTransform = dataclasses.field(
        default_factory=AffineTransform)
    origin: np.ndarray = dataclasses.field(
        default_factory=lambda: np.zeros(2))
    confidence: np.ndarray = None
    update_start: int = 0
    _momentum: np.ndarray = dataclasses.field(init=False, default=None)

    def __post_init__(self):
        """float32 positions; unit confidence and zero ADAM moments unless
        given.  Host (NumPy) and device (torch) arrays alike."""
        scan = self.initial_scan
        on_device = A.is_device(scan)
        if on_device:
            scan = scan.to(torch.float32)
            fill = lambda value, *shape: torch.full(  # noqa: E731
                shape, value, dtype=torch.float32, device=scan.device)
        else:
            scan = np.asarray(scan).astype(precision.floating)
            fill = lambda value, *shape: np.full(  # noqa: E731
                shape, value, dtype=precision.floating)
        self.initial_scan = scan
        if self.confidence is None:
            self.confidence = fill(1.0, *scan.shape)
        if self.use_adaptive_moment:
            self._momentum = fill(0.0, *scan.shape[:-1], 4)

    def _like(self, initial_scan, confidence, momentum=None, **changes):
        """A copy of the settings around other per-position arrays
        (momentum None: start from zero moments)."""
        settings = {
            f.name: getattr(self, f.name)
            for f in dataclasses.fields(self)
            if f.init and f.name not in ("initial_scan", "confidence")
        }
        settings.update(changes)
        new = PositionOptions(initial_scan, confidence=confidence, **settings)
        if self.use_adaptive_moment and momentum is not None:
            new._momentum = momentum
        return new

    def split(self, indices) -> "PositionOptions":
        """The options of the positions `indices` only (position.py:432-447)."""
        rows = lambda v: None if v is None else v[..., indices, :]  # noqa: E731
        return self._like(rows(self.initial_scan), rows(self.confidence),
                          rows(self._momentum))

    def insert(self, other, indices):
        """Write `other`'s per-position arrays into rows `indices` of this
        one's (the inverse of `split`, position.py:449-456)."""
        for name in ("initial_scan", "confidence", "_momentum"):
            mine, theirs = getattr(self, name), getattr(other, name)
            if mine is not None and theirs is not None:
                mine[..., indices, :] = theirs
        return self

    @staticmethod
    def join(x, reorder):
        """Concatenate per-worker options and undo the ordering
        (position.py:458-489)."""
        if None in x:
            return None
        cat = lambda parts: np.concatenate(parts, axis=0)[reorder]
        return x[0]._like(
            cat([e.initial_scan for e in x]),
            None if x[0].confidence is None else
            cat([e.confidence for e in x]),
            None if x[0]._momentum is None else cat([e._momentum for e in x]))

    def copy_to_device(self):
        d = lambda v: None if v is None else A.to_device(v, np.float32)
        return self._like(d(self.initial_scan), d(self.confidence),
                          d(self._momentum))

    def copy_to_host(self):
        h = lambda v: None if v is None else A.to_host(v)
        return self._like(h(self.initial_scan), h(self.confidence),
                          h(self._momentum))

    def resample(self, factor: float) -> "PositionOptions":
        """The options on a grid `factor` times finer: lengths scale, the
        ADAM moments restart from zero (position.py:534-553)."""
        return self._like(self.initial_scan * factor, self.confidence,
                          transform=self.transform.resample(factor),
                          origin=self.origin * factor)

    # second (v) and first (m) moments of ADAM, packed as the reference does
    @property
    def v(self):
        return self._momentum[..., 0:2]

    @v.setter
    def v(self, x):
        self._momentum[..., 0:2] = x

    @property
    def m(self):
        return self._momentum[..., 2:4]

    @m.setter
    def m(self, x):
        self._momentum[..., 2:4] = x


def affine_position_regularization(updated, position_options, max_error=32,
                                   *, positions0=None, positions1=None,
                                   relax=0.9):
    """Refresh `position_options.transform` -- the global affine map from the
    initial to the updated positions (RANSAC, about `origin`) -- and, when
    `use_position_regularization` is set, move every updated position the
    fraction `relax` of the way to where that map puts its initial position
    (translation excluded) (position.py:716-776).

    `updated` / `position_options.initial_scan` are this rank's positions;
    `positions0` / `positions1` are the host arrays the fit uses (all
    positions of the job; default: this rank's own).
    """
    if positions0 is None:
        positions0 = A.to_host(position_options.initial_scan)
        positions1 = A.to_host(updated)
    origin = A.to_host(position_options.origin)
    position_options.transform = estimate_global_transformation_ransac(
        positions0 - origin, positions1 - origin,
        transform=position_options.transform, max_error=max_error)[0]
    if not position_options.use_position_regularization:
        return updated, position_options
    target = position_options.transform(position_options.initial_scan,
                                        shift=False)
    pulled = updated * (1 - relax) + relax * target
    pulled = (pulled.to(torch.float32) if A.is_device(pulled) else
              pulled.astype(precision.floating))
    return pulled, position_options


# ------------------------------------------- gradient-of-intensity refinement
# share of the free device memory the stacked far planes of one chunk may take
# (the forward operators keep an intermediate of the same size next to them)
PD_WORKSPACE_SHARE = 0.25
# positions per chunk instead of the memory rule (tests)
PD_CHUNK_OVERRIDE = None


def _pd_chunk(S, det, slices, device):
    """Positions per chunk of `position_pd_shifts`: the (3, n, S, det, det)
    complex64 workspace within `PD_WORKSPACE_SHARE` of the free memory (a
    third of that for several slices, whose composition holds the waves
    between the slices as well)."""
    if PD_CHUNK_OVERRIDE:
        return int(PD_CHUNK_OVERRIDE)
    budget = PD_WORKSPACE_SHARE * torch.cuda.mem_get_info(device)[0]
    if slices > 1:
        budget /= 3
    return max(1, int(budget) // (3 * 8 * S * det * det))


def _pd_far_planes(operator, psi, probe, stacked, eigen_probe, weights, out):
    """Far planes (3n, 1, S, det, det) of the stacked positions: the fused
    forward into `out` for one slice, the slice-by-slice `operator.fwd`
    otherwise."""
    repeat3 = lambda t: None if t is None else t.repeat(  # noqa: E731
        3, *([1] * (t.ndim - 1)))
    if psi.shape[0] > 1:
        if weights is not None:
            from .probe import get_varying_probe
            probe = get_varying_probe(probe, eigen_probe, repeat3(weights))
        elif probe.shape[0] != 1:
            probe = repeat3(probe)
        return operator.fwd(probe=probe.contiguous(), scan=stacked,
                            psi=psi).contiguous()
    if probe.shape[0] != 1:
        probe = repeat3(probe)
    return operator.fwd_device(probe, stacked, psi, eigen_probe,
                               repeat3(weights), out=out)


def _pd_sums_device(operator, data, psi, probe, scan, dx, eigen_probe,
                    eigen_weights):
    """((N, 5) sums, (N) gaussian costs) of `tike_position_pd_sums` over all
    positions, chunk by chunk.  Device tensors; `data` is anything whose row
    slices are device tensors of float32 or uint16."""
    N, S, det = scan.shape[0], probe.shape[-3], operator.detector_shape
    dev = psi.device
    sums = torch.empty((N, 5), dtype=torch.float32, device=dev)
    costs = torch.empty((N,), dtype=torch.float32, device=dev)
    if N == 0:
        return sums, costs
    chunk = min(N, _pd_chunk(S, det, psi.shape[0], dev))
    work = None
    if psi.shape[0] == 1:
        work = torch.empty((3 * chunk, 1, S, det, det), dtype=torch.complex64,
                           device=dev)
    # rows of `scan` moved along the columns, then along the rows: the
    # reference's "dx" and "dy" (position.py:665-676)
    moves = torch.tensor([[0.0, 0.0], [0.0, dx], [dx, 0.0]],
                         dtype=torch.float32, device=dev)
    for lo in range(0, N, chunk):
        hi = min(N, lo + chunk)
        n = hi - lo
        stacked = (scan[lo:hi][None] + moves[:, None]).reshape(3 * n, 2)
        per = probe if probe.shape[0] == 1 else probe[lo:hi]
        w = None if eigen_weights is None else eigen_weights[lo:hi]
        far = _pd_far_planes(operator, psi, per, stacked.contiguous(),
                             eigen_probe, w,
                             None if work is None else work[:3 * n])
        rows = data[lo:hi]
        if rows.dtype not in (torch.float32, torch.uint16):
            rows = rows.to(torch.float32)
        rows = rows.contiguous()
        check(
            lib.tike_position_pd_sums(
                A.ptr(far[:n]), A.ptr(far[n:2 * n]), A.ptr(far[2 * n:]),
                A.ptr(rows), int(rows.dtype == torch.uint16), 1.0 / dx,
                A.ptr(sums[lo:hi]), A.ptr(costs[lo:hi]), n, S, det * det,
                A.stream_ptr()), "position_pd_shifts")
    return sums, costs


def _pd_solve(sums):
    """The least-squares shift of position.py:685-689 from the normal
    equations [[aa, ab], [ab, bb]] g = (ar, br) of every position at once
    (Cramer's rule in float64 on the device); column 0 goes with scan
    column 0."""
    aa, ab, bb, ar, br = sums.to(torch.float64).unbind(-1)
    det = aa * bb - ab * ab
    return torch.stack(((bb * ar - ab * br) / det, (aa * br - ab * ar) / det),
                       dim=-1).to(torch.float32)


def _pd_data_on_device(data):
    if A.is_device(data):
        return data if data.dtype == torch.uint16 else A.to_device(
            data, np.float32)
    data = np.asarray(data)
    if A.is_small_integer(data.dtype):
        return A.data_to_device(data)
    return A.to_device(data, np.float32)


def position_pd_shifts(operator, data, psi, probe, scan, dx=-1.0, *,
                       eigen_probe=None, eigen_weights=None, costs=False):
    """Shift estimate `grad` (N, 2) float32 of the gradient-of-intensity
    position refinement (Dwivedi et al. 2018; position.py:654-689): per
    position the least-squares solution of [dI/dy, dI/dx] g = data - I over
    the detector pixels, the derivatives being one-sided differences of the
    far plane over `dx` pixels, summed over the probe modes.  Column 0 of
    `grad` belongs to scan column 0; the refined position is scan - step *
    grad.  `costs=True` also returns the gaussian cost of every pattern at
    `scan`.

    Needs the forward model and the data only, so it runs next to any solver
    and on objects of several slices.  probe (1|N, 1, S, pw, pw); with
    `eigen_weights` (N, C + 1, S) the varying probe of probe.py:272-303.
    Host arrays or device tensors; the result is of `scan`'s kind.

    Per chunk: ONE forward over the stacked positions [scan; scan + (0, dx);
    scan + (dx, 0)] and one `tike_position_pd_sums`; the 2 x 2 systems of all
    positions are solved on the device.  The displaced positions go through
    the forward entry `Ptycho.fwd` uses, with its rule at the border: keep
    `scan` inside `check_allowed_positions`."""
    kind = scan
    if dx == 0:
        raise ValueError("dx must not be zero")
    on = lambda x, dtype: None if x is None else A.to_device(x, dtype)  # noqa: E731
    sums, each = _pd_sums_device(
        operator, _pd_data_on_device(data), on(psi, np.complex64),
        on(probe, np.complex64), on(scan, np.float32), float(dx),
        on(eigen_probe, np.complex64), on(eigen_weights, np.float32))
    grad = A.like_input(_pd_solve(sums), kind)
    return (grad, A.like_input(each, kind)) if costs else grad


def _pd_moved(scan, grad, step, before=None, after=None, count=None):
    """scan - step * grad, put back so that the mean position stays
    (position.py:694-698); float64 until the last rounding.  before / after /
    count: the position sums and the number of positions when they are not
    this array's own (several ranks)."""
    old = scan.to(torch.float64)
    new = old - step * grad.to(torch.float64)
    if before is None:
        before, after, count = old.sum(0), new.sum(0), max(1, old.shape[0])
    return (new + (before - after) / count).to(torch.float32)


def _pd_cost_sum(operator, data, psi, probe, scan, eigen_probe=None,
                 eigen_weights=None):
    """Sum over the positions of the gaussian per-pattern cost (0-d float64
    device tensor): `operator.cost(model="gaussian")` times N, chunk by
    chunk, for one or several slices."""
    from .ptycho import _intensity_chunks
    total = torch.zeros((), dtype=torch.float64, device=psi.device)
    for lo, hi, inten in _intensity_chunks(operator, psi, scan, probe,
                                           eigen_probe, eigen_weights):
        each = torch.empty((hi - lo,), dtype=torch.float32, device=psi.device)
        npix = inten.shape[-2] * inten.shape[-1]
        check(
            lib.tike_cost_each_pattern(
                A.ptr(A.data_f32(data, lo, hi).contiguous()), A.ptr(inten),
                A.ptr(each), hi - lo, npix, 0, A.stream_ptr()),
            "update_positions_pd (cost)")
        total += each.sum(dtype=torch.float64)
    return total


def update_positions_pd(operator, data, psi, probe, scan, dx=-1, step=0.05):
    """One step of the gradient-of-intensity position refinement
    (position.py:631-703): (scan - step * position_pd_shifts(...), moved back
    so that the mean position is unchanged; the gaussian cost there as a
    Python float).  ValueError from `check_allowed_positions` when a refined
    position leaves the field of view.

    A coarse estimator for a few calls, not a solver: with a one-pixel
    difference three steps of 0.5 bring the position error to 0.4 - 0.7 of
    its start on smooth test objects, after which the finite difference
    stalls and the error drifts up again.  It suits the start of a run whose
    positions are off by a good fraction of a pixel, e.g. ahead of `cgrad`.

    The cost is `operator.cost(..., model="gaussian")` at the new positions.
    (The reference calls `cost` without the keyword-only `model` and raises
    TypeError on that statement at this snapshot; everything before it is
    what this function computes.)"""
    kind = scan
    if dx == 0:
        raise ValueError("dx must not be zero")
    data = _pd_data_on_device(data)
    psi = A.to_device(psi, np.complex64)
    probe = A.to_device(probe, np.complex64)
    scan = A.to_device(scan, np.float32)
    sums, _ = _pd_sums_device(operator, data, psi, probe, scan, float(dx),
                              None, None)
    moved = _pd_moved(scan, _pd_solve(sums), step)
    check_allowed_positions(moved, psi, probe.shape)
    cost = _pd_cost_sum(operator, data, psi, probe, moved) / max(
        1, moved.shape[0])
    return A.like_input(moved, kind), float(cost.item())
