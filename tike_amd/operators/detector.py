"""What lies between the sample's plane and the measured counts: ONE value,
`Detector`, that every entry builds once and passes down (no reference
counterpart).

The kinds (`Detector.kind`) and what each carries in `value`:

* "far": every frame is the far-field intensity summed over its `fly`
  positions and the modes; nothing carried.
* "binned": a far plane `binning` = B times finer than the counts, a measured
  pixel the sum over its B x B far-plane pixels; nothing besides B.
* "background": the far-field intensity plus b (det, det) float32 >= 0.
* "blur": the far-field intensity convolved, cyclically, with K (k, k)
  float32, k in (3, 5, 7).
* "nearfield": |IFFT2(H FFT2(patch x probe))|^2, H (det, det) complex64.

`build` holds the table of what goes with what, once, for the four entries
(`simulate`, `autograd.cost`, `Ptycho.cost` / `_compute_intensity`,
`Reconstruction`), each of which words a refusal its own way (`Naming`).  The
checks of the values b, K and H stand here once per form -- host arrays
(`checked_background`, `checked_kernel`, `checked_propagator`), the device
tensors of `autograd.cost` (`device_value`), whatever `Ptycho.cost` is given
(`resident_value`).  `farplane_step` is what differs between the far-field
kinds in a chunk of whole frames, `cost_factor` the same for the tables of
`autograd.cost`, `intensity` for the entries that only want the frames.
"""
from typing import Any, NamedTuple, Optional

import numpy as np
import torch

from .. import _arrays as A
from .._lib import check, lib
from . import nearfield as NF

BLUR_WIDTHS = (3, 5, 7)


class Detector(NamedTuple):
    kind: str = "far"
    binning: int = 1
    value: Any = None  # b, K or H

    def width(self, det):
        """The width of the counts behind a plane `det` wide."""
        return det // self.binning


def far_field(binning=1):
    """The far-field detector with `binning` far-plane pixels per count."""
    return Detector("binned" if binning > 1 else "far", binning)


class Model(NamedTuple):
    """The noise model of a step, as far as `farplane_step` reads it (cgrad's
    `_CostModel` has the same three)."""
    model: int = 0
    nmeasured: Optional[int] = None  # None: every pixel
    mask: Optional[torch.Tensor] = None


class Naming(NamedTuple):
    """How an entry words a refusal: its exception, its sentence about `a`
    with `b`, and whether it names the models as `reconstruct`'s keywords."""
    error: type
    text: str
    options: bool = False


SIMULATE = Naming(NotImplementedError, "{a} with {b} is not implemented")
OPERATOR = Naming(ValueError, "{a} together with {b} is not supported")
RECONSTRUCTION = Naming(
    NotImplementedError, "{a} with {b}: this combination is not implemented",
    True)


def entry(name):
    """The naming of `autograd`'s function `name`: `SIMULATE` behind it."""
    return Naming(NotImplementedError, f"{name}: {SIMULATE.text}")


# what a model refuses, in the order asked; binning alone refuses nothing here
_REFUSES = dict(
    nearfield=("binning", "background", "blur", "slices", "eigen", "window"),
    blur=("binning", "background", "slices", "eigen"),
    background=("binning", "slices", "eigen"))


def refuse(kind, naming, *, binning=1, background=False, blur=False, slices=1,
           eigen=False, window=None, det=None):
    """Raise `naming.error` for the first thing the model `kind` cannot be
    combined with.  window: the probe's, held against `det` in the near
    field (None: not asked)."""
    models = "{}_options" if naming.options else "a {}"
    has = dict(
        binning=(binning > 1, f"binning={binning}"),
        background=(background, models.format("background")),
        blur=(blur, models.format("blur")),
        slices=(slices > 1, f"several slices (psi.shape[0] = {slices})"),
        eigen=(eigen, "eigen probes"),
        window=(window is not None and window != det,
                f"probe window {window} != detector {det}"))
    for other in _REFUSES.get(kind, ()):
        if has[other][0]:
            raise naming.error(naming.text.format(
                a=kind + "_options" * naming.options, b=has[other][1]))


def build(naming, det, *, binning=1, background=None, blur=None,
          nearfield=None, slices=1, eigen=False, window=None):
    """The `Detector` of an entry's keywords after the refusals of every
    model given; b, K or H as given: the entry checks it by its own form."""
    given = dict(nearfield=nearfield, blur=blur, background=background)
    for kind, value in given.items():
        if value is not None:
            refuse(kind, naming, binning=binning,
                   background=background is not None, blur=blur is not None,
                   slices=slices, eigen=eigen, window=window, det=det)
    for kind, value in given.items():  # (at most one is left)
        if value is not None:
            return Detector(kind, 1, value)
    return far_field(binning)


# -- the values ------------------------------------------------------------
def _host(x, what, shape, dtype):
    """x as a host array after validation of its shape -- None: that of a
    blur kernel -- and dtype."""
    x = np.asarray(A.to_host(x) if A.is_device(x) else x)
    if shape is None:
        k = x.shape[-1] if x.ndim else 0
        ok = x.shape == (k, k) and k in BLUR_WIDTHS
        expected = f"(k, k) with k in {BLUR_WIDTHS}"
    else:
        ok, expected = x.shape == shape, f"the detector's {shape}"
    if not ok:
        raise ValueError(f"{what} has shape {x.shape}; expected {expected}")
    if x.dtype != dtype:
        raise ValueError(f"{what} is {x.dtype}; expected {np.dtype(dtype)}")
    return x


def _finite(x, what, sign):
    if not np.all(np.isfinite(x)) or (sign and np.any(x < 0)):
        raise ValueError(f"{what} must be finite" + " and >= 0" * sign)


def checked_background(background, det, what="background"):
    """`background` as a host (det, det) float32 array, finite and >= 0."""
    b = _host(background, what, (det, det), np.float32)
    _finite(b, what, True)
    return b


def checked_kernel(kernel, det, what="blur"):
    """`kernel` as a host (k, k) float32 array of sum 1, after validation of
    its shape, dtype, finiteness and sign."""
    K = _host(kernel, what, None, np.float32)
    if K.shape[-1] > det:
        raise ValueError(
            f"{what} {K.shape} is wider than the detector ({det}, {det})")
    _finite(K, what, True)
    total = float(K.sum(dtype=np.float64))
    if not total > 0:
        raise ValueError(f"{what} must have a positive sum")
    return (K.astype(np.float64) / total).astype(np.float32)


def checked_propagator(propagator, det, what="nearfield"):
    """`propagator` as a host (det, det) complex64 array, after validation of
    its shape, dtype and finiteness."""
    if A.is_device(propagator) and propagator.requires_grad:
        raise ValueError(
            f"{what} that requires a gradient is not supported: the "
            "propagator is used as given")
    H = _host(propagator, what, (det, det), np.complex64)
    _finite(H, what, False)
    return np.ascontiguousarray(H)


def checked(detector, det):
    """`detector` with its b, K or H, host arrays, checked."""
    how = dict(background=checked_background, blur=checked_kernel,
               nearfield=checked_propagator)
    if detector.value is None:
        return detector
    return detector._replace(value=how[detector.kind](detector.value, det))


def _shape_error(kind, shape, det):
    """What is wrong with the shape of a device b, K or H, or None."""
    shape = tuple(shape)
    if kind != "blur":
        return (None if shape == (det, det) else
                f"{kind} must be ({det}, {det}), not {shape}")
    k = shape[-1] if shape else 0
    if shape != (k, k) or k not in BLUR_WIDTHS:
        return f"blur must be (k, k) with k in {BLUR_WIDTHS}, not {shape}"
    if k > det:
        return f"blur {shape} is wider than the detector ({det}, {det})"
    return None


def device_value(name, kind, x, det):
    """b, K or H of `autograd`'s function `name`, a device tensor, detached
    and contiguous after validation of its type, dtype, shape and device."""
    want = torch.complex64 if kind == "nearfield" else torch.float32
    if isinstance(x, torch.Tensor) and kind == "nearfield" and x.requires_grad:
        raise NotImplementedError(
            f"{name}: nearfield that requires a gradient is not implemented: "
            "the propagator is used as given")
    if not isinstance(x, torch.Tensor):
        raise TypeError(
            f"{name}: {kind} must be a torch device tensor, not "
            f"{type(x).__name__}")
    if x.dtype != want:
        raise TypeError(f"{name}: {kind} must be {want}, not {x.dtype}")
    wrong = _shape_error(kind, x.shape, det)
    if wrong:
        raise ValueError(f"{name}: {wrong}")
    if x.device.type != "cuda":
        raise TypeError(
            f"{name}: {kind} lives on {x.device}; tike_amd runs on the GPU "
            "only and there is no CPU fallback")
    return x.detach().contiguous()


def resident_value(detector, det):
    """`detector` with its b, K or H on the device, used as given, after
    validation of its shape (`Ptycho.cost`, `_compute_intensity`: host arrays
    or device tensors)."""
    kind, x = detector.kind, detector.value
    if x is None:
        return detector
    if kind == "nearfield":
        return detector._replace(value=NF.device_propagator(x, det))
    x = A.to_device(x, np.float32).contiguous()
    wrong = _shape_error(kind, x.shape, det)
    if wrong:
        raise ValueError(wrong)
    return detector._replace(value=x)


# -- a chunk of whole frames -------------------------------------------------
def upstream_unit(ws, name, n, dev, nmeasured):
    """(n,) float32 of a workspace, every entry num_measured: as the upstream
    of an entry that divides by it, (float)(n * (1 / n)) = 1 -- the factor is
    the unnormalised l' of the other routes."""
    unit = ws.get(name, (n,), torch.float32, dev)
    unit.fill_(float(nmeasured))
    return unit


def workspaces(detector, ws, dev, nframe, det, cm):
    """What `farplane_step(want_grad=...)` of this kind needs from one
    evaluation's set-up, for chunks of at most `nframe` frames.  Blurred: the
    chunk's intensities, its table and the upstream; else None."""
    if detector.kind != "blur":
        return None
    return (ws.get("blur_intensity", (nframe, det, det), torch.float32, dev),
            ws.get("blur_table", (nframe, det, det), torch.float32, dev),
            upstream_unit(ws, "blur_upstream", nframe, dev, cm.nmeasured))


def farplane_step(op, detector, far, counts, fly, cm, *, costs=None,
                  want_grad=False, intensity=None, work=None):
    """The far-plane step of a chunk of whole frames of a far-field kind:
    far (FRAME * fly, 1, S, det, det), counts (FRAME, w, w) float32 or
    uint16, cm the noise model (`Model`).  Writes the frames' costs, into
    `intensity` (FRAME, w, w), if given, the intensities WITHOUT background
    or blur, and with want_grad overwrites `far` by MINUS the unnormalised
    gradient.  One launch, `tike_{fly,binned,background}_farplane_gradient`;
    blurred (work: `workspaces`): `tike_fly_farplane_gradient` only stores
    the intensities (one read of the far plane), `tike_blur_cost_factor`
    forms the costs and, for a gradient, the table K (star) (mask l'), which
    `tike_farplane_scale` applies to the far plane."""
    how = dict(model=cm.model, measured=cm.mask, num_measured=cm.nmeasured,
               costs=costs)
    if detector.kind == "blur":
        nf = counts.shape[0]
        inten_all, table_all, unit = work
        inten = inten_all[:nf] if intensity is None else intensity
        op.fly_farplane_gradient(far, counts, fly, intensity=inten)
        table = table_all[:nf] if want_grad else None
        op.blur_cost_factor(inten, detector.value, counts, upstream=unit[:nf],
                            table=table, **how)
        if want_grad:
            check(
                lib.tike_farplane_scale(A.ptr(far), A.ptr(table), nf,
                                        far.shape[-3] * fly,
                                        far.shape[-1] * far.shape[-2], -1.0,
                                        A.stream_ptr()),
                "blur (table applied to the far plane)")
        return
    how["apply_gradient"] = want_grad
    if intensity is not None:
        how["intensity"] = intensity
    if detector.kind == "background":
        op.background_farplane_gradient(far, counts, fly, detector.value,
                                        **how)
    elif detector.kind == "binned":
        op.binned_farplane_gradient(far, counts, fly, detector.binning, **how)
    else:
        op.fly_farplane_gradient(far, counts, fly, **how)


def cost_factor(detector, far, inten, counts, u16, mask, upstream, costs,
                table, nf, fly, model, nmeasured):
    """The costs and the upstream table of `nf` frames of `autograd.cost`:
    the kind's `tike_*_cost_factor` on the far plane -- blurred: on `inten`,
    the stored intensities of this far plane.  counts, upstream, costs:
    raw pointers or None, at the chunk's first frame."""
    S, det = far.shape[-3], far.shape[-1]
    head = (A.ptr(far), counts, u16, A.ptr(mask))
    tail = (upstream, costs, A.ptr(table), nf, S * fly, det * far.shape[-2],
            model, nmeasured)
    st = A.stream_ptr()
    if detector.kind == "blur":
        K = detector.value
        check(
            lib.tike_blur_cost_factor(A.ptr(inten), A.ptr(K), K.shape[-1],
                                      counts, u16, A.ptr(mask), upstream,
                                      costs, A.ptr(table), None, nf, det,
                                      model, nmeasured, st),
            "cost (tike_blur_cost_factor)")
    elif detector.kind == "background":
        check(
            lib.tike_background_cost_factor(*head, A.ptr(detector.value),
                                            *tail, st),
            "cost (tike_background_cost_factor)")
    elif detector.kind == "binned":
        check(
            lib.tike_binned_cost_factor(*head, *tail, det, detector.binning,
                                        st), "cost (tike_binned_cost_factor)")
    else:
        check(lib.tike_cost_factor(*head, *tail, st),
              "cost (tike_cost_factor)")


def intensity(op, detector, far, fly, always_binned=False):
    """The frames (FRAME, w, w) float32 that this kind models from a chunk's
    far plane (N, 1, S, det, det) -- but for a background, which the caller
    adds (one in place, chunk by chunk, one into a new array).  always_binned: `_compute_intensity`'s
    habit of taking a fly scan through the binned entry at B = 1."""
    N, _, S, det, _ = far.shape
    w = detector.width(det)
    inten = torch.empty((N // fly, w, w), dtype=torch.float32,
                        device=far.device)
    # (the counts are read by the cost and the gradient only: any array of
    # the frames' shape serves)
    if detector.kind == "binned" or (always_binned and fly > 1):
        op.binned_farplane_gradient(far, torch.zeros_like(inten), fly,
                                    detector.binning, intensity=inten)
    elif fly > 1:
        op.fly_farplane_gradient(far, torch.zeros_like(inten), fly,
                                 intensity=inten)
    else:
        check(
            lib.tike_intensity(A.ptr(far), A.ptr(inten), N, S, det * det,
                               A.stream_ptr()), "intensity")
    if detector.kind == "blur":
        blurred = torch.empty_like(inten)
        op.blur_cost_factor(inten, detector.value, blurred=blurred)
        return blurred
    return inten
