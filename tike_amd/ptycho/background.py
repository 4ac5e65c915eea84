"""A fitted incoherent background per detector pixel (no reference
counterpart).

Air scatter, fluorescence, dark current and parasitic scatter from the optics
add a non-negative count to every detector pixel that does not move with the
scan:

    I_model[f][p] = sum_{j < fly * S} |farplane[f][j][p]|^2 + b[p],   b >= 0

`BackgroundOptions` hands `cgrad` a first guess of b (a dark frame, a small
constant) and says whether to fit it; the solver fits a = sqrt(b), so that
b = a * a stays non-negative through every trial of a line search and a pixel
that starts at 0 stays there.
"""
from __future__ import annotations

import dataclasses

import numpy as np
import torch

from .. import _arrays as A
from .._lib import check, lib
from ..operators import detector as D


@dataclasses.dataclass
class BackgroundOptions:
    """The incoherent background of `reconstruct(..., background_options=)`."""

    background: np.ndarray
    """(det, det) float32, >= 0, in the stored (FFT-shifted) layout of the
    data: the first guess going in, the fitted background coming out (a host
    array, written when `reconstruct` returns or `get_result()` is called)."""

    update: bool = True
    """Fit the background (a third conjugate-gradient block per minibatch,
    after the object's and the probe's); False: keep it as given."""

    update_start: int = 0
    """The first epoch that fits it."""


def refuse(options, parameters, det, *, binning=1, data_on_host=False,
           local_data=None, world_size=1, background_options=None,
           blur_options=None):
    """Raise, by name, for everything a background cannot be combined with,
    before any device work; the checked background otherwise.  (The keywords
    are those of every model's `refuse`.)"""
    if not isinstance(options, BackgroundOptions):
        raise TypeError(
            "background_options must be a tike_amd.ptycho.BackgroundOptions, "
            f"not {type(options).__name__}")
    name = parameters.algorithm_options.name
    if name != "cgrad":
        raise NotImplementedError(
            f"background_options with {name}: a fitted background is "
            "reconstructed by cgrad only")
    D.refuse("background", D.RECONSTRUCTION, binning=binning,
             slices=parameters.psi.shape[0],
             eigen=(parameters.eigen_probe is not None
                    or parameters.eigen_weights is not None))
    if parameters.position_options is not None:
        raise NotImplementedError(
            "background_options with position_options: position correction "
            "together with a background is not implemented")
    if data_on_host:
        raise NotImplementedError(
            "background_options with data_on_host: the background block "
            "reads the minibatch's patterns in HBM")
    if local_data is not None:
        raise NotImplementedError(
            "background_options with local_data (the ranks started by "
            "reconstruct(num_gpu=N)) is not implemented")
    if world_size > 1:
        raise NotImplementedError(
            "background_options with the ranks of a torch.distributed job: a "
            "background is fitted in one process")
    return D.checked_background(options.background, det,
                                "background_options.background")


class State:
    """What cgrad reads of the background on the device: a = sqrt(b) (det,
    det) float32, the variable of its third block, and b = a * a, the `value`
    of the far-plane step."""

    def __init__(self, options, background):
        self.options = options
        self.set(torch.sqrt(A.to_device(background, np.float32)).contiguous())

    def set(self, a):
        self.a = a
        self.value = (a * a).contiguous()

    def write_back(self):
        self.options.background = A.to_host(self.value)

    def cost_and_grad(self, op, counts, stored, a, cm, want_grad):
        """(sum of the per-frame costs at b = a * a, a device scalar; d / d a
        of that sum = 2 a bgrad, or None) of the frames whose intensities
        `stored` holds: one `tike_background_sums` launch."""
        npix = stored.shape[-1] * stored.shape[-2]
        b = (a * a).contiguous()
        partials = torch.zeros(lib.tike_background_sums_partials(npix),
                               dtype=torch.float64, device=a.device)
        bgrad = torch.empty_like(b) if want_grad else None
        check(
            lib.tike_background_sums(
                A.ptr(stored), A.ptr(counts),
                int(counts.dtype == torch.uint16), A.ptr(cm.mask), A.ptr(b),
                None, A.ptr(partials), A.ptr(bgrad), counts.shape[0], npix,
                cm.model, cm.nmeasured, A.stream_ptr()),
            "cgrad background sums")
        return partials.sum(), (2 * a * bgrad if want_grad else None)
