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


def refuse(options, parameters, det, *, fly=1, binning=1, data_on_host=False,
           local_data=None, world_size=1):
    """Raise, by name, for everything a background cannot be combined with,
    before any device work."""
    if not isinstance(options, BackgroundOptions):
        raise TypeError(
            "background_options must be a tike_amd.ptycho.BackgroundOptions, "
            f"not {type(options).__name__}")
    name = parameters.algorithm_options.name
    if name != "cgrad":
        raise NotImplementedError(
            f"background_options with {name}: a fitted background is "
            "reconstructed by cgrad only")
    if binning > 1:
        raise NotImplementedError(
            f"background_options with binning={binning}: a background of "
            "binned data is not implemented")
    if parameters.psi.shape[0] > 1:
        raise NotImplementedError(
            "background_options with several slices (psi.shape[0] = "
            f"{parameters.psi.shape[0]}): a background of a multislice "
            "reconstruction is not implemented")
    if (parameters.eigen_probe is not None
            or parameters.eigen_weights is not None):
        raise NotImplementedError(
            "background_options with eigen probes is not implemented")
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
    b = options.background
    if A.is_device(b):
        b = A.to_host(b)
    b = np.asarray(b)
    if b.shape != (det, det):
        raise ValueError(
            f"background_options.background has shape {b.shape}; expected "
            f"the detector's ({det}, {det})")
    if b.dtype != np.float32:
        raise ValueError(
            f"background_options.background is {b.dtype}; expected float32")
    if not np.all(np.isfinite(b)) or np.any(b < 0):
        raise ValueError(
            "background_options.background must be finite and >= 0")
    return b


class State:
    """What cgrad reads of the background on the device: a = sqrt(b) (det,
    det) float32, the variable of its third block, and b = a * a."""

    def __init__(self, options, background):
        self.options = options
        self.set(torch.sqrt(A.to_device(background, np.float32)).contiguous())

    def set(self, a):
        self.a = a
        self.b = (a * a).contiguous()

    def write_back(self):
        self.options.background = A.to_host(self.b)
