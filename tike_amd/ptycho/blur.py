"""Far-field blur: partial spatial coherence and the detector's point-spread
function (no reference counterpart).

A source of finite size -- in the Gaussian-Schell approximation, partial
spatial coherence -- convolves the far-field intensity with the scaled image
of the source; charge sharing, scintillator blur or the MTF of an electron
detector convolve it with the detector's point-spread function.  Both are a
small non-negative kernel on the recorded intensity:

    I_model[f] = K (*) I[f],   I[f][p] = sum_{j < fly * S} |farplane[f][j][p]|^2

K (k, k), k in (3, 5, 7), every entry >= 0, centre at [k // 2, k // 2], sum 1.
The convolution is CYCLIC over the (det, det) plane in the stored
(FFT-shifted) layout of the data.  The shift between the stored and the
physical layout is itself cyclic, so this is the physical convolution with
the detector's opposite edges joined; the edges are the dark part of a frame.

One probe mode and such a kernel is the standard compact model of what
otherwise takes several probe modes (Clark et al. 2011; Burdet et al. 2015),
and the only one of a point-spread function, which acts after |.|^2.

`BlurOptions` hands `cgrad` a first guess of K and says whether to fit it.
The scale of K is the probe's power, so K is kept at sum 1: it is normalised
once on entry, and the solver fits a real a (k, k) with K = a^2 / sum a^2,
which stays non-negative through every trial of a line search; an entry that
starts at 0 stays there.  With g = d cost / d K,

    d cost / d a = 2 a / sum a^2 (g - sum(g K)).
"""
from __future__ import annotations

import dataclasses

import numpy as np
import torch

from .. import _arrays as A

WIDTHS = (3, 5, 7)


@dataclasses.dataclass
class BlurOptions:
    """The far-field blur of `reconstruct(..., blur_options=)`."""

    kernel: np.ndarray
    """(k, k) float32, k in (3, 5, 7), >= 0, not all zero, the centre at
    [k // 2, k // 2], in the stored (FFT-shifted) layout of the data: the first
    guess going in (normalised to sum 1 on entry), the fitted kernel coming
    out (a host array, written when `reconstruct` returns or `get_result()`
    is called)."""

    update: bool = True
    """Fit the kernel (a third conjugate-gradient block per minibatch, after
    the object's and the probe's); False: keep it as given."""

    update_start: int = 0
    """The first epoch that fits it."""


def checked_kernel(kernel, det, what="blur"):
    """`kernel` as a host (k, k) float32 array of sum 1, after validation of
    its shape, dtype, finiteness and sign."""
    K = kernel
    if A.is_device(K):
        K = A.to_host(K)
    K = np.asarray(K)
    k = K.shape[-1] if K.ndim else 0
    if K.ndim != 2 or K.shape != (k, k) or k not in WIDTHS:
        raise ValueError(
            f"{what} has shape {K.shape}; expected (k, k) with k in {WIDTHS}")
    if K.dtype != np.float32:
        raise ValueError(f"{what} is {K.dtype}; expected float32")
    if k > det:
        raise ValueError(
            f"{what} {K.shape} is wider than the detector ({det}, {det})")
    if not np.all(np.isfinite(K)) or np.any(K < 0):
        raise ValueError(f"{what} must be finite and >= 0")
    total = float(K.sum(dtype=np.float64))
    if not total > 0:
        raise ValueError(f"{what} must have a positive sum")
    return (K.astype(np.float64) / total).astype(np.float32)


def refuse(options, parameters, det, *, fly=1, binning=1, data_on_host=False,
           local_data=None, world_size=1, background_options=None):
    """Raise, by name, for everything a blur cannot be combined with, before
    any device work; the normalised kernel otherwise."""
    if not isinstance(options, BlurOptions):
        raise TypeError(
            "blur_options must be a tike_amd.ptycho.BlurOptions, not "
            f"{type(options).__name__}")
    name = parameters.algorithm_options.name
    if name != "cgrad":
        raise NotImplementedError(
            f"blur_options with {name}: a blurred far field is reconstructed "
            "by cgrad only")
    if binning > 1:
        raise NotImplementedError(
            f"blur_options with binning={binning}: a blur of binned data is "
            "not implemented")
    if background_options is not None:
        raise NotImplementedError(
            "blur_options with background_options: a blur together with a "
            "background is not implemented")
    if parameters.psi.shape[0] > 1:
        raise NotImplementedError(
            "blur_options with several slices (psi.shape[0] = "
            f"{parameters.psi.shape[0]}): a blur of a multislice "
            "reconstruction is not implemented")
    if (parameters.eigen_probe is not None
            or parameters.eigen_weights is not None):
        raise NotImplementedError(
            "blur_options with eigen probes is not implemented")
    if parameters.position_options is not None:
        raise NotImplementedError(
            "blur_options with position_options: position correction "
            "together with a blur is not implemented")
    if data_on_host:
        raise NotImplementedError(
            "blur_options with data_on_host: the kernel block reads the "
            "minibatch's patterns in HBM")
    if local_data is not None:
        raise NotImplementedError(
            "blur_options with local_data (the ranks started by "
            "reconstruct(num_gpu=N)) is not implemented")
    if world_size > 1:
        raise NotImplementedError(
            "blur_options with the ranks of a torch.distributed job: a blur "
            "kernel is fitted in one process")
    return checked_kernel(options.kernel, det, "blur_options.kernel")


def kernel_of(a):
    """K = a^2 / sum a^2 (k, k) float32 on the device, the sum in float64."""
    sq = a.to(torch.float64)**2
    return (sq / sq.sum()).to(torch.float32).contiguous()


def chain(a, kgrad):
    """d / d a of a function of K = a^2 / sum a^2 whose gradient with respect
    to K is kgrad (k, k) float64: 2 a / sum a^2 (g - sum(g K)), k^2 numbers in
    float64, rounded once."""
    a64 = a.to(torch.float64)
    sq = a64 * a64
    total = sq.sum()
    return (2 * a64 / total * (kgrad - (kgrad * sq).sum() / total)).to(
        torch.float32)


class State:
    """What cgrad reads of the blur on the device: a (k, k) float32, the
    variable of its third block, and K = a^2 / sum a^2."""

    def __init__(self, options, kernel):
        self.options = options
        self.set(torch.sqrt(A.to_device(kernel, np.float32)).contiguous())

    def set(self, a):
        self.a = a
        self.kernel = kernel_of(a)

    def write_back(self):
        self.options.kernel = A.to_host(self.kernel)
