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
from ..operators import detector as D

WIDTHS = D.BLUR_WIDTHS
checked_kernel = D.checked_kernel


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


def refuse(options, parameters, det, *, binning=1, data_on_host=False,
           local_data=None, world_size=1, background_options=None,
           blur_options=None):
    """Raise, by name, for everything a blur cannot be combined with, before
    any device work; the normalised kernel otherwise.  (The keywords are
    those of every model's `refuse`.)"""
    if not isinstance(options, BlurOptions):
        raise TypeError(
            "blur_options must be a tike_amd.ptycho.BlurOptions, not "
            f"{type(options).__name__}")
    name = parameters.algorithm_options.name
    if name != "cgrad":
        raise NotImplementedError(
            f"blur_options with {name}: a blurred far field is reconstructed "
            "by cgrad only")
    D.refuse("blur", D.RECONSTRUCTION, binning=binning,
             background=background_options is not None,
             slices=parameters.psi.shape[0],
             eigen=(parameters.eigen_probe is not None
                    or parameters.eigen_weights is not None))
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
    variable of its third block, and K = a^2 / sum a^2, the `value` of the
    far-plane step."""

    def __init__(self, options, kernel):
        self.options = options
        self.set(torch.sqrt(A.to_device(kernel, np.float32)).contiguous())

    def set(self, a):
        self.a = a
        self.value = kernel_of(a)

    def write_back(self):
        self.options.kernel = A.to_host(self.value)

    def cost_and_grad(self, op, counts, stored, a, cm, want_grad):
        """(sum of the per-frame costs at K = a^2 / sum a^2, a device scalar;
        d / d a of that sum, or None) of the frames whose intensities `stored`
        holds: one `tike_blur_kernel_sums` launch (with the gradient, its
        k * k lanes of a second), then `chain`, k * k numbers in torch."""
        partials, kgrad = op.blur_kernel_sums(
            stored, kernel_of(a), counts, model=cm.model, measured=cm.mask,
            num_measured=cm.nmeasured, want_gradient=want_grad)
        return partials.sum(), (chain(a, kgrad) if want_grad else None)
