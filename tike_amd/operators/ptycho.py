"""The ptychography operator (reference operators/cupy/ptycho.py:26-204).

``fwd`` and ``adj`` keep the reference's signatures and shapes but run as
fused HIP kernels: patch gather * probe -> FFT2 (``tike_ptycho_fwd``) and,
for the adjoint, the two-pass inverse transform whose second pass forms both
products in place (``tike_ptycho_adj``; other shapes: ``tike_ifft2_crop``
followed by the unfused object scatter-add and probe product).
"""

import numpy as np
import torch

from .. import _tuning
from .. import _arrays as A
from .._lib import check, lib
from . import detector as D
from . import nearfield as NF
from . import objective
from .multislice import Multislice
from .operator import Operator
from .propagation import Propagation, fft_scales


def sub_batch_positions(S, det, mib=None):
    """Positions per sub-batch of the two-kernel 256^2 / 512^2 operators: the
    ``sub_batch`` argument of ``tike_ptycho_fwd`` / ``tike_ptycho_adj``
    (0 = the library's default -- 256 MiB of far plane for the forward
    operator, one batch for the adjoint --, -1 = one batch).
    ``TIKE_FWD_SUB_MIB`` (`tike_amd._tuning`) is read on the host side of
    the C ABI, never inside the library."""
    if mib is None:
        mib = _tuning.fwd_sub_mib
    if mib is None:
        return 0
    mib = float(mib)
    if mib <= 0:
        return -1
    return max(1, int(mib * 2**20) // (8 * S * det * det))


def _positions_allowed(scan, psi_shape, pw):
    """check_allowed_positions as a predicate (position.py:600-628): every
    patch and its +1 taps inside the object.  Host arrays are tested on the
    host; a device tensor costs one small reduction and a read-back."""
    hi_y, hi_x = psi_shape[-2] - pw - 1, psi_shape[-1] - pw - 1
    if isinstance(scan, torch.Tensor):
        c = torch.floor(scan)
        lo = c.amin(dim=0)
        hi = c.amax(dim=0)
        ok = (lo >= 1).all() & (hi[0] <= hi_y) & (hi[1] <= hi_x)
        return bool(ok.item())
    c = np.floor(scan)
    return bool(c.min() >= 1 and c[..., 0].max() <= hi_y
                and c[..., 1].max() <= hi_x)


class Ptycho(Operator):
    """Compose diffraction and far-field propagation.

    farplane (POSI, 1, SHARED, det, det) complex64;
    probe (1|POSI, 1, SHARED, pw, pw) complex64; psi (DEPTH, H, W) complex64;
    scan (POSI, 2) float32; data (FRAME, det, det) float32.

    ``probe_wavelength``, ``probe_FOV_lengths`` and
    ``multislice_propagation_distance`` are only used by multi-slice objects
    and default to the values ``reconstruct`` passes for one slice.
    """

    def __init__(self, detector_shape, probe_shape,
                 probe_wavelength=float("nan"),
                 probe_FOV_lengths=(float("nan"), float("nan")), nz=None,
                 n=None, multislice_propagation_distance=1e-9,
                 propagation=Propagation, diffraction=Multislice, norm="ortho",
                 **kwargs):
        if nz is None or n is None:
            raise TypeError("Ptycho requires nz and n (object height, width)")
        shapes = dict(probe_shape=probe_shape, detector_shape=detector_shape,
                      nz=nz, n=n)
        optics = dict(
            probe_wavelength=probe_wavelength,
            probe_FOV_lengths=probe_FOV_lengths,
            multislice_propagation_distance=multislice_propagation_distance)
        vars(self).update(shapes, norm=norm, **optics)
        self.diffraction = diffraction(**shapes, **optics, **kwargs)
        self.propagation = propagation(detector_shape=detector_shape,
                                       norm=norm, **kwargs)

    def __enter__(self):
        self.propagation.__enter__()
        self.diffraction.__enter__()
        return self

    def __exit__(self, type, value, traceback):
        self.propagation.__exit__(type, value, traceback)
        self.diffraction.__exit__(type, value, traceback)

    # -- device-level entry points used by the solvers ---------------------
    def fwd_device(self, probe, scan, psi, eigen_probe=None,
                   eigen_weights=None, out=None, sub_batch=None):
        """Fused forward on device tensors; optional on-the-fly eigen probes.

        probe (1|N,1,S,pw,pw); eigen_probe (1,C,Sm,pw,pw) and eigen_weights
        (N,C+1,S) select the varying probe of probe.py:272-303.  sub_batch:
        positions per sub-batch at 256^2 / 512^2 (None: sub_batch_positions).
        """
        Multislice._one_slice(psi)
        N = scan.shape[0]
        S, pw, det = probe.shape[-3], self.probe_shape, self.detector_shape
        assert probe.shape[-1] == pw and probe.shape[-2] == pw
        assert probe.shape[0] in (1, N)
        if out is None:
            out = torch.empty((N, 1, S, det, det), dtype=torch.complex64,
                              device=psi.device)
        C = Sm = 0
        if eigen_weights is not None:
            assert probe.shape[0] == 1
            assert eigen_weights.shape[0] == N and eigen_weights.shape[2] == S
            if eigen_probe is not None:
                C, Sm = eigen_probe.shape[-4], eigen_probe.shape[-3]
            assert eigen_weights.shape[1] >= C + 1
            if eigen_weights.shape[1] != C + 1:
                eigen_weights = eigen_weights[:, :C + 1].contiguous()
        check(
            lib.tike_ptycho_fwd(
                A.ptr(psi), A.ptr(scan), A.ptr(probe),
                int(probe.shape[0] != 1), A.ptr(eigen_probe),
                A.ptr(eigen_weights), C, Sm, A.ptr(out), N, S, pw, det,
                psi.shape[-2], psi.shape[-1], fft_scales(det, self.norm)[0],
                sub_batch_positions(S, det) if sub_batch is None else
                int(sub_batch), A.stream_ptr()), "Ptycho.fwd")
        return out

    def fwd(self, probe, scan, psi, **kwargs):
        kind = psi
        psi = A.to_device(psi, np.complex64)
        scan = A.to_device(scan, np.float32)
        probe = A.to_device(probe, np.complex64)
        assert probe.ndim == 5 and probe.shape[1] == 1, probe.shape
        if psi.shape[0] > 1:
            # several object slices (ptycho.py:114-129 over multislice.py:
            # 69-92): slice-by-slice composition, then the far-field transform
            far = self.propagation.fwd(self.diffraction.fwd(
                psi=psi, scan=scan, probe=probe[..., 0, :, :, :]),
                                       overwrite=True)[..., None, :, :, :]
            return A.like_input(far, kind)
        return A.like_input(self.fwd_device(probe, scan, psi), kind)

    def fwd_return_intermediate_probes(self, probe, scan, psi, **kwargs):
        """(farplane, probes incident on every slice) -- ptycho.py:131-146."""
        on_device = (A.to_device(psi, np.complex64),
                     A.to_device(scan, np.float32),
                     A.to_device(probe, np.complex64))
        exitwave, beams = self.diffraction.fwd_return_intermediate_probes(
            psi=on_device[0], scan=on_device[1], probe=on_device[2])
        far = self.propagation.fwd(nearplane=exitwave, overwrite=True)
        return (A.like_input(far.unsqueeze(-4), psi),
                A.like_input(beams, psi))

    def fused_adjoint_shapes(self, S):
        """Shapes the fused adjoint (``tike_ptycho_adj``) takes: probe window =
        detector in {128, 256, 512}, at most 8 modes."""
        return (self.probe_shape == self.detector_shape
                and self.detector_shape in (128, 256, 512) and S <= 8)

    def adj_device(self, farplane, probe, scan, psi, psi_adj=None,
                   probe_adj=None, sub_batch=None):
        """Fused adjoint on device tensors (``tike_ptycho_adj``): inverse pass 1
        into ``probe_adj``, pass 2 in place with both products, grouped
        footprint scatter.  Requires ``fused_adjoint_shapes`` and scan positions
        that satisfy ``check_allowed_positions`` (position.py:600-628: what the
        solvers guarantee; ``adj`` checks it).  ``farplane`` is not modified.
        """
        Multislice._one_slice(psi)
        N, S = scan.shape[0], farplane.shape[-3]
        pw, det = self.probe_shape, self.detector_shape
        assert tuple(farplane.shape) == (N, 1, S, det, det), farplane.shape
        assert probe.shape[0] in (1, N) and probe.shape[-3] == S
        H, W = psi.shape[-2:]
        dev = psi.device
        if probe_adj is None:
            probe_adj = torch.empty((N, 1, S, pw, pw), dtype=torch.complex64,
                                    device=dev)
        if psi_adj is None:
            psi_adj = torch.empty_like(psi)
        objproj = torch.empty((max(N, 1), pw, pw), dtype=torch.complex64,
                              device=dev)
        acc = torch.empty((2, H, W), dtype=torch.float32, device=dev)
        check(
            lib.tike_ptycho_adj(
                A.ptr(farplane), A.ptr(probe), int(probe.shape[0] != 1),
                A.ptr(scan), A.ptr(psi), A.ptr(psi_adj), A.ptr(probe_adj),
                A.ptr(objproj), A.ptr(acc), N, S, pw, det, H, W,
                fft_scales(det, self.norm)[1],
                sub_batch_positions(S, det) if sub_batch is None else
                int(sub_batch), A.stream_ptr()), "Ptycho.adj")
        return psi_adj, probe_adj

    def adj(self, farplane, probe, scan, psi, overwrite=False, **kwargs):
        kind = farplane
        farplane_in = farplane
        host_scan = None if A.is_device(scan) else np.asarray(scan)
        farplane = A.to_device(farplane, np.complex64)
        psi = A.to_device(psi, np.complex64)
        scan = A.to_device(scan, np.float32)
        probe = A.to_device(probe, np.complex64)
        if psi.shape[0] > 1:  # ptycho.py:148-176 over multislice.py:144-194
            psi_adj, probe_adj = self.diffraction.adj(
                nearplane=self.propagation.adj(
                    farplane, overwrite=False)[..., 0, :, :, :],
                probe=probe[..., 0, :, :, :], scan=scan, psi=psi)
            return (A.like_input(psi_adj, kind),
                    A.like_input(probe_adj[..., None, :, :, :], kind))
        N, S = scan.shape[0], farplane.shape[-3]
        pw, det = self.probe_shape, self.detector_shape
        assert tuple(farplane.shape) == (N, 1, S, det, det), farplane.shape
        assert probe.shape[0] in (1, N) and probe.shape[-3] == S
        if N > 0 and self.fused_adjoint_shapes(S) and _positions_allowed(
                scan if host_scan is None else host_scan, psi.shape, pw):
            psi_adj, probe_adj = self.adj_device(farplane, probe, scan, psi)
            return A.like_input(psi_adj, kind), A.like_input(probe_adj, kind)
        # general shapes (probe window narrower than the detector, other
        # sizes, more than 8 modes) and positions whose taps leave the image
        # (the reference's linear tap addressing, convolution.cu:113-133):
        # IFFT2 + crop, then the unfused Convolution adjoints
        in_place = (overwrite and A.is_device(farplane_in)
                    and farplane.data_ptr() == farplane_in.data_ptr())
        work = farplane if in_place else torch.empty_like(farplane)
        chi = work if pw == det else torch.empty(
            (N, 1, S, pw, pw), dtype=torch.complex64, device=psi.device)
        check(
            lib.tike_ifft2_crop(A.ptr(farplane), A.ptr(work), A.ptr(chi),
                                N * S, det, pw,
                                fft_scales(det, self.norm)[1],
                                A.stream_ptr()), "Ptycho.adj (ifft2)")
        psi_adj = torch.zeros_like(psi)
        check(
            lib.tike_conv_adj(A.ptr(chi), A.ptr(scan), A.ptr(probe),
                              int(probe.shape[0] != 1), A.ptr(psi_adj), N, S,
                              pw, pw, psi.shape[-2], psi.shape[-1],
                              A.stream_ptr()), "Ptycho.adj (object)")
        probe_adj = torch.empty((N, 1, S, pw, pw), dtype=torch.complex64,
                                device=psi.device)
        check(
            lib.tike_conv_adj_probe(A.ptr(chi), A.ptr(scan), A.ptr(psi),
                                    A.ptr(probe_adj), N, S, pw, pw,
                                    psi.shape[-2], psi.shape[-1],
                                    A.stream_ptr()), "Ptycho.adj (probe)")
        return A.like_input(psi_adj, kind), A.like_input(probe_adj, kind)

    def fly_farplane_gradient(self, farplane, data, fly, *, model=0,
                              measured=None, num_measured=None,
                              intensity=None, costs=None, apply_gradient=False,
                              unmeasured_scaling=1.0):
        """`tike_fly_farplane_gradient` on device tensors: farplane
        (FRAME * fly, 1, SHARED, det, det) complex64, frame f exposed by the
        positions f * fly ... f * fly + fly - 1; data (FRAME, det, det) float32
        or uint16; measured a (det, det) uint8 mask or None; intensity
        (FRAME, det, det) and costs (FRAME) float32 outputs or None.  With
        apply_gradient farplane becomes -gradient on the measured pixels."""
        det = self.detector_shape
        S = farplane.shape[-3]
        nframe = data.shape[0]
        assert farplane.shape[0] == nframe * fly, (farplane.shape, nframe, fly)
        assert tuple(data.shape[1:]) == (det, det), data.shape
        assert data.dtype in (torch.float32, torch.uint16), data.dtype
        check(
            lib.tike_fly_farplane_gradient(
                A.ptr(farplane), A.ptr(data), int(data.dtype == torch.uint16),
                A.ptr(measured), A.ptr(intensity), A.ptr(costs), nframe,
                int(fly), S, det, int(model), int(bool(apply_gradient)),
                float(unmeasured_scaling),
                det * det if num_measured is None else int(num_measured),
                A.stream_ptr()), "Ptycho.fly_farplane_gradient")
        return farplane

    def background_farplane_gradient(self, farplane, data, fly, background, *,
                                     model=0, measured=None,
                                     num_measured=None, intensity=None,
                                     costs=None, apply_gradient=False,
                                     unmeasured_scaling=1.0):
        """`tike_background_farplane_gradient` on device tensors:
        `fly_farplane_gradient` with an incoherent background (det, det)
        float32 added to every frame's intensity, in the stored (FFT-shifted)
        layout of the data.  Costs and the gradient factor are taken at
        I + background; `intensity` receives I without it.  background None
        is `fly_farplane_gradient`."""
        det = self.detector_shape
        S = farplane.shape[-3]
        nframe = data.shape[0]
        assert farplane.shape[0] == nframe * fly, (farplane.shape, nframe, fly)
        assert tuple(data.shape[1:]) == (det, det), data.shape
        assert data.dtype in (torch.float32, torch.uint16), data.dtype
        if background is not None:
            assert tuple(background.shape) == (det, det), background.shape
            assert background.dtype == torch.float32, background.dtype
            assert background.is_contiguous()
        check(
            lib.tike_background_farplane_gradient(
                A.ptr(farplane), A.ptr(data), int(data.dtype == torch.uint16),
                A.ptr(measured), A.ptr(background), A.ptr(intensity),
                A.ptr(costs), nframe, int(fly), S, det, int(model),
                int(bool(apply_gradient)), float(unmeasured_scaling),
                det * det if num_measured is None else int(num_measured),
                A.stream_ptr()), "Ptycho.background_farplane_gradient")
        return farplane

    def binned_farplane_gradient(self, farplane, data, fly, binning, *,
                                 model=0, measured=None, num_measured=None,
                                 intensity=None, costs=None,
                                 apply_gradient=False, unmeasured_scaling=1.0):
        """`tike_binned_farplane_gradient` on device tensors: the far plane
        (FRAME * fly, 1, SHARED, det, det) is `binning` = B times finer than
        the measured pixels, w = det // B.  data (FRAME, w, w) float32 or
        uint16; measured a (w, w) uint8 mask or None; intensity (FRAME, w, w)
        and costs (FRAME) float32 outputs or None.  In the stored layout
        (FFT-shifted, the peak at the corners) a measured pixel (U, V) is the
        sum of |farplane|^2 over the rows U * B ... U * B + B - 1, the columns
        V * B ... V * B + B - 1, the frame's positions and the modes.  When w
        is even this block sum equals the block sum on the centred detector:
        fftshift(I) == blocksum(fftshift(fine)), because the shift by det / 2
        = (w / 2) * B moves whole blocks.  With apply_gradient every far-plane
        pixel of a bin is scaled by the bin's factor (-gradient factor on
        measured bins).  binning == 1 is `fly_farplane_gradient`."""
        det = self.detector_shape
        B = int(binning)
        if B < 1 or det % B:
            raise ValueError(
                f"binning={binning!r} does not divide the far-plane width "
                f"{det}")
        w = det // B
        S = farplane.shape[-3]
        nframe = data.shape[0]
        assert farplane.shape[0] == nframe * fly, (farplane.shape, nframe, fly)
        assert tuple(farplane.shape[-2:]) == (det, det), farplane.shape
        assert tuple(data.shape[1:]) == (w, w), data.shape
        assert data.dtype in (torch.float32, torch.uint16), data.dtype
        assert measured is None or tuple(measured.shape) == (w, w)
        assert intensity is None or tuple(intensity.shape) == (nframe, w, w)
        check(
            lib.tike_binned_farplane_gradient(
                A.ptr(farplane), A.ptr(data), int(data.dtype == torch.uint16),
                A.ptr(measured), A.ptr(intensity), A.ptr(costs), nframe,
                int(fly), S, det, B, int(model), int(bool(apply_gradient)),
                float(unmeasured_scaling),
                w * w if num_measured is None else int(num_measured),
                A.stream_ptr()), "Ptycho.binned_farplane_gradient")
        return farplane

    def blur_cost_factor(self, intensity, kernel, data=None, *, model=0,
                         measured=None, num_measured=None, upstream=None,
                         costs=None, table=None, blurred=None):
        """`tike_blur_cost_factor` on device tensors: the model
        I_model = kernel (*) intensity, cyclic over the (det, det) plane in
        the stored (FFT-shifted) layout, on STORED intensities (FRAME, det,
        det) float32 -- what `fly_farplane_gradient(intensity=)` or
        `_compute_intensity` write.  kernel (k, k) float32, k in (3, 5, 7),
        used as given; data (FRAME, det, det) float32 or uint16 (None when only
        `blurred` is asked for); measured a (det, det) uint8 mask or None;
        upstream (FRAME) float32 or None.  Outputs, each float32 or None:
        costs (FRAME), table (FRAME, det, det) = kernel (star) (upstream mask
        l' / num_measured), the factor the far plane is multiplied by for the
        gradient, and blurred (FRAME, det, det) = I_model."""
        det = self.detector_shape
        nframe = intensity.shape[0]
        assert tuple(intensity.shape[1:]) == (det, det), intensity.shape
        assert intensity.dtype == torch.float32 and intensity.is_contiguous()
        assert kernel.dtype == torch.float32 and kernel.is_contiguous()
        assert kernel.ndim == 2 and kernel.shape[0] == kernel.shape[1]
        if data is not None:
            assert tuple(data.shape) == (nframe, det, det), data.shape
            assert data.dtype in (torch.float32, torch.uint16), data.dtype
        check(
            lib.tike_blur_cost_factor(
                A.ptr(intensity), A.ptr(kernel), int(kernel.shape[0]),
                A.ptr(data),
                int(data is not None and data.dtype == torch.uint16),
                A.ptr(measured), A.ptr(upstream), A.ptr(costs), A.ptr(table),
                A.ptr(blurred), nframe, det, int(model),
                det * det if num_measured is None else int(num_measured),
                A.stream_ptr()), "Ptycho.blur_cost_factor")

    def blur_kernel_sums(self, intensity, kernel, data, *, model=0,
                         measured=None, num_measured=None, upstream=None,
                         want_gradient=True):
        """`tike_blur_kernel_sums` on device tensors (arguments as
        `blur_cost_factor`): (cost partials float64, kgrad (k, k) float64 or
        None).  The sum of the partials is sum_f upstream_f cost_f (upstream
        None: ones), kgrad its gradient with respect to the kernel.  One
        launch without the gradient, a second of k * k lanes with it; no
        forward operator, no transform."""
        det = self.detector_shape
        nframe, k = intensity.shape[0], int(kernel.shape[0])
        assert tuple(intensity.shape[1:]) == (det, det), intensity.shape
        assert intensity.dtype == torch.float32 and intensity.is_contiguous()
        assert kernel.dtype == torch.float32 and kernel.is_contiguous()
        assert tuple(data.shape) == (nframe, det, det), data.shape
        assert data.dtype in (torch.float32, torch.uint16), data.dtype
        n = lib.tike_blur_kernel_sums_partials(det, k)
        if n <= 0:
            raise ValueError(
                f"blur kernel {tuple(kernel.shape)} on a ({det}, {det}) "
                "detector: incompatible shapes / arguments")
        buf = torch.empty(n, dtype=torch.float64, device=intensity.device)
        kgrad = (torch.empty((k, k), dtype=torch.float64,
                             device=intensity.device)
                 if want_gradient else None)
        check(
            lib.tike_blur_kernel_sums(
                A.ptr(intensity), A.ptr(kernel), k, A.ptr(data),
                int(data.dtype == torch.uint16), A.ptr(measured),
                A.ptr(upstream), A.ptr(buf), A.ptr(kgrad), nframe, det,
                int(model),
                det * det if num_measured is None else int(num_measured),
                A.stream_ptr()), "Ptycho.blur_kernel_sums")
        return buf[:n // (1 + k * k)], kgrad

    def _detector(self, psi, probe, binning, background, blur, nearfield):
        """The `detector.Detector` of `_compute_intensity` and `cost` (host
        or device arrays), its b, K or H on the device."""
        det = self.detector_shape
        window = probe.shape[-1]
        return D.resident_value(
            D.build(D.OPERATOR, det, binning=binning, background=background,
                    blur=blur, nearfield=nearfield, slices=psi.shape[0],
                    window=window if window != det else self.probe_shape),
            det)

    def _frame_inputs(self, psi, scan, probe, fly):
        """psi, scan and probe on the device, scan in whole frames."""
        scan = A.to_device(scan, np.float32)
        if scan.shape[0] % fly:
            raise ValueError(
                f"{scan.shape[0]} scan positions are not a multiple of "
                f"fly={fly}")
        return (A.to_device(psi, np.complex64), scan,
                A.to_device(probe, np.complex64))

    def _compute_intensity(self, data, psi, scan, probe, fly=1, binning=1,
                           background=None, blur=None, nearfield=None):
        """(intensity (FRAME,det,det), farplane) -- ptycho.py:178-191; with
        fly > 1 a frame is the sum over `fly` consecutive positions
        (ptycho.py:104-125); with binning = B > 1 the intensity is
        (FRAME, det // B, det // B), a pixel the sum over its B x B far-plane
        pixels (`binned_farplane_gradient`); with a background (det, det) the
        intensity includes it; with a blur (k, k) the intensity is convolved
        with it, cyclically over the plane (`blur_cost_factor`); with nearfield
        (det, det) complex64 the detector sits in the near field: the
        intensity is |IFFT2(nearfield FFT2(patch x probe))|^2 and the second
        result is that detector-plane wave (`operators.nearfield`).  What the
        detector does: `operators.detector`."""
        det = self.detector_shape
        if binning < 1 or det % binning:
            raise ValueError(
                f"binning={binning!r} does not divide the far-plane "
                f"width {det}")
        detector = self._detector(psi, probe, binning, background, blur,
                                  nearfield)
        psi_d, scan_d, probe_d = self._frame_inputs(psi, scan, probe, fly)
        if detector.kind == "nearfield":
            w = NF.detector_wave(self, psi_d, scan_d, probe_d, detector.value)
            N, S = w.shape[:2]
            intensity = torch.empty((N // fly, det, det), dtype=torch.float32,
                                    device=w.device)
            self.fly_farplane_gradient(w, torch.zeros_like(intensity), fly,
                                       intensity=intensity)
            far = w.view(N, 1, S, det, det)
        else:
            far = self.fwd_device(probe_d, scan_d, psi_d)
            intensity = D.intensity(self, detector, far, fly,
                                    always_binned=True)
            if detector.kind == "background":
                intensity = intensity + detector.value
        return A.like_input(intensity, psi), A.like_input(far, psi)

    def cost(self, data, psi, scan, probe, *, model, fly=1, binning=1,
             background=None, blur=None, nearfield=None):
        """ptycho.py:193-204; with fly > 1 or binning > 1 the mean over frames
        of the cost of each frame's summed (and binned) intensity; with a
        background (det, det) the cost of intensity + background
        (`background_farplane_gradient`); with a blur (k, k) the cost of
        blur (*) intensity (`blur_cost_factor` on the stored intensities); with
        nearfield (det, det) complex64 the mean over frames of the cost of
        |IFFT2(nearfield FFT2(patch x probe))|^2 (`operators.nearfield`, the
        general route).  What the detector does: `operators.detector`."""
        detector = self._detector(psi, probe, binning, background, blur,
                                  nearfield)
        if detector.kind == "far" and fly == 1:
            intensity, _ = self._compute_intensity(data, psi, scan, probe)
            return getattr(objective, model)(data, intensity)
        if model not in objective._MODELS:
            raise ValueError(f"unknown noise model {model!r}")
        cm = D.Model(objective._MODELS[model])
        psi_d, scan_d, probe_d = self._frame_inputs(psi, scan, probe, fly)
        if detector.kind != "nearfield":
            far = self.fwd_device(probe_d, scan_d, psi_d)
        if detector.kind == "blur":
            stored = D.intensity(self, D.Detector(), far, fly,
                                 always_binned=True)
        counts = A.counts(A.to_device(data)).contiguous()
        if counts.shape[0] * fly != scan_d.shape[0]:
            raise ValueError(
                f"{counts.shape[0]} frames of fly={fly} do not match "
                f"{scan_d.shape[0]} scan positions")
        costs = torch.empty(counts.shape[0], dtype=torch.float32,
                            device=psi_d.device)
        if detector.kind == "nearfield":
            S, det = probe_d.shape[-3], self.detector_shape
            NF.wave_and_back(
                self, psi_d, scan_d, probe_d, detector.value, counts, fly,
                "general", NF.buffers(None, psi_d.device, 0, S, det, fly,
                                      "general", table=False),
                model=cm.model, costs=costs)
        elif detector.kind == "blur":
            self.blur_cost_factor(stored, detector.value, counts,
                                  model=cm.model, costs=costs)
        else:
            # (a fly scan alone goes through the binned entry at B = 1)
            D.farplane_step(
                self, detector._replace(kind="binned")
                if detector.kind == "far" else detector, far, counts, fly, cm,
                costs=costs)
        return A.like_input(costs.mean(), psi)
