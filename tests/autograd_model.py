"""Float64 model of `tike_amd.autograd.intensity` (test infrastructure).

`intensity` restates the forward model in complex128 torch on the CPU --
bilinear gather with the taps of `oracle.operators._patch_geometry`, probe
product, centred zero padding, `torch.fft.fft2` with the operator's norm,
|.|^2, sums over the modes and over the `fly` positions of a frame -- so that
its gradients come from `torch.autograd` itself.  `hand_gradients` holds the
formulas the HIP backward implements, in float64, with the absolute-term sums
A_n the scan-gradient bars are stated in; `problem` is the position-recovery
problem of the CPU and GPU tests.
"""
import numpy as np
import torch
from scipy.ndimage import gaussian_filter

C128, F64 = torch.complex128, torch.float64


def as_model(psi, probe, scan):
    """float32 / complex64 host arrays -> the model's float64 tensors (the
    float32 VALUES: fractions and taps are those the kernels see)."""
    return (torch.from_numpy(np.asarray(psi)).to(C128),
            torch.from_numpy(np.asarray(probe)).to(C128),
            torch.from_numpy(np.asarray(scan, dtype=np.float32)).to(F64))


def _taps(psi, scan, pw):
    """(O00, O01, O10, O11) each (N, pw, pw), and the fractions (fy, fx)
    (N, 1, 1).  The integer part of a position is a constant."""
    corner = torch.floor(scan.detach())
    frac = scan - corner
    sy, sx = corner[:, 0].long(), corner[:, 1].long()
    r = torch.arange(pw)
    yy = sy[:, None, None] + r[None, :, None]
    xx = sx[:, None, None] + r[None, None, :]
    img = psi[0]
    taps = (img[yy, xx], img[yy, xx + 1], img[yy + 1, xx], img[yy + 1, xx + 1])
    return taps, frac[:, 0, None, None], frac[:, 1, None, None]


def patches(psi, scan, pw):
    """Bilinear gather: weights (1-fx)(1-fy), fx(1-fy), (1-fx)fy, fx fy on
    O00, O01, O10, O11."""
    (o00, o01, o10, o11), fy, fx = _taps(psi, scan, pw)
    return ((1 - fx) * (1 - fy) * o00 + fx * (1 - fy) * o01
            + (1 - fx) * fy * o10 + fx * fy * o11)


def farplane(psi, probe, scan, det, norm="ortho"):
    """(N, S, det, det) complex128."""
    pw = probe.shape[-1]
    N, S = scan.shape[0], probe.shape[2]
    pad = (det - pw) // 2
    wave = patches(psi, scan, pw)[:, None] * probe[0, 0][None]
    near = torch.zeros((N, S, det, det), dtype=C128)
    near[:, :, pad:pad + pw, pad:pad + pw] = wave
    return torch.fft.fft2(near, norm=norm)


def intensity(psi, probe, scan, det, fly=1, norm="ortho"):
    """(N // fly, det, det) float64; differentiable by torch.autograd."""
    far = farplane(psi, probe, scan, det, norm)
    each = (far.real**2 + far.imag**2).sum(dim=1)
    return each.reshape(scan.shape[0] // fly, fly, det, det).sum(dim=1)


def autograd_gradients(psi, probe, scan, det, g, fly=1, norm="ortho"):
    """(intensity, psi.grad, probe.grad, scan.grad) of sum(g * intensity) by
    torch.autograd on the model."""
    psi, probe, scan = (x.detach().clone().requires_grad_(True)
                        for x in (psi, probe, scan))
    inten = intensity(psi, probe, scan, det, fly, norm)
    (inten * g).sum().backward()
    return inten.detach(), psi.grad, probe.grad, scan.grad


def forward_scale(det, norm):
    """The scale of the transform F; F^H is the unscaled inverse times it."""
    return {"ortho": 1.0 / det, "forward": 1.0 / (det * det),
            "backward": 1.0}[norm]


def scan_gradient(objproj, psi, scan):
    """(grad (N, 2), A (N, 2)) float64: sum_px Re((Dy, Dx) conj(objproj)) and
    the absolute-term sums sum_px (|Dy|, |Dx|) |objproj|."""
    pw = objproj.shape[-1]
    (o00, o01, o10, o11), fy, fx = _taps(psi, scan.detach(), pw)
    dy = (1 - fx) * (o10 - o00) + fx * (o11 - o01)
    dx = (1 - fy) * (o01 - o00) + fy * (o11 - o10)
    q = objproj.to(C128)
    grad = torch.stack([(dy * q.conj()).real.sum(dim=(1, 2)),
                        (dx * q.conj()).real.sum(dim=(1, 2))], dim=1)
    A = torch.stack([(dy.abs() * q.abs()).sum(dim=(1, 2)),
                     (dx.abs() * q.abs()).sum(dim=(1, 2))], dim=1)
    return grad, A


def hand_gradients(psi, probe, scan, det, g, fly=1, norm="ortho"):
    """The backward of tike_amd/autograd.py in float64, no autograd:
    dict(psi, probe, scan, A, objproj)."""
    with torch.no_grad():
        pw = probe.shape[-1]
        H, W = psi.shape[-2:]
        pad = (det - pw) // 2
        far = farplane(psi, probe, scan, det, norm)
        G = 2 * g.repeat_interleave(fly, dim=0)[:, None] * far
        back = torch.fft.ifft2(G, norm="forward") * forward_scale(det, norm)
        chi = back[:, :, pad:pad + pw, pad:pad + pw]
        patch = patches(psi, scan, pw)
        gprobe = (patch.conj()[:, None] * chi).sum(dim=0)[None, None]
        objproj = (probe[0, 0].conj()[None] * chi).sum(dim=1)
        # adjoint of the bilinear gather
        corner = torch.floor(scan)
        frac = scan - corner
        fy, fx = frac[:, 0, None, None], frac[:, 1, None, None]
        r = torch.arange(pw)
        yy = (corner[:, 0].long()[:, None, None] + r[None, :, None]).expand(
            -1, pw, pw)
        xx = (corner[:, 1].long()[:, None, None] + r[None, None, :]).expand(
            -1, pw, pw)
        gpsi = torch.zeros((H, W), dtype=C128)
        for dy, dx, w in ((0, 0, (1 - fx) * (1 - fy)), (0, 1, fx * (1 - fy)),
                          (1, 0, (1 - fx) * fy), (1, 1, fx * fy)):
            gpsi.index_put_((yy + dy, xx + dx), w * objproj, accumulate=True)
        gscan, A = scan_gradient(objproj, psi, scan)
    return dict(psi=gpsi[None], probe=gprobe, scan=gscan, A=A, objproj=objproj)


# ----------------------------------------------------------- position recovery
def amplitude_loss(inten, data):
    """The gaussian amplitude loss mean((sqrt(I) - sqrt(d))^2)."""
    return ((torch.sqrt(inten) - torch.sqrt(data))**2).mean()


def rms(scan, truth):
    """Root of the mean squared DISTANCE of a position from its truth."""
    d = np.asarray(scan, dtype=np.float64) - np.asarray(truth, dtype=np.float64)
    return float(np.sqrt(np.mean(np.sum(d * d, axis=-1))))


def problem(pw=32, H=96, fly=2, side=14, step=4, seed=0):
    """Smooth object (white noise under a gaussian filter of 3 px, in
    amplitude and in phase), one gaussian probe mode, a side x side raster of `step`
    pixels with a random sub-pixel offset per position, data from the true
    positions, start = truth +- 0.3 px uniform.  Host arrays:
    dict(psi, probe, scan_true, scan_start, data, det, fly)."""
    rng = np.random.default_rng(seed)
    smooth = lambda: gaussian_filter(rng.standard_normal((H, H)), 3.0)
    a, b = smooth(), smooth()
    psi = ((0.7 + 0.3 * a / np.abs(a).max()) * np.exp(
        0.8j * np.pi * b / np.abs(b).max()))[None].astype(np.complex64)
    c = np.arange(pw) - (pw - 1) / 2
    w = np.exp(-(c[:, None]**2 + c[None, :]**2) / (2 * (pw / 6.0)**2))
    probe = w[None, None, None].astype(np.complex64)
    ij = np.stack(np.meshgrid(np.arange(side), np.arange(side), indexing="ij"),
                  -1).reshape(-1, 2)
    truth = (4 + step * ij + rng.random(ij.shape)).astype(np.float32)
    start = (truth + rng.uniform(-0.3, 0.3, truth.shape)).astype(np.float32)
    with torch.no_grad():
        data = intensity(*as_model(psi, probe, truth), pw, fly).numpy()
    return dict(psi=psi, probe=probe, scan_true=truth, scan_start=start,
                data=data.astype(np.float32), det=pw, fly=fly)


def recover(cost_of, start, steps=40, lr=0.05):
    """`steps` of Adam(lr) on the positions alone; cost_of(scan) -> loss.
    Returns (final positions as a host array, [cost per step])."""
    scan = start.detach().clone().requires_grad_(True)
    opt = torch.optim.Adam([scan], lr=lr)
    costs = []
    for _ in range(steps):
        opt.zero_grad()
        loss = cost_of(scan)
        loss.backward()
        opt.step()
        costs.append(float(loss.detach()))
    return scan.detach().cpu().numpy(), costs
