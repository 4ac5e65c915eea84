"""Float64 model of `tike_amd.autograd.intensity` with eigen probes (test
infrastructure), on `autograd_model`.

`intensity` restates the forward model with the varying probe of the
reference's `get_varying_probe` in complex128 torch on the CPU, so that its
gradients come from `torch.autograd` itself.  `entry_model` holds the formulas
of `tike_eigen_probe_gradients` on a given chi, `hand_gradients` the whole
backward of tike_amd/autograd.py with them, both with the absolute-term sums
A[n,c,s] = sum_px |B_{c,s}| |q[n,s]| the weight-gradient bars are stated in
(B_{0,s} = probe[s], B_{c+1,s} = eigen[c,s]).  `problem` / `recover`: recovery
of the eigen weights of a drifting probe on fly-scan data.
"""
import functools

import numpy as np
import torch

import autograd_model as am

C128, F64 = am.C128, am.F64

# (nscan, S, M, C, pw, H, W): tike_eigen_probe_gradients alone
ENTRY_CASES = [(5, 1, 1, 1, 15, 40, 40), (6, 3, 2, 2, 16, 48, 50),
               (7, 2, 0, 0, 20, 48, 48), (4, 2, 1, 1, 100, 240, 240),
               (3, 16, 16, 1, 16, 40, 40), (4, 8, 8, 2, 32, 80, 80)]
# The kernel of a shape (csrc/autograd_eigen.hip): S in 1 ... 6 and 8 without
# an eigen probe or with ONE on mode 0 is compiled for its counts; everything
# else runs the general kernel of the smallest bounds (SB, EB), each 4, 8 or
# 16, that hold S and C M.  ENTRY_CASES reaches <1,1>, <2,0>, <2,1> and the
# general kernels (4,4), (16,16), (8,16); these reach every other
# instantiation, and more than one chunk of positions (grid.y) together with
# more than one pixel tile (pw = 20: two tiles): a position chunk holds
# 64 (S + C M) / S positions, rounded up to eight -- 72 at (8, 1, 1): three
# chunks of 200; 152 at (3, 2, 2): two of 300; 144 at (5, 2, 3): two of 150;
# 384 at (2, 5, 2): two of 400.
ENTRY_CASES_EVERY_KERNEL = (
    [(5, S, 0, 0, 16, 40, 44) for S in (1, 3, 4, 5, 6, 8)]
    + [(5, S, 1, 1, 17, 40, 44) for S in (3, 4, 5, 6, 8)]
    + [(200, 8, 1, 1, 20, 48, 52), (130, 4, 0, 0, 20, 48, 52),
       (300, 3, 2, 2, 20, 48, 52),  # general (4, 4)
       (4, 4, 4, 2, 16, 40, 44),  # general (4, 8)
       (400, 2, 2, 5, 20, 48, 52),  # general (4, 16)
       (5, 6, 1, 2, 16, 40, 44),  # general (8, 4)
       (150, 5, 2, 3, 20, 48, 52),  # general (8, 8)
       (5, 9, 1, 2, 16, 40, 44),  # general (16, 4)
       (5, 10, 3, 2, 16, 40, 44)])  # general (16, 8)
# (N, S, M, C, pw, det, H, fly): end to end through `intensity`
END_TO_END_CASES = [(6, 3, 2, 2, 16, 20, 48, 2), (5, 1, 1, 1, 15, 15, 40, 1),
                    (4, 2, 1, 1, 100, 128, 240, 2), (4, 8, 8, 2, 32, 32, 80, 1)]
# the c3 configuration (8 modes + one eigen probe), 4 modes without an eigen
# probe, and 2 eigen probes on all of 4 modes (general kernel), end to end
END_TO_END_CASES_MORE = [(6, 8, 1, 1, 16, 16, 48, 2), (6, 4, 0, 0, 16, 20, 48, 1),
                         (4, 4, 4, 2, 20, 20, 48, 2)]
WEIGHTS_ENTRY_BAR = 1e-7  # x A: the bar of tike_scan_gradient alone
WEIGHTS_BAR = 1e-6  # x A, end to end
SCAN_BAR = 1e-6  # x A_n, end to end


def rc(rng, *s):
    return (rng.standard_normal(s) + 1j * rng.standard_normal(s)).astype(
        np.complex64)


def rel(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def t128(a):
    """A float32 / complex64 host array (or None) as the model's float64
    tensor: the float32 VALUES."""
    if a is None:
        return None
    a = torch.from_numpy(np.asarray(a))
    return a.to(C128 if a.is_complex() else F64)


def varying_probe(probe, eigen, weights):
    """(N, S, pw, pw): w[n,0,s] probe[s] + sum_c w[n,c+1,s] eigen[c,s] for
    s < M, the first term alone for s >= M.  probe (1, 1, S, pw, pw), eigen
    (1, C, M, pw, pw) or None, weights (N, C + 1, S)."""
    P = weights[:, 0, :, None, None] * probe[0, 0][None]
    if eigen is None:
        return P
    M = eigen.shape[2]
    extra = (weights[:, 1:, :M, None, None] * eigen[0][None]).sum(dim=1)
    return torch.cat([P[:, :M] + extra, P[:, M:]], dim=1)


def farplane(psi, probe, scan, eigen, weights, det, norm="ortho"):
    """(N, S, det, det) complex128."""
    P = varying_probe(probe, eigen, weights)
    pw = P.shape[-1]
    pad = (det - pw) // 2
    wave = am.patches(psi, scan, pw)[:, None] * P
    near = torch.zeros(P.shape[:2] + (det, det), dtype=wave.dtype)
    near[:, :, pad:pad + pw, pad:pad + pw] = wave
    return torch.fft.fft2(near, norm=norm)


def intensity(psi, probe, scan, eigen, weights, det, fly=1, norm="ortho"):
    """(N // fly, det, det) float64; differentiable by torch.autograd."""
    far = farplane(psi, probe, scan, eigen, weights, det, norm)
    each = (far.real**2 + far.imag**2).sum(dim=1)
    return each.reshape(scan.shape[0] // fly, fly, det, det).sum(dim=1)


def autograd_gradients(psi, probe, scan, eigen, weights, det, g, fly=1,
                       norm="ortho"):
    """dict(intensity, psi, probe, scan, eigen, weights) of sum(g * intensity)
    by torch.autograd on the model (eigen: None when there is none)."""
    leaf = lambda x: None if x is None else x.detach().clone().requires_grad_(
        True)
    psi, probe, scan, eigen, weights = map(leaf, (psi, probe, scan, eigen,
                                                  weights))
    inten = intensity(psi, probe, scan, eigen, weights, det, fly, norm)
    (inten * g).sum().backward()
    return dict(intensity=inten.detach(), psi=psi.grad, probe=probe.grad,
                scan=scan.grad, eigen=None if eigen is None else eigen.grad,
                weights=weights.grad)


def entry_model(chi, psi, probe, eigen, weights, scan, single=False):
    """The outputs of tike_eigen_probe_gradients from chi (N, S, pw, pw):
    dict(probe (1,1,S,pw,pw), eigen (1,C,M,pw,pw) or None, weights (N,C+1,S),
    A like weights, objproj (N,pw,pw)) in float64.  single: the patch, q and
    every term in float32 / complex64, the SUMS of the weight gradient in
    float64 -- what the kernel's arithmetic is held to."""
    with torch.no_grad():
        ct, ft = (torch.complex64, torch.float32) if single else (C128, F64)
        chi, psi, probe, weights, scan = (chi.to(ct), psi.to(ct),
                                          probe.to(ct), weights.to(ft),
                                          scan.to(ft))
        eigen = None if eigen is None else eigen.to(ct)
        pw = probe.shape[-1]
        q = am.patches(psi, scan, pw).conj()[:, None] * chi  # (N, S, pw, pw)
        gprobe = (weights[:, 0, :, None, None] * q).sum(dim=0)[None, None]
        term = (probe[0, 0].conj()[None] * q).real.to(F64)
        gw = torch.zeros(weights.shape, dtype=F64)
        A = torch.zeros(weights.shape, dtype=F64)
        gw[:, 0] = term.sum(dim=(-2, -1))
        A[:, 0] = (probe[0, 0].abs()[None] * q.abs()).to(F64).sum(dim=(-2, -1))
        geigen = None
        if eigen is not None:
            M = eigen.shape[2]
            qm = q[:, None, :M]  # (N, 1, M, pw, pw)
            geigen = (weights[:, 1:, :M, None, None] * qm).sum(dim=0)[None]
            gw[:, 1:, :M] = (eigen[0].conj()[None] * qm).real.to(F64).sum(
                dim=(-2, -1))
            A[:, 1:, :M] = (eigen[0].abs()[None] * qm.abs()).to(F64).sum(
                dim=(-2, -1))
        P = varying_probe(probe, eigen, weights)
        objproj = (P.conj() * chi).sum(dim=1)
    return dict(probe=gprobe, eigen=geigen, weights=gw, A=A, objproj=objproj)


def _scatter(objproj, scan, H, W):
    """Adjoint of the bilinear gather: (H, W)."""
    pw = objproj.shape[-1]
    corner = torch.floor(scan)
    frac = scan - corner
    fy, fx = frac[:, 0, None, None], frac[:, 1, None, None]
    r = torch.arange(pw)
    yy = (corner[:, 0].long()[:, None, None] + r[None, :, None]).expand(
        -1, pw, pw)
    xx = (corner[:, 1].long()[:, None, None] + r[None, None, :]).expand(
        -1, pw, pw)
    out = torch.zeros((H, W), dtype=objproj.dtype)
    for dy, dx, w in ((0, 0, (1 - fx) * (1 - fy)), (0, 1, fx * (1 - fy)),
                      (1, 0, (1 - fx) * fy), (1, 1, fx * fy)):
        out.index_put_((yy + dy, xx + dx), w * objproj, accumulate=True)
    return out


def hand_gradients(psi, probe, scan, eigen, weights, det, g, fly=1,
                   norm="ortho", single=False):
    """The backward of tike_amd/autograd.py with eigen probes, no autograd:
    dict(psi, probe, scan, eigen, weights, A (weights), A_scan, objproj).
    single: the whole chain in complex64 / float32 with the weight and scan
    SUMS in float64, as the kernels have it."""
    with torch.no_grad():
        ct, ft = (torch.complex64, torch.float32) if single else (C128, F64)
        cast = lambda x, t: None if x is None else x.to(t)
        psi, probe, eigen = cast(psi, ct), cast(probe, ct), cast(eigen, ct)
        scan, weights, g = cast(scan, ft), cast(weights, ft), cast(g, ft)
        pw = probe.shape[-1]
        H, W = psi.shape[-2:]
        pad = (det - pw) // 2
        far = farplane(psi, probe, scan, eigen, weights, det, norm)
        G = 2 * g.repeat_interleave(fly, dim=0)[:, None] * far
        back = torch.fft.ifft2(G, norm="forward") * am.forward_scale(det, norm)
        chi = back[:, :, pad:pad + pw, pad:pad + pw]
        out = entry_model(chi, psi, probe, eigen, weights, scan, single)
        out["psi"] = _scatter(out["objproj"], scan, H, W)[None]
        out["scan"], out["A_scan"] = am.scan_gradient(
            out["objproj"], psi.to(C128), scan.to(F64))
    return out


# ------------------------------------------------------------------ the inputs
def inputs(N, S, M, C, pw, H, W, seed, edges=False):
    """Host arrays dict(psi, probe, scan, eigen (None for C = 0), weights):
    psi, probe and positions as `_case` of test_autograd_gpu.py (edges: the
    positions of its `_edge_positions`, whose footprints touch the object's
    edge); eigen probes 0.3 x complex normal; weights row 0 = 1 + 0.1 normal,
    the other rows 0.5 normal."""
    rng = np.random.default_rng(seed)
    psi, probe = rc(rng, 1, H, W), rc(rng, 1, 1, S, pw, pw)
    if edges:
        frac = lambda *s: 0.05 + 0.9 * rng.random(s)
        scan = np.stack([rng.integers(1, H - pw, N) + frac(N),
                         rng.integers(1, W - pw, N) + frac(N)], 1)
        scan[0] = (1.0, 1 + frac())
        scan[1] = (H - pw - 1 + frac(), W - pw - 1 + frac())
        scan = scan.astype(np.float32)
        assert tuple(np.floor(scan[0])) == (1, 1)
        assert tuple(np.floor(scan[1])) == (H - pw - 1, W - pw - 1)
    else:
        scan = np.stack([1 + rng.random(N) * (H - pw - 1),
                         1 + rng.random(N) * (W - pw - 1)],
                        1).astype(np.float32)
    eigen = (0.3 * rc(rng, 1, C, M, pw, pw)).astype(
        np.complex64) if C else None
    weights = 0.5 * rng.standard_normal((N, C + 1, S))
    weights[:, 0] = 1 + 0.1 * rng.standard_normal((N, S))
    return dict(psi=psi, probe=probe, scan=scan, eigen=eigen,
                weights=weights.astype(np.float32))


def model_of(c):
    """The five model tensors of a case, in the model's argument order."""
    return (t128(c["psi"]), t128(c["probe"]), t128(c["scan"]),
            t128(c["eigen"]), t128(c["weights"]))


@functools.lru_cache(maxsize=None)
def entry_case(nscan, S, M, C, pw, H, W):
    """Inputs of an ENTRY_CASES shape with a random float32 chi and the
    model's outputs on it -- computed once, shared, left unchanged."""
    c = inputs(nscan, S, M, C, pw, H, W, seed=nscan + 3 * S + 5 * pw,
               edges=True)
    c["chi"] = rc(np.random.default_rng(7 + nscan + pw), nscan, S, pw, pw)
    psi, probe, scan, eigen, weights = model_of(c)
    want = entry_model(t128(c["chi"]), psi, probe, eigen, weights, scan)
    c["want"] = {k: None if v is None else v.numpy() for k, v in want.items()}
    return c


@functools.lru_cache(maxsize=None)
def case(N, S, M, C, pw, det, H, fly, norm="ortho"):
    """Inputs of an END_TO_END_CASES shape with a random signed upstream
    gradient, and the model's intensity and hand gradients -- computed once,
    shared, left unchanged."""
    c = inputs(N, S, M, C, pw, H, H, seed=N + 3 * S + 5 * det)
    rng = np.random.default_rng(11 + N + det)
    c["g"] = rng.standard_normal((N // fly, det, det)).astype(np.float32)
    m = model_of(c)
    with torch.no_grad():
        c["intensity"] = intensity(*m, det, fly, norm).numpy()
    hand = hand_gradients(*m, det, t128(c["g"]), fly, norm)
    c["want"] = {k: None if v is None else v.numpy() for k, v in hand.items()}
    return c


# ------------------------------------------------------------ weight recovery
RECOVERY = dict(steps=60, lr=0.05, rms=0.35, cost=0.01)


def problem(seed=0):
    """`autograd_model.problem(seed)` (14 x 14 raster, pw = det = 32, fly = 2)
    with ONE eigen probe on its single mode: the probe times the column
    coordinate (x - (pw - 1) / 2) / (pw / 6), scaled to the probe's norm -- a
    probe that drifts sideways.  True weights: row 0 = 1, row 1 uniform in
    +-0.3; data from the model at the true positions; start: row 0 = 1, row
    1 = 0.  Host arrays: the keys of `autograd_model.problem` and eigen,
    weights_true, weights_start."""
    p = am.problem(seed=seed)
    pw = p["det"]
    probe = p["probe"]
    x = (np.arange(pw) - (pw - 1) / 2) / (pw / 6.0)
    eigen = probe[0, 0] * x[None, None, :]
    eigen = eigen * (np.linalg.norm(probe) / np.linalg.norm(eigen))
    N = p["scan_true"].shape[0]
    rng = np.random.default_rng(100)
    w = np.ones((N, 2, 1), dtype=np.float32)
    w[:, 1, 0] = rng.uniform(-0.3, 0.3, N)
    start = np.ones((N, 2, 1), dtype=np.float32)
    start[:, 1] = 0
    p["eigen"] = eigen[None, None].astype(np.complex64)  # (1, C, M, pw, pw)
    p["weights_true"], p["weights_start"] = w, start
    with torch.no_grad():
        p["data"] = intensity(t128(p["psi"]), t128(p["probe"]),
                              t128(p["scan_true"]), t128(p["eigen"]), t128(w),
                              pw, p["fly"]).numpy().astype(np.float32)
    return p


def weights_rms(w, truth):
    """Root of the mean squared error over ALL weight entries."""
    d = np.asarray(w, dtype=np.float64) - np.asarray(truth, dtype=np.float64)
    return float(np.sqrt(np.mean(d * d)))


def recover(cost_of, start, steps=RECOVERY["steps"], lr=RECOVERY["lr"]):
    """`steps` of Adam(lr) on the weights alone; cost_of(weights) -> loss.
    Returns (final weights as a host array, [cost per step])."""
    w = start.detach().clone().requires_grad_(True)
    opt = torch.optim.Adam([w], lr=lr)
    costs = []
    for _ in range(steps):
        opt.zero_grad()
        loss = cost_of(w)
        loss.backward()
        opt.step()
        costs.append(float(loss.detach()))
    return w.detach().cpu().numpy(), costs
