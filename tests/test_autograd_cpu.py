"""The differentiable intensity model without a GPU: the float64 model
(tests/autograd_model.py) against the oracle, its hand formulas against
torch.autograd and a finite difference, every refusal of
`tike_amd.autograd.intensity`, the two new ABI entries, and position recovery
on the model."""
import ctypes

import numpy as np
import pytest
import torch

import autograd_model as am

# (N, S, pw, det, H, W, fly): odd sizes, probe window < detector, fly 1, 2, 3
SHAPES = [(6, 2, 8, 12, 24, 31, 1), (8, 3, 16, 16, 40, 37, 2),
          (12, 1, 13, 20, 37, 45, 3)]


def case(N, S, pw, det, H, W, fly, seed=0):
    """float32 / complex64 host arrays: psi, probe, scan, and a signed
    upstream gradient g (N // fly, det, det)."""
    rng = np.random.default_rng(seed + 7 * det + N)
    rc = lambda *s: (rng.standard_normal(s) + 1j * rng.standard_normal(s)
                     ).astype(np.complex64)
    psi, probe = rc(1, H, W), rc(1, 1, S, pw, pw)
    scan = np.stack([1 + rng.random(N) * (H - pw - 2),
                     1 + rng.random(N) * (W - pw - 2)], 1).astype(np.float32)
    g = rng.standard_normal((N // fly, det, det)).astype(np.float32)
    return psi, probe, scan, g


def rel(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def _oracle_intensity(psi, probe, scan, det, fly):
    from oracle import operators as oracle
    far = oracle.ptycho_fwd(probe, scan, psi, det)
    return oracle.intensity_from_farplane(far).reshape(
        scan.shape[0] // fly, fly, det, det).sum(axis=1)


# (N, S, pw, H, W, fly) at det = 4
EXACT_SHAPES = [(6, 2, 2, 9, 11, 1), (8, 3, 4, 12, 10, 2), (9, 1, 3, 11, 13, 3)]


@pytest.mark.parametrize("shape", EXACT_SHAPES)
def test_model_intensity_equals_the_oracle_exactly(shape):
    """To 1e-12 against `oracle.operators` (ptycho_fwd +
    intensity_from_farplane, frames summed).  The oracle rounds to float32 at
    every step, so the bar can only be met where float32 is exact: object and
    probe values in {-1, 0, 1} + i {-1, 0, 1}, fractions 0 or 1/2 (weights in
    quarters) and a 4 x 4 detector, whose transform multiplies by +-1, +-i and
    1/4 alone -- every intermediate is a small multiple of a power of two.
    The gather's taps and weights, the probe product, the centred padding
    (pw 2 and 3 in 4), the transform's axes and norm, and the sums over modes
    and fly positions are all in play."""
    N, S, pw, H, W, fly = shape
    det = 4
    rng = np.random.default_rng(N)
    ri = lambda *s: (rng.integers(-1, 2, s) + 1j * rng.integers(-1, 2, s)
                     ).astype(np.complex64)
    psi, probe = ri(1, H, W), ri(1, 1, S, pw, pw)
    scan = np.stack([rng.integers(1, H - pw, N) + rng.integers(0, 2, N) / 2,
                     rng.integers(1, W - pw, N) + rng.integers(0, 2, N) / 2],
                    1).astype(np.float32)
    got = am.intensity(*am.as_model(psi, probe, scan), det, fly).numpy()
    want = _oracle_intensity(psi, probe, scan, det, fly)
    assert np.abs(want).max() > 1
    assert rel(got, want) < 1e-12


@pytest.mark.parametrize("shape", SHAPES)
def test_model_intensity_equals_the_oracle(shape):
    """Random data: against the oracle within the oracle's own float32
    rounding (the project's operator bar), and to 1e-12 against the same
    steps in float64 NumPy, independent of torch."""
    N, S, pw, det, H, W, fly = shape
    psi, probe, scan, _ = case(*shape)
    got = am.intensity(*am.as_model(psi, probe, scan), det, fly).numpy()
    assert rel(got, _oracle_intensity(psi, probe, scan, det, fly)) < 1e-5
    sy, sx = np.floor(scan[:, 0]).astype(int), np.floor(scan[:, 1]).astype(int)
    fy = (scan[:, 0] - np.floor(scan[:, 0])).astype(np.float64)[:, None, None]
    fx = (scan[:, 1] - np.floor(scan[:, 1])).astype(np.float64)[:, None, None]
    r = np.arange(pw)
    yy = sy[:, None, None] + r[None, :, None]
    xx = sx[:, None, None] + r[None, None, :]
    img = psi[0].astype(np.complex128)
    patch = ((1 - fx) * (1 - fy) * img[yy, xx] + fx * (1 - fy) * img[yy, xx + 1]
             + (1 - fx) * fy * img[yy + 1, xx] + fx * fy * img[yy + 1, xx + 1])
    pad = (det - pw) // 2
    near = np.zeros((N, S, det, det), np.complex128)
    near[:, :, pad:pad + pw, pad:pad + pw] = patch[:, None] * probe[0, 0][None]
    want = (np.abs(np.fft.fft2(near, norm="ortho"))**2).sum(axis=1).reshape(
        N // fly, fly, det, det).sum(axis=1)
    assert rel(got, want) < 1e-12


@pytest.mark.parametrize("norm", ["ortho", "backward", "forward"])
@pytest.mark.parametrize("shape", SHAPES)
def test_hand_formulas_equal_torch_autograd(shape, norm):
    N, S, pw, det, H, W, fly = shape
    psi, probe, scan, g = case(*shape)
    m = am.as_model(psi, probe, scan)
    gt = torch.from_numpy(g).to(am.F64)
    _, gpsi, gprobe, gscan = am.autograd_gradients(*m, det, gt, fly, norm)
    hand = am.hand_gradients(*m, det, gt, fly, norm)
    assert rel(hand["psi"], gpsi) < 1e-12
    assert rel(hand["probe"], gprobe) < 1e-12
    assert rel(hand["scan"], gscan) < 1e-12
    # the terms cancel: the sums are far below their absolute terms
    assert np.all(hand["scan"].abs().numpy() <= hand["A"].numpy())


@pytest.mark.parametrize("shape", SHAPES)
def test_scan_gradient_equals_a_finite_difference(shape):
    N, S, pw, det, H, W, fly = shape
    psi, probe, scan, g = case(*shape)
    mpsi, mprobe, mscan = am.as_model(psi, probe, scan)
    gt = torch.from_numpy(g).to(am.F64)
    grad = am.hand_gradients(mpsi, mprobe, mscan, det, gt, fly)["scan"]
    h = 1e-6
    # (fractions in (h, 1 - h): the step crosses no integer)
    frac = mscan - torch.floor(mscan)
    assert float(frac.min()) > h and float(frac.max()) < 1 - h
    fd = torch.zeros_like(mscan)
    with torch.no_grad():
        for n in range(N):
            for k in range(2):
                d = torch.zeros_like(mscan)
                d[n, k] = h
                up = (am.intensity(mpsi, mprobe, mscan + d, det, fly) * gt).sum()
                dn = (am.intensity(mpsi, mprobe, mscan - d, det, fly) * gt).sum()
                fd[n, k] = (up - dn) / (2 * h)
    assert rel(grad, fd) < 1e-5


# ------------------------------------------------------------------ refusals
def test_every_refusal():
    """The argument checks come before any device work: CPU tensors reach
    every one of them, and are themselves refused last."""
    import tike_amd.operators as ops
    from tike_amd.autograd import MAX_MODES, intensity
    pw, det, H, W, N = 8, 12, 24, 31, 6
    psi = torch.zeros((1, H, W), dtype=torch.complex64)
    probe = torch.zeros((1, 1, 2, pw, pw), dtype=torch.complex64)
    scan = torch.full((N, 2), 3.5)
    with ops.Ptycho(probe_shape=pw, detector_shape=det, nz=H, n=W) as op:
        with pytest.raises(NotImplementedError, match="several slices"):
            intensity(op, psi.expand(2, H, W), probe, scan)
        with pytest.raises(NotImplementedError, match="probe per position"):
            intensity(op, psi, probe.expand(N, 1, 2, pw, pw), scan)
        with pytest.raises(TypeError, match="psi must be a torch"):
            intensity(op, psi.numpy(), probe, scan)
        with pytest.raises(TypeError, match="scan must be a torch"):
            intensity(op, psi, probe, scan.numpy())
        with pytest.raises(TypeError, match="probe must be torch.complex64"):
            intensity(op, psi, probe.to(torch.complex128), scan)
        with pytest.raises(TypeError, match="scan must be torch.float32"):
            intensity(op, psi, probe, scan.to(torch.float64))
        with pytest.raises(ValueError, match="not a multiple of fly=4"):
            intensity(op, psi, probe, scan, fly=4)
        many = torch.zeros((1, 1, MAX_MODES + 1, pw, pw), dtype=torch.complex64)
        with pytest.raises(ValueError, match=f"at most {MAX_MODES}"):
            intensity(op, psi, many, scan)
        for bad in ((0.5, 3.0), (3.0, W - pw + 0.5)):
            outside = scan.clone()
            outside[2] = torch.tensor(bad)
            with pytest.raises(ValueError, match="Scan positions must be >= 1"):
                intensity(op, psi, probe, outside)
            # unchecked, the call goes on to the next refusal
            with pytest.raises(TypeError, match="no CPU fallback"):
                intensity(op, psi, probe, outside, check_positions=False)
        with pytest.raises(TypeError, match="no CPU fallback"):
            intensity(op, psi, probe, scan)


# ------------------------------------------------------------------- the ABI
def test_abi_has_the_new_entries():
    """Fails on the parent commit: the symbols do not exist."""
    import tike_amd._lib as L
    for name, arity in (("tike_farplane_scale", 7), ("tike_scan_gradient", 9)):
        assert name in L.declared_symbols()
        assert len(L._PROTOTYPES[name]) == arity
        assert hasattr(ctypes.CDLL(L.LIB_PATH), name)
    assert L.ABI_VERSION >= 19
    assert "autograd.hip" in open(
        L.LIB_PATH.replace("libtike_amd.so", "Makefile")).read()


def _calls(fn, ok):
    def call(**change):
        args = list(ok)
        for k, v in change.items():
            args[int(k[1:])] = v
        return fn(*args)
    return call


def test_abi_entries_check_their_arguments_without_a_gpu():
    """Argument checks come before any launch.  Fails on the parent commit."""
    import tike_amd._lib as L
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p)
    # (farplane, table, nframe, P, npix, scale, stream)
    call = _calls(L.lib.tike_farplane_scale, (p, p, 1, 2, 4, 1.0, None))
    assert call(a0=None) == L.ERR_ARG  # farplane
    assert call(a1=None) == L.ERR_ARG  # table
    assert call(a2=-1) == L.ERR_ARG  # nframe
    assert call(a3=0) == L.ERR_ARG  # P
    assert call(a4=0) == L.ERR_ARG  # npix
    assert call(a2=0) == 0  # no frame: no launch
    # (objproj, scan, psi, grad, nscan, pw, H, W, stream)
    call = _calls(L.lib.tike_scan_gradient, (p, p, p, p, 1, 2, 4, 4, None))
    for k in range(4):
        assert call(**{f"a{k}": None}) == L.ERR_ARG  # a NULL array
    assert call(a4=-1) == L.ERR_ARG  # nscan
    assert call(a4=1 << 31) == L.ERR_ARG  # more than grid.x holds
    assert call(a5=0) == L.ERR_ARG  # pw
    assert call(a6=0) == L.ERR_ARG  # H
    assert call(a7=0) == L.ERR_ARG  # W
    assert call(a4=0) == 0  # no position: no launch


# --------------------------------------------------------- position recovery
def test_model_recovers_the_positions():
    """40 steps of Adam(lr=0.05) on the positions alone, fly = 2: the RMS
    position error falls to 0.15 of its start or less (0.08 - 0.10 measured on
    the model when the bar was set) and the cost below 1 % of its start."""
    p = am.problem()
    psi, probe, truth = am.as_model(p["psi"], p["probe"], p["scan_true"])
    data = torch.from_numpy(p["data"]).to(am.F64)
    start = torch.from_numpy(p["scan_start"]).to(am.F64)
    final, costs = am.recover(
        lambda s: am.amplitude_loss(
            am.intensity(psi, probe, s, p["det"], p["fly"]), data), start)
    r0, r1 = am.rms(p["scan_start"], p["scan_true"]), am.rms(
        final, p["scan_true"])
    print(f"rms {r0:.3f} -> {r1:.3f}, cost {costs[0]:.2e} -> {costs[-1]:.2e}")
    assert r1 <= 0.15 * r0, (r0, r1)
    assert costs[-1] < 0.01 * costs[0], (costs[0], costs[-1])
