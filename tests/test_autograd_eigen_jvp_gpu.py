"""The forward-mode derivative of `tike_amd.autograd.intensity` with eigen
probes on the GPU against the float64 model (tests/autograd_eigen_jvp.py):
`tike_eigen_wave_tangent` on its own, `eigen_intensity_jvp` end to end and cut
into chunks, the adjoint identity between the forward and the reverse mode,
`eigen_gauss_newton_product`, the refusals that stay, and joint
Levenberg-Marquardt recovery of positions and eigen weights.

Every figure a bar is set on is printed before it is asserted."""
import numpy as np
import pytest

import autograd_eigen as ae
import autograd_eigen_jvp as ej
import autograd_jvp as aj
import autograd_model as am
from util import OP_MAXABS, OP_NORMWISE, assert_close, maxerr, relerr

pytestmark = pytest.mark.gpu

SENTINEL = complex(7e30, -7e30)


# --------------------------------------------- the entry alone
# (pw, det, S, M, C, N): tiny; odd det - pw, M < S and two eigen probes; C = 0
# with eigen_probe NULL and an odd size; exactly one full item (the halo
# column lies outside the window); a second column segment of one column and
# items that lie in the padding altogether; the limits of S and C M; the
# headline counts
ENTRY_CASES = [(5, 5, 1, 1, 1, 3), (15, 20, 3, 2, 2, 7), (33, 33, 2, 0, 0, 5),
               (64, 64, 1, 1, 1, 4), (65, 128, 2, 2, 1, 3),
               (16, 16, 16, 16, 1, 3), (128, 128, 8, 1, 1, 2)]


def _entry_inputs(pw, det, S, M, C, N):
    """Host arrays at positions on the object's edges, with five tangents."""
    H, W = pw + 9, pw + 12
    c = ae.inputs(N, S, M, C, pw, H, W, seed=pw + det + S, edges=True)
    c.update(ej.tangents(c, seed=3 + pw + det + S))
    return c, H, W


def _call_entry(c, shape, H, W, names, buf):
    """One call of tike_eigen_wave_tangent into `buf` (device, with a guard
    row behind the planes); the tangents not in `names` are NULL.  C = 0:
    eigen_probe is NULL, and a d_eigen in `names` is a pointer the entry must
    ignore."""
    import torch

    from tike_amd import _arrays as A
    from tike_amd._lib import check, lib
    pw, det, S, M, C, N = shape
    on = {k: None if v is None else torch.from_numpy(
        np.ascontiguousarray(v)).to(buf.device) for k, v in c.items()}
    if C == 0:
        on["d_eigen"] = on["d_probe"]  # (never read)
    ptr = lambda k: A.ptr(on[k]) if k in names else None
    check(lib.tike_eigen_wave_tangent(
        A.ptr(on["psi"]), ptr("d_psi"), A.ptr(on["scan"]), ptr("d_scan"),
        A.ptr(on["probe"]), ptr("d_probe"), A.ptr(on["eigen"]), ptr("d_eigen"),
        A.ptr(on["weights"]), ptr("d_weights"), C, M, A.ptr(buf), N, S, pw,
        det, H, W, A.stream_ptr()), "tike_eigen_wave_tangent")
    return buf.cpu().numpy()


def _check_entry(c, shape, H, W, what):
    """Every tangent subset of a case against `tangent_nearplane`."""
    import torch
    pw, det, S, M, C, N = shape
    m = ae.model_of(c)
    pad = (det - pw) // 2
    window = np.zeros((det, det), bool)
    window[pad:pad + pw, pad:pad + pw] = True
    count = N * S * det * det
    buf = torch.empty(count + det, dtype=torch.complex64, device="cuda")
    for names in ej.TANGENTS + [()]:
        live = tuple(k for k in names if c[k] is not None)
        want = ej.tangent_nearplane(*m, det, **ej.model_tangents(
            c, live)).numpy()
        buf.fill_(SENTINEL)
        got = _call_entry(c, shape, H, W, names, buf)
        # nothing behind the planes; every element written; the padding 0.0
        assert np.all(got[count:] == np.complex64(SENTINEL)), names
        got = got[:count].reshape(N, S, det, det)
        assert np.all(got.view(np.float32).reshape(N, S, det, det, 2)[
            :, :, ~window] == 0.0), names
        print(f"{what} {shape} {names}: normwise {relerr(got, want):.2e} "
              f"max-abs {maxerr(got, want):.2e}")
        if live:
            assert np.abs(want).max() > 0
            assert_close(got, want, OP_NORMWISE, OP_MAXABS, str(names))
        else:  # no tangent (or only the one C = 0 ignores): zeros, written
            assert not got.any()
        buf.fill_(SENTINEL)  # no atomics: a second call gives the same bits
        again = _call_entry(c, shape, H, W, names, buf)[:count]
        assert np.array_equal(again.view(np.float32),
                              got.ravel().view(np.float32)), names


@pytest.mark.parametrize("shape", ENTRY_CASES)
def test_eigen_wave_tangent_vs_float64_model(shape):
    """Entry by entry within the operator bars (normwise 1e-5, max-abs 1e-4 of
    the largest entry) for each of the five tangents alone -- the others NULL
    --, all five and none, at positions on the object's edges; the padding
    exactly 0.0; every element written (the buffer starts as a sentinel) and
    nothing behind the planes (a guard row keeps its sentinel); all NULL gives
    all zeros; a second call gives the same bits."""
    c, H, W = _entry_inputs(*shape)
    _check_entry(c, shape, H, W, "eigen tangent")


def test_weight_rows_of_modes_without_an_eigen_probe_are_not_used():
    """M < S: rows c + 1 of w and dw hold 1e30 in the modes s >= M; those
    modes still match the model, which ignores the rows."""
    shape = ENTRY_CASES[1]
    pw, det, S, M, C, N = shape
    assert 0 < M < S
    c, H, W = _entry_inputs(*shape)
    for k in ("weights", "d_weights"):
        c[k] = c[k].copy()
        c[k][:, 1:, M:] = 1e30
    _check_entry(c, shape, H, W, "eigen tangent, 1e30 in the unused rows")


def test_eigen_wave_tangent_argument_errors_launch_nothing():
    """TIKE_ERR_ARG / TIKE_ERR_UNSUPPORTED for what include/tike_amd.h lists,
    on device buffers: the plane keeps its sentinel."""
    import torch

    from tike_amd import _arrays as A
    from tike_amd._lib import ERR_ARG, ERR_UNSUPPORTED, lib
    shape = pw, det, S, M, C, N = 5, 8, 2, 1, 1, 3
    c, H, W = _entry_inputs(*shape)
    dev = torch.device("cuda")
    on = {k: torch.from_numpy(v).to(dev) for k, v in c.items()}
    buf = torch.full((N * S * det * det,), SENTINEL, dtype=torch.complex64,
                     device=dev)
    p = lambda k: A.ptr(on[k])
    ok = [p("psi"), p("d_psi"), p("scan"), p("d_scan"), p("probe"),
          p("d_probe"), p("eigen"), p("d_eigen"), p("weights"),
          p("d_weights"), C, M, A.ptr(buf), N, S, pw, det, H, W,
          A.stream_ptr()]

    def call(**change):
        args = list(ok)
        for k, v in change.items():
            args[int(k[1:])] = v
        return lib.tike_eigen_wave_tangent(*args)

    for k in (0, 2, 4, 8, 12):
        assert call(**{f"a{k}": None}) == ERR_ARG  # a NULL required array
    assert call(a6=None) == ERR_ARG  # eigen_probe NULL with C > 0
    assert call(a11=0) == ERR_ARG  # M < 1 with C > 0
    assert call(a11=S + 1) == ERR_ARG  # M > S with C > 0
    for k in (10, 11, 13):
        assert call(**{f"a{k}": -1}) == ERR_ARG  # negative counts
    for k in (14, 15, 17, 18):
        assert call(**{f"a{k}": 0}) == ERR_ARG  # S, pw, H, W
    assert call(a16=pw - 1) == ERR_ARG  # det < pw
    assert call(a13=1 << 31) == ERR_ARG  # nscan > 2^31 - 1
    # more items than one launch holds: ceil(det / 64) ceil(det / 8) / 4
    # groups against gridDim.y
    limit = int(lib.tike_max_grid_dim_y())
    big = 64
    while (-(-big // 64)) * (-(-big // 8)) <= 4 * limit:
        big *= 2
    assert call(a16=big) == ERR_ARG
    assert call(a14=17) == ERR_UNSUPPORTED  # S
    assert call(a14=16, a10=17, a11=1) == ERR_UNSUPPORTED  # C M = 17
    assert call(a14=16, a10=2, a11=9) == ERR_UNSUPPORTED  # C M = 18
    assert call(a13=0) == 0  # no position: no launch
    torch.cuda.synchronize()
    assert bool((buf == SENTINEL).all())
    assert call() == 0  # (the arguments were good)
    torch.cuda.synchronize()
    assert not bool((buf == SENTINEL).any())


# ------------------------------------------------------------------ end to end
def _operator(shape, norm="ortho"):
    import tike_amd.operators as ops
    N, S, M, C, pw, det, H, fly = shape
    return ops.Ptycho(probe_shape=pw, detector_shape=det, nz=H, n=H, norm=norm)


_KEYWORD = dict(d_psi="d_psi", d_probe="d_probe", d_scan="d_scan",
                d_eigen="d_eigen_probe", d_weights="d_eigen_weights")


def _device(c, *names):
    import torch
    return [None if c[k] is None else torch.from_numpy(c[k]).to("cuda")
            for k in names]


def _primals(c):
    """(psi, probe, scan), dict(eigen_probe=, eigen_weights=) on the device."""
    psi, probe, scan, eigen, weights = _device(c, "psi", "probe", "scan",
                                               "eigen", "weights")
    return (psi, probe, scan), dict(eigen_probe=eigen, eigen_weights=weights)


def _tangents(c, names=ej.TANGENT_NAMES):
    return {_KEYWORD[k]: t for k, t in zip(names, _device(c, *names))
            if t is not None}


def _run_jvp(shape, norm="ortho", names=ej.TANGENT_NAMES):
    """(I, dI, I of `intensity`) as host arrays."""
    import torch

    from tike_amd.autograd import eigen_intensity_jvp, intensity
    c = ej.case(*shape, norm)
    fly = shape[-1]
    primal, kw = _primals(c)
    with _operator(shape, norm) as op:
        inten, tangent = eigen_intensity_jvp(op, *primal, fly=fly, **kw,
                                             **_tangents(c, names))
        with torch.no_grad():
            plain = intensity(op, *primal, fly=fly, **kw)
    for x in (inten, tangent):
        assert x.dtype == torch.float32 and not x.requires_grad
        assert tuple(x.shape) == (shape[0] // fly, shape[5], shape[5])
    return tuple(x.cpu().numpy() for x in (inten, tangent, plain))


def _assert_jvp(shape, norm, got, what):
    c = ej.case(*shape, norm)
    inten, tangent, plain = got
    print(f"{what}: dI normwise {relerr(tangent, c['tangent']):.2e} max-abs "
          f"{maxerr(tangent, c['tangent']):.2e}; I normwise "
          f"{relerr(inten, c['intensity']):.2e}")
    assert np.array_equal(inten, plain), what  # the bits of intensity(...)
    assert_close(inten, c["intensity"], OP_NORMWISE, OP_MAXABS, what + " I")
    assert_close(tangent, c["tangent"], OP_NORMWISE, OP_MAXABS, what + " dI")


@pytest.mark.parametrize("shape",
                         ae.END_TO_END_CASES + ae.END_TO_END_CASES_MORE)
def test_eigen_intensity_jvp_vs_model(shape):
    """dI within the operator bars (normwise 1e-5, max-abs 1e-4) of the
    float64 `hand_jvp` with all five tangents (the float32 restatement on the
    CPU: 1.5 - 2.0e-7 normwise); I bit-identical to `intensity(...,
    eigen_probe=, eigen_weights=)`."""
    _assert_jvp(shape, "ortho", _run_jvp(shape), str(shape))


@pytest.mark.parametrize("norm", ["ortho", "forward", "backward"])
@pytest.mark.parametrize("shape", [ae.END_TO_END_CASES[0],
                                   ae.END_TO_END_CASES[2]])
def test_eigen_intensity_jvp_other_norms(shape, norm):
    """The operator's norm is honoured (the forward scale rides on the
    transform of the tangent): det 20 and 128."""
    assert shape[5] in (20, 128)
    _assert_jvp(shape, norm, _run_jvp(shape, norm), f"{shape} norm={norm}")


def test_no_tangent_gives_zeros():
    got = _run_jvp(ae.END_TO_END_CASES[0], names=())
    assert np.array_equal(got[0], got[2]) and not got[1].any()


THREE_CHUNKS = (12, 3, 2, 2, 16, 20, 48, 2)


def test_three_chunks(monkeypatch):
    """Cut into three chunks of whole frames at fly = 2: the bits of I and dI
    of the whole run (a chunk holds half of `chunk_positions`: two far
    planes).  d_scan and d_eigen_weights are sliced with their chunk."""
    from tike_amd.ptycho.solvers import lstsq
    N, S, M, C, pw, det, H, fly = THREE_CHUNKS
    whole = _run_jvp(THREE_CHUNKS)
    monkeypatch.setattr(lstsq, "CHUNK_POSITIONS_OVERRIDE", 8)
    assert max(1, lstsq.chunk_positions(S, det) // 2 // fly) * fly * 3 == N
    cut = _run_jvp(THREE_CHUNKS)
    _assert_jvp(THREE_CHUNKS, "ortho", cut, "three chunks")
    assert np.array_equal(whole[0], cut[0])
    assert np.array_equal(whole[1], cut[1])


# ------------------------------------------------------------ adjoint identity
# fly = 2 with probe window < detector; fly = 1 with window = detector and
# eigen probes on every mode; C = 0
ADJOINT_CASES = [ae.END_TO_END_CASES[0], ae.END_TO_END_CASES[3],
                 ae.END_TO_END_CASES_MORE[1]]


def _norm(a):
    return float(np.linalg.norm(np.asarray(a, np.complex128).ravel()))


@pytest.mark.parametrize("shape", ADJOINT_CASES)
def test_adjoint_identity_on_the_device(shape):
    """<u, dI> against the five inner products of the tangents with the grads
    of the existing backward of `intensity(..., eigen_probe=, eigen_weights=)`
    (real inner products in the `.grad` convention, summed in float64 on the
    host).  The bound is the sum of the bars the two sides already carry: dI,
    psi.grad, probe.grad and eigen_probe.grad are each 1e-5 normwise -- by
    Cauchy-Schwarz 1e-5 (|u| |dI| + |g_psi| |d_psi| + |g_probe| |d_probe| +
    |g_E| |d_E|) --, scan.grad SCAN_BAR A_n per position and coordinate and
    eigen_weights.grad WEIGHTS_BAR A[n,c,s] per entry, the A of
    `autograd_eigen.hand_gradients` for this u."""
    from tike_amd.autograd import eigen_intensity_jvp, intensity
    N, S, M, C, pw, det, H, fly = shape
    c = ej.case(*shape)
    primal, kw = _primals(c)
    leaves = [x.requires_grad_(True) for x in primal]
    kw = {k: None if v is None else v.requires_grad_(True)
          for k, v in kw.items()}
    (u,) = _device(c, "u")
    t = _tangents(c)
    with _operator(shape) as op:
        _, tangent = eigen_intensity_jvp(op, *leaves, fly=fly, **kw, **t)
        (intensity(op, *leaves, fly=fly, **kw) * u).sum().backward()
    grads = dict(d_psi=leaves[0].grad, d_probe=leaves[1].grad,
                 d_scan=leaves[2].grad,
                 d_eigen_probe=None if C == 0 else kw["eigen_probe"].grad,
                 d_eigen_weights=kw["eigen_weights"].grad)
    left = aj.inner(u, tangent)
    right = sum(aj.inner(grads[k], t[k]) for k in t)
    hand = ae.hand_gradients(*ae.model_of(c), det, ae.t128(c["u"]), fly)
    bound = 1e-5 * (_norm(c["u"]) * _norm(c["tangent"])
                    + _norm(hand["psi"].numpy()) * _norm(c["d_psi"])
                    + _norm(hand["probe"].numpy()) * _norm(c["d_probe"]))
    if C:
        bound += 1e-5 * _norm(hand["eigen"].numpy()) * _norm(c["d_eigen"])
    bound += ae.SCAN_BAR * float(
        (hand["A_scan"].numpy() * np.abs(c["d_scan"].astype(np.float64))).sum())
    bound += ae.WEIGHTS_BAR * float(
        (hand["A"].numpy() * np.abs(c["d_weights"].astype(np.float64))).sum())
    print(f"adjoint identity {shape}: <u, Jv> = {left:.9e}, <J^T u, v> = "
          f"{right:.9e}, difference {abs(left - right):.2e}, bound {bound:.2e}")
    assert abs(left - right) <= bound


# -------------------------------------------------- eigen_gauss_newton_product
@pytest.mark.parametrize("shape,weighted", [
    (ae.END_TO_END_CASES[0], False), (ae.END_TO_END_CASES[3], True),
    (ae.END_TO_END_CASES_MORE[1], True)])
def test_eigen_gauss_newton_product_vs_model(shape, weighted, monkeypatch):
    """J^T W J v against the float64 model (`hand_jvp`, then
    `autograd_eigen.hand_gradients` with g = W dI): the object, the probe and
    the eigen probe part normwise 1e-5, the scan part SCAN_BAR A_n per
    position and coordinate and the weights part WEIGHTS_BAR A[n,c,s] per
    entry (exactly 0 where A is), the A for that g; weight None and
    1 / (I + 1).  wrt=("eigen_weights",) launches no object scatter and gives
    the bits of the weights part of the full product."""
    import torch

    from tike_amd import autograd
    N, S, M, C, pw, det, H, fly = shape
    c = ej.case(*shape)
    weight = (1.0 / (c["intensity"] + 1.0)).astype(np.float32) if weighted \
        else None
    g = c["tangent"] if weight is None else weight.astype(np.float64) * c[
        "tangent"]
    hand = ae.hand_gradients(*ae.model_of(c), det, torch.from_numpy(g), fly)
    primal, kw = _primals(c)
    t = _tangents(c)
    w = None if weight is None else torch.from_numpy(weight).to("cuda")
    wrt = tuple(k for k in autograd._EIGEN_WRT if C or k != "eigen_probe")
    scatters = []
    scatter = autograd.lib.tike_scatter_patches
    monkeypatch.setattr(autograd.lib, "tike_scatter_patches",
                        lambda *a: scatters.append(1) or scatter(*a))
    with _operator(shape) as op:
        full = dict(zip(wrt, autograd.eigen_gauss_newton_product(
            op, *primal, weight=w, fly=fly, wrt=wrt, **kw, **t)))
        assert scatters
        del scatters[:]
        (only,) = autograd.eigen_gauss_newton_product(
            op, *primal, weight=w, fly=fly, wrt=("eigen_weights",), **kw, **t)
        assert not scatters
    host = lambda x: x.cpu().numpy()
    key = dict(psi="psi", probe="probe", eigen_probe="eigen")
    line = [f"eigen_gauss_newton_product {shape} weighted={weighted}:"]
    for k in wrt:
        if k in key:
            line.append(f"{k} normwise "
                        f"{relerr(host(full[k]), hand[key[k]].numpy()):.2e}")
    sratio = (np.abs(host(full["scan"]) - hand["scan"].numpy())
              / hand["A_scan"].numpy())
    A = hand["A"].numpy()
    live = A > 0
    gw = host(full["eigen_weights"])
    wratio = np.abs(gw - hand["weights"].numpy())[live] / A[live]
    print(" ".join(line) + f", scan max |err| / A_n {sratio.max():.2e}, "
          f"weights max |err| / A {wratio.max():.2e}")
    for k, x in zip(("psi", "probe", "scan"), primal):
        assert full[k].shape == x.shape and full[k].dtype == x.dtype
    assert gw.shape == c["weights"].shape and gw.dtype == np.float32
    for k in wrt:
        if k in key:
            assert relerr(host(full[k]), hand[key[k]].numpy()) <= OP_NORMWISE, k
    assert np.all(sratio <= ae.SCAN_BAR), sratio.max()
    assert np.all(wratio <= ae.WEIGHTS_BAR), wratio.max()
    assert np.all(gw[~live] == 0)
    assert np.array_equal(host(only), gw)


# ------------------------------------------------------- the refusals that stay
def test_the_existing_refusals_still_hold():
    """`intensity_jvp` and `gauss_newton_product` take no eigen parameter, and
    the eigen form of `intensity` on forward_ad dual tensors keeps torch's
    refusal: `_EigenIntensity` has no jvp rule; the functions are the
    interface."""
    import torch
    import torch.autograd.forward_ad as fwad

    from tike_amd import autograd
    shape = ae.END_TO_END_CASES[0]
    c = ej.case(*shape)
    fly = shape[-1]
    primal, kw = _primals(c)
    (d_scan,) = _device(c, "d_scan")
    assert "jvp" not in vars(autograd._EigenIntensity)
    with _operator(shape) as op:
        for fn in (autograd.intensity_jvp, autograd.gauss_newton_product):
            with pytest.raises(TypeError, match="eigen_weights"):
                fn(op, *primal, fly=fly, d_scan=d_scan,
                   eigen_weights=kw["eigen_weights"])
        with fwad.dual_level():
            dual = fwad.make_dual(primal[2], d_scan)
            with pytest.raises((NotImplementedError, RuntimeError),
                               match="(?i)implement the jvp"):
                autograd.intensity(op, primal[0], primal[1], dual, fly=fly,
                                   **kw)


# ------------------------------------------- joint recovery: scan and weights
def test_joint_levenberg_marquardt_recovers_positions_and_weights():
    """`autograd_eigen_jvp.recovery_problem()`: `autograd_eigen.problem()`
    (14 x 14 raster, pw = det = 32, one eigen probe) with the positions
    started at scan_start (+- 0.3 px), the weights at row 1 = 0, and fly = 1
    data -- at the problem's own fly = 2 the joint problem is degenerate in
    the float64 model itself (see `recovery_problem`).  Four
    Levenberg-Marquardt steps of at most 20 CG iterations on (scan, weights)
    jointly (`joint_gauss_newton`), every product on the GPU -- J v by
    `eigen_intensity_jvp`, J^T u by the backward of `intensity`.  Required:
    finite costs that fall with every step, and a final position RMS and
    weights RMS of at most what the float64 model reaches plus twice the
    deviation of the float32 restatement of the same iteration on the CPU from
    it (`JOINT_RECOVERY`, reproduced by test_autograd_eigen_jvp_cpu.py):

        float64 model    0.162853973 px   0.010376284   (from 0.2433, 0.1210)
        float32 on CPU   0.162854100 px   0.010376345
        bound            0.162854227 px   0.010376405
        MI355X           0.162854186 px   0.010376313   (when the test was
                                                         written)

    60 steps of Adam on the weights alone (`autograd_eigen.recover`) from the
    same start are printed next to it, not asserted."""
    import torch

    from tike_amd.autograd import eigen_intensity_jvp, intensity
    p = ej.recovery_problem()
    fly, det = p["fly"], p["det"]
    psi, probe, eigen, data, scan0, w0 = _device(
        p, "psi", "probe", "eigen", "data", "scan_start", "weights_start")
    shape = (0, 1, 1, 1, det, det, psi.shape[-1], fly)
    with _operator(shape) as op:

        def forward(x):
            with torch.no_grad():
                return intensity(op, psi, probe, x[0], eigen_probe=eigen,
                                 eigen_weights=x[1], fly=fly)

        def jtu(x, u):
            s, w = (t.detach().requires_grad_(True) for t in x)
            return torch.autograd.grad(
                intensity(op, psi, probe, s, eigen_probe=eigen,
                          eigen_weights=w, fly=fly), (s, w), grad_outputs=u)

        jv = lambda x, v: eigen_intensity_jvp(
            op, psi, probe, x[0], eigen_probe=eigen, eigen_weights=x[1],
            d_scan=v[0], d_eigen_weights=v[1], fly=fly)[1]
        after, costs = ej.joint_gauss_newton(forward, jv, jtu, data,
                                             (scan0, w0))
        adam, _ = ae.recover(
            lambda w: am.amplitude_loss(
                intensity(op, psi, probe, scan0, eigen_probe=eigen,
                          eigen_weights=w, fly=fly), data), w0)
    r0 = am.rms(p["scan_start"], p["scan_true"])
    q0 = ae.weights_rms(p["weights_start"], p["weights_true"])
    r = [am.rms(a[0], p["scan_true"]) for a in after]
    q = [ae.weights_rms(a[1], p["weights_true"]) for a in after]
    qa = ae.weights_rms(adam, p["weights_true"])
    rbound, qbound = ej.joint_recovery_bounds()
    print(f"joint LM recovery: rms {r0:.4f} -> "
          + ", ".join(f"{x:.9f}" for x in r) + f" (bound {rbound:.9f}); "
          f"weights rms {q0:.4f} -> " + ", ".join(f"{x:.9f}" for x in q)
          + f" (bound {qbound:.9f}); cost "
          + " -> ".join(f"{x:.6e}" for x in costs)
          + f"; 60 steps of Adam on the weights alone, positions left at "
          f"their start: weights rms {qa:.6f}")
    assert np.isfinite(costs).all()
    assert all(b < a for a, b in zip(costs, costs[1:])), costs
    assert r[-1] <= rbound, (r[-1], rbound)
    assert q[-1] <= qbound, (q[-1], qbound)
