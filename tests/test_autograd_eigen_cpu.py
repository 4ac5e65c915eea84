"""`tike_amd.autograd.intensity` with eigen probes, without a GPU: the formulas
of the HIP backward against `torch.autograd` on the float64 model
(tests/autograd_eigen.py), a finite difference, the float32 restatement the
GPU bars rest on, every new refusal, the ABI, and the weight recovery of the
GPU test on the model alone."""
import ctypes

import numpy as np
import pytest
import torch

import autograd_eigen as ae
import autograd_model as am

rel = ae.rel


# ------------------------------------------------ formulas against autograd
@pytest.mark.parametrize("norm", ["ortho", "backward"])
@pytest.mark.parametrize("shape", ae.END_TO_END_CASES
                         + ae.END_TO_END_CASES_MORE)
def test_hand_formulas_equal_torch_autograd(shape, norm):
    """All five gradients to 1e-12 normwise; the block of modes without an
    eigen probe (s >= M, rows >= 1) is exactly zero in both."""
    N, S, M, C, pw, det, H, fly = shape
    c = ae.case(*shape, norm)
    m = ae.model_of(c)
    auto = ae.autograd_gradients(*m, det, ae.t128(c["g"]), fly, norm)
    hand = c["want"]
    for k in ("psi", "probe", "scan", "eigen", "weights"):
        if hand[k] is None:  # C = 0: no eigen probe
            assert k == "eigen" and C == 0 and auto[k] is None
            continue
        err = rel(hand[k], auto[k].numpy())
        print(f"{shape} {norm} {k}: {err:.2e}")
        assert err < 1e-12, k
    assert hand["weights"].shape == (N, C + 1, S)
    assert np.all(hand["weights"][:, 1:, M:] == 0)
    assert np.all(auto["weights"].numpy()[:, 1:, M:] == 0)
    assert np.all(hand["A"][:, 1:, M:] == 0)
    assert np.all(np.abs(hand["weights"]) <= hand["A"])


def test_no_eigen_probe_is_a_scale_per_position():
    """C = 0: eigen=None with weights (N, 1, S)."""
    N, S, pw, det, H, fly = 4, 2, 8, 12, 30, 2
    c = ae.inputs(N, S, 0, 0, pw, H, H, seed=3)
    assert c["eigen"] is None and c["weights"].shape == (N, 1, S)
    m = ae.model_of(c)
    g = torch.from_numpy(np.random.default_rng(4).standard_normal(
        (N // fly, det, det)))
    auto = ae.autograd_gradients(*m, det, g, fly)
    hand = ae.hand_gradients(*m, det, g, fly)
    assert auto["eigen"] is None and hand["eigen"] is None
    for k in ("psi", "probe", "scan", "weights"):
        assert rel(hand[k].numpy(), auto[k].numpy()) < 1e-12, k
    # weights of one: the shared-probe model
    ones = torch.ones_like(m[4])
    with torch.no_grad():
        a = ae.intensity(*m[:3], None, ones, det, fly)
        b = am.intensity(*m[:3], det, fly)
    assert torch.equal(a, b)


def test_gradients_equal_a_finite_difference():
    """One weight and one eigen-probe pixel (both parts), to 1e-5."""
    shape = ae.END_TO_END_CASES[0]
    N, S, M, C, pw, det, H, fly = shape
    c = ae.case(*shape)
    psi, probe, scan, eigen, weights = ae.model_of(c)
    g = ae.t128(c["g"])
    f = lambda e, w: float((ae.intensity(psi, probe, scan, e, w, det, fly)
                            * g).sum())
    h = 1e-6
    with torch.no_grad():
        for idx in ((2, 0, 1), (3, 2, 1), (1, 1, 0)):
            d = torch.zeros_like(weights)
            d[idx] = h
            fd = (f(eigen, weights + d) - f(eigen, weights - d)) / (2 * h)
            want = c["want"]["weights"][idx]
            print(f"weight {idx}: {want:.8e} fd {fd:.8e}")
            assert abs(fd - want) <= 1e-5 * abs(want)
        idx = (0, 1, 1, 5, 7)
        got = []
        for part in (1.0, 1j):
            d = torch.zeros_like(eigen)
            d[idx] = h * part
            got.append((f(eigen + d, weights) - f(eigen - d, weights))
                       / (2 * h))
        fd, want = complex(*got), c["want"]["eigen"][idx]
        print(f"eigen pixel {idx}: {want:.8e} fd {fd:.8e}")
        assert abs(fd - want) <= 1e-5 * abs(want)


# ------------------------------------------- the float32 restatement: the bars
@pytest.mark.parametrize("shape", ae.ENTRY_CASES
                         + ae.ENTRY_CASES_EVERY_KERNEL)
def test_float32_products_with_float64_sums_fix_the_entry_bar(shape):
    """`entry_model(single=True)` -- patch, q and terms in float32, the sums
    in float64, the kernel's arithmetic -- against the float64 one on the same
    float32 chi: the weight gradient stays below a third of 1e-7 A (measured
    when the bar was set: 2.2e-9 to 1.7e-8 A over all the shapes), so the GPU
    test holds the entry to the bar of `tike_scan_gradient` alone; the planes
    stay two orders below the operator bar."""
    c = ae.entry_case(*shape)
    psi, probe, scan, eigen, weights = ae.model_of(c)
    got = ae.entry_model(ae.t128(c["chi"]), psi, probe, eigen, weights, scan,
                         single=True)
    want = c["want"]
    live = want["A"] > 0
    ratio = (np.abs(got["weights"].numpy() - want["weights"])[live]
             / want["A"][live]).max()
    planes = [rel(got[k].numpy(), want[k]) for k in ("probe", "objproj")]
    if want["eigen"] is not None:
        planes.append(rel(got["eigen"].numpy(), want["eigen"]))
    print(f"{shape}: float32 restatement: weights / A {ratio:.2e}, planes "
          f"{max(planes):.2e}")
    assert np.all(got["weights"].numpy()[~live] == 0)
    assert ratio <= ae.WEIGHTS_ENTRY_BAR / 3
    assert max(planes) <= 1e-6


@pytest.mark.parametrize("shape", ae.END_TO_END_CASES
                         + ae.END_TO_END_CASES_MORE)
def test_complex64_restatement_fixes_the_end_to_end_bars(shape):
    """The whole backward in complex64 / float32 (sums of the weight and scan
    gradients in float64) against the float64 one: planes 2.1 - 2.5e-7
    normwise, weights at most 5.4e-8 A and scan at most 2.3e-8 A_n on these
    inputs when the bars were set -- a margin of 18 and more under 1e-6 A:
    the GPU bars test the kernels, not the model.  (The issue quotes 1.8 -
    2.1e-7 and 4.4e-8 A, a margin above 20, for its own random inputs at the
    first four shapes; the generator here draws other numbers, the bars are
    the issue's.)"""
    N, S, M, C, pw, det, H, fly = shape
    c = ae.case(*shape)
    got = ae.hand_gradients(*ae.model_of(c), det, ae.t128(c["g"]), fly,
                            single=True)
    want = c["want"]
    live = want["A"] > 0
    ratio = (np.abs(got["weights"].numpy() - want["weights"])[live]
             / want["A"][live]).max()
    sratio = (np.abs(got["scan"].numpy() - want["scan"])
              / want["A_scan"]).max()
    planes = max(rel(got[k].numpy(), want[k])
                 for k in ("psi", "probe", "eigen") if want[k] is not None)
    print(f"{shape}: complex64 restatement: planes {planes:.2e}, weights / A "
          f"{ratio:.2e}, scan / A_n {sratio:.2e}")
    assert planes <= 1e-6
    assert ratio <= ae.WEIGHTS_BAR / 10
    assert sratio <= ae.SCAN_BAR / 10


# ------------------------------------------------------------------ refusals
def test_every_new_refusal():
    """CPU tensors reach every refusal of the eigen arguments, and are
    themselves refused last."""
    import tike_amd.operators as ops
    from tike_amd.autograd import (MAX_EIGEN_PLANES, intensity,
                                   multislice_intensity)
    assert MAX_EIGEN_PLANES == 16
    pw, det, H, W, N, S = 8, 12, 24, 31, 6, 3
    c64 = torch.complex64
    psi = torch.zeros((1, H, W), dtype=c64)
    probe = torch.zeros((1, 1, S, pw, pw), dtype=c64)
    scan = torch.full((N, 2), 3.5)
    eigen = torch.zeros((1, 2, 2, pw, pw), dtype=c64)
    w = torch.ones((N, 3, S))
    with ops.Ptycho(probe_shape=pw, detector_shape=det, nz=H, n=W) as op:
        f = lambda **k: intensity(op, psi, probe, scan, **k)
        with pytest.raises(ValueError, match="eigen_probe without eigen_w"):
            f(eigen_probe=eigen)
        with pytest.raises(TypeError, match="eigen_weights must be a torch"):
            f(eigen_probe=eigen, eigen_weights=w.numpy())
        with pytest.raises(TypeError, match="eigen_probe must be a torch"):
            f(eigen_probe=eigen.numpy(), eigen_weights=w)
        with pytest.raises(TypeError,
                           match="eigen_weights must be torch.float32"):
            f(eigen_probe=eigen, eigen_weights=w.double())
        with pytest.raises(TypeError,
                           match="eigen_probe must be torch.complex64"):
            f(eigen_probe=eigen.to(torch.complex128), eigen_weights=w)
        # ranks
        with pytest.raises(ValueError, match=r"eigen_weights \(N, C \+ 1, S\)"):
            f(eigen_probe=eigen, eigen_weights=w[0])
        with pytest.raises(ValueError, match=r"eigen_weights \(N, C \+ 1, S\)"):
            f(eigen_probe=eigen[0], eigen_weights=w)
        # the eigen probes' shape
        with pytest.raises(ValueError, match="eigen_probe must be"):
            f(eigen_probe=eigen[..., :7], eigen_weights=w)
        with pytest.raises(ValueError, match="eigen_probe must be"):
            f(eigen_probe=eigen.expand(2, 2, 2, pw, pw), eigen_weights=w)
        with pytest.raises(ValueError, match="eigen_probe must be"):
            f(eigen_probe=eigen[:, :0], eigen_weights=w[:, :1])
        with pytest.raises(ValueError, match="1 <= M <= S = 3"):  # M > S
            f(eigen_probe=torch.zeros((1, 2, S + 1, pw, pw), dtype=c64),
              eigen_weights=w)
        # the weights: C + 1 rows, N positions, S columns
        for bad in (w[:, :2], torch.ones((N, 4, S)), w[:N - 1], w[:, :, :2],
                    torch.ones((N // 2, 3, S))):
            with pytest.raises(ValueError, match="eigen_weights must be"):
                f(eigen_probe=eigen, eigen_weights=bad)
        with pytest.raises(ValueError, match="eigen_weights must be"):
            f(eigen_weights=w)  # C = 0 takes (N, 1, S)
        # the planes the kernel takes
        big = torch.zeros((1, 6, 3, pw, pw), dtype=c64)
        with pytest.raises(ValueError, match=f"at most {MAX_EIGEN_PLANES}"):
            f(eigen_probe=big, eigen_weights=torch.ones((N, 7, S)))
        # a probe tensor per position is still refused, and says where to go
        with pytest.raises(NotImplementedError, match="probe per position"):
            intensity(op, psi, probe.expand(N, 1, S, pw, pw), scan)
        with pytest.raises(NotImplementedError, match="eigen_weights="):
            intensity(op, psi, probe.expand(N, 1, S, pw, pw), scan)
        # fly: the weights belong to positions
        with pytest.raises(ValueError, match="not a multiple of fly=4"):
            f(eigen_probe=eigen, eigen_weights=w, fly=4)
        # several slices do not get the keywords
        with pytest.raises(TypeError, match="unexpected keyword"):
            multislice_intensity(op, psi, probe, scan, eigen_weights=w)
        # the last refusal: fails on the parent commit with "unexpected
        # keyword argument"
        for k in (dict(eigen_probe=eigen, eigen_weights=w),
                  dict(eigen_weights=w[:, :1]),
                  dict(eigen_probe=eigen, eigen_weights=w, fly=2),
                  dict(eigen_probe=torch.zeros((1, 16, 1, pw, pw), dtype=c64),
                       eigen_weights=torch.ones((N, 17, S)))):
            with pytest.raises(TypeError, match="no CPU fallback"):
                f(**k)


# ------------------------------------------------------------------- the ABI
NAME = "tike_eigen_probe_gradients"


def test_abi_has_the_new_entry():
    """Fails on the parent commit: the symbol does not exist."""
    import tike_amd._lib as L
    assert NAME in L.declared_symbols()
    assert len(L._PROTOTYPES[NAME]) == 19
    assert hasattr(ctypes.CDLL(L.LIB_PATH), NAME)
    assert L.ABI_VERSION >= 21
    assert "autograd_eigen.hip" in open(
        L.LIB_PATH.replace("libtike_amd.so", "Makefile")).read()


def test_abi_entry_checks_its_arguments_without_a_gpu():
    """What needs no device: the limits, the counts, nothing to do."""
    import tike_amd._lib as L
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p)
    # (chi, scan, psi, probe, eigen_probe, eigen_weights, num_eigen,
    #  eigen_modes, probe_grad, eigen_grad, weights_grad, objproj, work, nscan,
    #  S, pw, H, W, stream)
    ok = (p, p, p, p, p, p, 1, 1, p, p, p, p, p, 1, 2, 2, 4, 4, None)

    def call(**change):
        args = list(ok)
        for k, v in change.items():
            args[int(k[1:])] = v
        return getattr(L.lib, NAME)(*args)
    assert call(a6=17, a7=1) == L.ERR_UNSUPPORTED  # C * M = 17
    assert call(a6=3, a7=6, a14=8) == L.ERR_UNSUPPORTED  # C * M = 18
    assert call(a14=17) == L.ERR_UNSUPPORTED  # S
    assert call(a13=-1) == L.ERR_ARG  # nscan
    assert call(a14=0) == L.ERR_ARG  # S
    assert call(a15=0) == L.ERR_ARG  # pw
    assert call(a16=0) == L.ERR_ARG  # H
    assert call(a17=0) == L.ERR_ARG  # W
    assert call(a6=-1) == L.ERR_ARG  # C
    assert call(a7=0) == L.ERR_ARG  # M < 1 with C > 0
    assert call(a7=3) == L.ERR_ARG  # M > S
    assert call(a4=None) == L.ERR_ARG  # eigen probes missing with C > 0
    for k in (0, 1, 2, 3, 5):
        assert call(**{f"a{k}": None}) == L.ERR_ARG  # a NULL input
    assert call(a12=None) == L.ERR_ARG  # weights_grad without work
    assert call(a13=0) == 0  # no position: no launch
    assert call(a8=None, a9=None, a10=None, a11=None) == 0  # no output


# ------------------------------------------------------------ weight recovery
def test_model_recovers_the_eigen_weights():
    """The condition on the inputs of the GPU test: 60 steps of Adam(lr=0.05)
    on eigen_weights alone, fly = 2, bring the RMS error over all weight
    entries to 0.35 of its start or less and the cost below 1 % of its start
    on the float64 model ALONE, with margin (0.19 and 0.17 % at seed 0 when
    the bars were set; asserted here at 0.25 and 0.5 %)."""
    p = ae.problem(seed=0)
    assert p["fly"] == 2 and p["det"] == 32 and p["eigen"].shape[1:3] == (1, 1)
    assert p["scan_true"].shape[0] == 14 * 14
    psi, probe, scan, eigen = (ae.t128(p[k]) for k in (
        "psi", "probe", "scan_true", "eigen"))
    data = ae.t128(p["data"])
    final, costs = ae.recover(
        lambda w: am.amplitude_loss(
            ae.intensity(psi, probe, scan, eigen, w, p["det"], p["fly"]),
            data), ae.t128(p["weights_start"]))
    r0 = ae.weights_rms(p["weights_start"], p["weights_true"])
    r1 = ae.weights_rms(final, p["weights_true"])
    print(f"weights rms {r0:.4f} -> {r1:.4f} ({r1 / r0:.3f}), cost "
          f"{costs[0]:.3e} -> {costs[-1]:.3e} ({costs[-1] / costs[0]:.5f})")
    assert np.isfinite(costs).all() and len(costs) == ae.RECOVERY["steps"]
    assert r1 <= 0.25 * r0, (r0, r1)
    assert costs[-1] < 0.005 * costs[0], (costs[0], costs[-1])
