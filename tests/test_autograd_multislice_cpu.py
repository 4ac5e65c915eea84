"""`tike_amd.autograd.multislice_intensity` without a GPU: the float64 model
(tests/autograd_multislice.py) pinned to what the project already pins -- the
multislice model of cgrad (tests/cgrad_multislice.py) --, its hand formulas
against torch.autograd, every refusal, the new ABI entry, the float32
restatement that fixes the scan bar of the GPU tests, and the condition on the
position-recovery problem.

Every figure a bar is set on is printed before it is asserted."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import autograd_model as am
import autograd_multislice as mm
import cgrad_multislice as ms


def rel(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


# ------------------------------------------- the model against cgrad's model
PINNED = [dict(obj=24, pw=8, S=2, D=2, N=6, seed=1),
          dict(obj=40, pw=16, S=3, D=3, N=8, seed=2),
          dict(obj=37, pw=12, S=1, D=2, N=9, seed=3)]


@functools.lru_cache(maxsize=None)
def _pinned(i):
    """`cgrad_multislice.problem` with the fractions of the positions moved to
    quarters: cgrad's model rounds the four bilinear weights to float32
    (oracle.operators._patch_geometry), this one forms them in float64 from
    the float32 positions; products of quarters are exact in both, so the two
    can be compared far below float32's rounding.  A strong probe (amp 300)
    keeps the 1e-9 that cgrad's gaussian factor adds to sqrt(I) below the
    bar of the gradient comparison (3.3e-10 normwise at amp 30, 3.3e-11 here)."""
    kw = PINNED[i]
    P = ms.problem(**kw, amp=300.0)
    rng = np.random.default_rng(kw["seed"])
    scan = (np.floor(P["scan"]) + rng.integers(0, 4, P["scan"].shape) / 4
            ).astype(np.float32)
    data = ms.simulate(P["probe"], scan, P["psi"], P["H"])
    return dict(P, scan=scan, data=data)


@pytest.mark.parametrize("i", range(len(PINNED)))
def test_model_intensity_equals_cgrads_model(i):
    P = _pinned(i)
    got = mm.intensity(*mm.as_model(P["psi"], P["probe"], P["scan"])).numpy()
    e = rel(got, P["data"])
    print(f"{PINNED[i]}: intensity normwise {e:.2e}")
    assert got.shape == P["data"].shape
    assert e <= 1e-12


@pytest.mark.parametrize("i", range(len(PINNED)))
def test_autograd_of_the_gaussian_cost_equals_cgrads_gradients(i):
    """cost = mean over positions and pixels of (sqrt(I) - sqrt(d))^2, at the
    first iterates.  `cgrad_multislice.gradients` returns the unnormalised
    adjoint, cost' = 2 / (N npix) Re <gradient, direction>; a complex leaf's
    .grad in PyTorch is dL/dRe + i dL/dIm, so .grad = 2 / (N npix) gradient."""
    P = _pinned(i)
    psi, probe, scan, Hprop = mm.as_model(P["psi0"], P["probe0"], P["scan"])
    psi.requires_grad_(True), probe.requires_grad_(True)
    data = torch.from_numpy(P["data"]).to(am.F64)
    cost = am.amplitude_loss(mm.intensity(psi, probe, scan, Hprop), data)
    cost.backward()
    want_cost = ms.cost("gaussian", P["data"], P["psi0"], P["scan"],
                        P["probe0"], P["H"])
    gpsi, gprobe = ms.gradients("gaussian", P["data"], P["psi0"], P["scan"],
                                P["probe0"], P["H"])
    k = 2.0 / data.numel()
    e_psi = rel(psi.grad.numpy(), k * gpsi)
    e_probe = rel(probe.grad.numpy(), k * gprobe)
    print(f"{PINNED[i]}: cost {abs(float(cost.detach()) - want_cost) / want_cost:.2e}, "
          f"psi.grad {e_psi:.2e}, probe.grad {e_probe:.2e}")
    assert abs(float(cost.detach()) - want_cost) <= 1e-12 * want_cost
    assert e_psi <= 1e-10 and e_probe <= 1e-10
    for d in range(gpsi.shape[0]):  # every slice on its own
        assert rel(psi.grad[d].numpy(), k * gpsi[d]) <= 1e-10


# ------------------------------------------------- hand formulas vs autograd
# (N, S, pw, obj, D, fly)
SHAPES = [(6, 2, 8, 24, 2, 1), (8, 3, 16, 40, 3, 2), (9, 1, 12, 37, 2, 3)]


@pytest.mark.parametrize("norm", ["ortho", "backward", "forward"])
@pytest.mark.parametrize("shape", SHAPES)
def test_hand_formulas_equal_torch_autograd(shape, norm):
    c = mm.case(*shape, norm=norm)
    m = mm.as_model(c["psi"], c["probe"], c["scan"])
    g = torch.from_numpy(c["g"]).to(am.F64)
    fly = c["fly"]
    inten, gpsi, gprobe, gscan = mm.autograd_gradients(*m, g, fly, norm)
    hand = mm.hand_gradients(*m, g, fly, norm)
    ratio = ((hand["scan"] - gscan).abs() / hand["A"]).max()
    print(f"{shape} {norm}: psi {rel(hand['psi'], gpsi):.2e} probe "
          f"{rel(hand['probe'], gprobe):.2e} scan / A_n {float(ratio):.2e}")
    assert hand["psi"].shape == m[0].shape and inten.shape == g.shape
    assert rel(hand["psi"], gpsi) <= 1e-10
    for d in range(shape[4]):
        assert rel(hand["psi"][d], gpsi[d]) <= 1e-10
    assert rel(hand["probe"], gprobe) <= 1e-10
    assert float(ratio) <= 1e-10
    # the terms cancel: the sums are far below their absolute terms
    assert np.all(hand["scan"].abs().numpy() <= hand["A"].numpy())


def test_one_slice_is_the_single_slice_model():
    """D = 1: the model and its hand formulas are autograd_model's."""
    N, S, pw, obj, fly = 6, 2, 8, 24, 2
    c = mm.case(N, S, pw, obj, 1, fly)
    m = mm.as_model(c["psi"], c["probe"], c["scan"])
    g = torch.from_numpy(c["g"]).to(am.F64)
    one = am.hand_gradients(*m[:3], pw, g, fly)
    many = mm.hand_gradients(*m, g, fly)
    for k in ("psi", "probe", "scan", "A"):
        assert rel(many[k], one[k]) <= 1e-13, k


# ------------------------------------------------------------------ refusals
def test_every_refusal():
    """Fails on the parent commit: the function does not exist.  The argument
    checks come before any device work, in `intensity`'s order: CPU tensors
    reach every one of them, and are themselves refused last."""
    import tike_amd.operators as ops
    from tike_amd.autograd import MAX_MODES, intensity, multislice_intensity
    pw, H, W, N, D = 8, 24, 31, 6, 2
    psi = torch.zeros((D, H, W), dtype=torch.complex64)
    probe = torch.zeros((1, 1, 2, pw, pw), dtype=torch.complex64)
    scan = torch.full((N, 2), 3.5)
    f = multislice_intensity
    with ops.Ptycho(probe_shape=pw, detector_shape=pw, nz=H, n=W,
                    **mm.optics(pw)) as op:
        with pytest.raises(TypeError, match="psi must be a torch"):
            f(op, psi.numpy(), probe, scan)
        with pytest.raises(TypeError, match="scan must be a torch"):
            f(op, psi, probe, scan.numpy())
        with pytest.raises(TypeError, match="probe must be torch.complex64"):
            f(op, psi, probe.to(torch.complex128), scan)
        with pytest.raises(TypeError, match="scan must be torch.float32"):
            f(op, psi, probe, scan.to(torch.float64))
        with pytest.raises(ValueError, match=r"psi \(D, H, W\)"):
            f(op, psi[0], probe, scan)
        with pytest.raises(ValueError, match=r"psi \(D, H, W\)"):
            f(op, psi[:0], probe, scan)
        with pytest.raises(ValueError, match=r"psi \(D, H, W\)"):
            f(op, psi, probe[0], scan)
        with pytest.raises(ValueError, match=r"psi \(D, H, W\)"):
            f(op, psi, probe, scan[:, :1])
        # a probe per position comes before the shapes, as in `intensity`
        with pytest.raises(NotImplementedError, match="probe per position"):
            f(op, psi[:, :5], probe.expand(N, 1, 2, pw, pw), scan)
        with pytest.raises(ValueError, match="probe must be"):
            f(op, psi, probe[..., :7], scan)
        with pytest.raises(ValueError, match=f"psi must be .D, {H}, {W}."):
            f(op, psi[:, :, :30], probe, scan)
        with pytest.raises(ValueError, match="not a multiple of fly=4"):
            f(op, psi, probe, scan, fly=4)
        many = torch.zeros((1, 1, MAX_MODES + 1, pw, pw), dtype=torch.complex64)
        with pytest.raises(ValueError, match=f"at most {MAX_MODES}"):
            f(op, psi, many, scan)
        for bad in ((0.5, 3.0), (3.0, W - pw + 0.5)):
            outside = scan.clone()
            outside[2] = torch.tensor(bad)
            with pytest.raises(ValueError, match="Scan positions must be >= 1"):
                f(op, psi, probe, outside)
            # unchecked, the call goes on to the next refusal
            with pytest.raises(TypeError, match="no CPU fallback"):
                f(op, psi, probe, outside, check_positions=False)
        with pytest.raises(TypeError, match="multislice_intensity: psi lives"):
            f(op, psi, probe, scan)
        # one slice is taken too, and refused as late
        with pytest.raises(TypeError, match="no CPU fallback"):
            f(op, psi[:1], probe, scan)
        # `intensity` still turns several slices down, and says where to go
        with pytest.raises(NotImplementedError, match="several slices"):
            intensity(op, psi, probe, scan)
        with pytest.raises(NotImplementedError, match="multislice_intensity"):
            intensity(op, psi, probe, scan)
    # several slices need probe window = detector; one slice does not
    with ops.Ptycho(probe_shape=pw, detector_shape=12, nz=H, n=W) as op:
        with pytest.raises(ValueError, match="detector_shape == probe_shape"):
            f(op, psi, probe, scan)
        with pytest.raises(ValueError, match="detector_shape == probe_shape"):
            f(op, psi, probe, scan, fly=4)  # (the shapes come before fly)
        with pytest.raises(ValueError, match="not a multiple of fly=4"):
            f(op, psi[:1], probe, scan, fly=4)
        with pytest.raises(TypeError, match="no CPU fallback"):
            f(op, psi[:1], probe, scan)
    # more than 8 modes at a fused size: the general route takes them
    with ops.Ptycho(probe_shape=128, detector_shape=128, nz=140, n=140,
                    **mm.optics(128)) as op:
        psi = torch.zeros((D, 140, 140), dtype=torch.complex64)
        ok = torch.zeros((1, 1, MAX_MODES, 128, 128), dtype=torch.complex64)
        with pytest.raises(TypeError, match="no CPU fallback"):
            f(op, psi, ok, scan)
        over = torch.zeros((1, 1, MAX_MODES + 1, 128, 128),
                           dtype=torch.complex64)
        with pytest.raises(ValueError, match=f"at most {MAX_MODES}"):
            f(op, psi, over, scan)


# ------------------------------------------------------------------- the ABI
def test_abi_has_the_new_entry():
    """Fails on the parent commit: the symbol does not exist."""
    import tike_amd._lib as L
    name = "tike_scan_gradient_slices"
    assert name in L.declared_symbols()
    assert len(L._PROTOTYPES[name]) == 11
    assert hasattr(ctypes.CDLL(L.LIB_PATH), name)
    assert L.ABI_VERSION >= 20


def test_abi_entry_checks_its_arguments_without_a_gpu():
    """Argument checks come before any launch."""
    import tike_amd._lib as L
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p)
    # (objproj, slice_stride, scan, psi, grad, nscan, D, pw, H, W, stream)
    ok = (p, 4, p, p, p, 1, 2, 2, 4, 4, None)

    def call(**change):
        args = list(ok)
        for k, v in change.items():
            args[int(k[1:])] = v
        return L.lib.tike_scan_gradient_slices(*args)
    for k in (0, 2, 3, 4):
        assert call(**{f"a{k}": None}) == L.ERR_ARG  # a NULL array
    assert call(a1=3) == L.ERR_ARG  # the planes would overlap
    assert call(a5=-1) == L.ERR_ARG  # nscan
    assert call(a5=1 << 31, a1=1 << 40) == L.ERR_ARG  # more than grid.x holds
    assert call(a6=0) == L.ERR_ARG  # D
    assert call(a7=0) == L.ERR_ARG  # pw
    assert call(a8=0) == L.ERR_ARG  # H
    assert call(a9=0) == L.ERR_ARG  # W
    assert call(a5=0) == 0  # no position: no launch
    assert call(a5=0, a1=0) == 0


# ------------------------------------------- the float32 restatement: the bars
@pytest.mark.parametrize("shape", mm.END_TO_END_CASES)
def test_float32_restatement_fixes_the_scan_bar(shape):
    """`hand_gradients` in complex64 / float32 (terms in float32, the scan
    sums in float64, as the kernels have it) against the float64 one, on the
    inputs of the GPU end-to-end cases: the scan gradient stays within 1e-7
    A_n, so the GPU bar is the single-slice bar, 1e-6 A_n (`mm.SCAN_BAR`);
    intensity and the other gradients stay two orders below the operator bar.
    Measured when the bars were set: profiles/autograd_multislice.md."""
    c = mm.case(*shape)
    want, got = mm.case_model(c), mm.case_model(c, single=True)
    ratio = np.abs(got["grad_scan"] - want["grad_scan"]) / want["grad_A"]
    per_slice = max(rel(got["grad_psi"][d], want["grad_psi"][d])
                    for d in range(shape[4]))
    print(f"{shape}: float32 restatement: intensity "
          f"{rel(got['intensity'], want['intensity']):.2e}, psi.grad "
          f"{rel(got['grad_psi'], want['grad_psi']):.2e} (worst slice "
          f"{per_slice:.2e}), probe.grad "
          f"{rel(got['grad_probe'], want['grad_probe']):.2e}, scan.grad / A_n "
          f"{ratio.max():.2e}")
    assert ratio.max() <= 1e-7
    assert mm.SCAN_BAR == 1e-6
    assert per_slice <= 1e-6
    assert rel(got["grad_probe"], want["grad_probe"]) <= 1e-6


# --------------------------------------------------------- position recovery
def test_model_recovers_the_positions_of_a_two_slice_object():
    """The condition on the inputs of the GPU test: with `mm.RECOVERY`'s seed
    and steps the float64 model ALONE at least halves the RMS position error
    (0.43 of its start, the cost to 0.8 % of its start, when they were
    chosen)."""
    p = mm.problem(seed=mm.RECOVERY["seed"])
    assert p["psi"].shape[0] == 2 and p["fly"] == 2 and p["det"] == 32
    final, costs = mm.recover_on_model(p)
    r0, r1 = am.rms(p["scan_start"], p["scan_true"]), am.rms(
        final, p["scan_true"])
    print(f"rms {r0:.3f} -> {r1:.3f} ({r1 / r0:.3f}), cost {costs[0]:.2e} -> "
          f"{costs[-1]:.2e} ({costs[-1] / costs[0]:.4f})")
    assert np.isfinite(costs).all() and len(costs) == mm.RECOVERY["steps"]
    assert r1 <= 0.5 * r0, (r0, r1)
