"""The noise-model entries, called through tike_amd._lib with raw pointers,
against the float64 model of tests/noise_models.py on the cases of its table
(tests/test_noise_models_cpu.py pins the model, the preconditions of the cases
and the reach of the bounds).

Stored-input entries (24^2, 48^2, 15^2): tike_gradient_scale,
tike_farplane_gradient, tike_cost_each_pattern, tike_objective_grad,
tike_poisson_steps (all modes and dominant mode) and tike_scale_modes.  The
two stand-alone objective helpers take no mask and read every count, so they
run on the unmasked cases only.  Hand-off entries (256^2, 512^2):
tike_fwd_gradient_scale, tike_fwd_grad_ifft2_pass1, tike_poisson_steps_handoff
+ tike_grad_ifft2_pass1, tike_poisson_steps_grad_ifft2_pass1 +
tike_ifft2_pass2_gradients_scaled.  A `work` buffer is judged through
tike_ifft2_pass2_gradients[_scaled], one position at a time: with patches
identically 1 and mpu_scale = 1, m_probe_update[s] is chi[n, s].

Every output lies in a buffer with a guard pattern behind it and starts from
garbage (m_probe_update, which the entry adds to, from zero).  The bounds are
those of tests/noise_models.py; unmeasured pixels must hold their stated value
exactly.  The worst error / bound of every (entry, detector, model, data type)
is printed after the module (profiles/noise_model_entries.md)."""
import functools

import numpy as np
import pytest

import noise_models as nm

pytestmark = pytest.mark.gpu

STORED = [c.name for c in nm.CASES if c.kind == "stored"]
HANDOFF = [c.name for c in nm.CASES if c.kind == "handoff"]
GUARD = 64
PATTERN = np.arange(GUARD, dtype=np.float32) * 0.25 - 321.0
WORST = {}  # (entry, det, model, data type) -> worst error / bound


@pytest.fixture(scope="module", autouse=True)
def _report_worst_ratios():
    """After the module: the worst error / bound of every group it saw."""
    yield
    for key in sorted(WORST):
        print("WORST", *key, "{:.4f}".format(WORST[key]))


def _api():
    import tike_amd._arrays as A
    from tike_amd._lib import check, lib
    return A, check, lib


def _note(entry, c, model, err, bound):
    """The worst error / bound of an output (0 / 0 = 0; a NaN is infinite)."""
    err, bound = np.asarray(err, np.float64), np.asarray(bound, np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        r = np.where(err <= bound, np.where(bound > 0, err / bound, 0.0),
                     np.where(bound > 0, err / bound, np.inf))
    r = np.where(np.isnan(r), np.inf, r)
    worst = float(np.max(r))
    key = (entry, c.det, "-" if model is None else nm.MODELS[model],
           "u16" if c.u16 else "f32")
    WORST[key] = max(WORST.get(key, 0.0), worst)
    print("RATIO {} {} {} {:.4f}".format(entry, c.name, key[2], worst))
    return worst


class Guarded:
    """A float32 / complex64 device buffer with GUARD floats of PATTERN behind
    its logical end, which must come back untouched."""

    def __init__(self, host):
        A, _, _ = _api()
        host = np.ascontiguousarray(host)
        self.dtype, self.shape = host.dtype, host.shape
        flat = host.view(np.float32).ravel()
        self.n = flat.size
        self.t = A.to_device(np.concatenate([flat, PATTERN]))

    def ptr(self, offset=0):
        return self.t.data_ptr() + 4 * offset

    def get(self):
        host = self.t.cpu().numpy()
        np.testing.assert_array_equal(host[self.n:], PATTERN,
                                      err_msg="written past the end")
        return host[:self.n].copy().view(self.dtype).reshape(self.shape)


def _garbage(shape, dtype=np.float32):
    return Guarded(np.full(shape, np.nan, dtype))


def _device_data(P):
    """The counts as the case stores them (uint16 stays 2 bytes wide) and the
    mask."""
    import torch
    A, _, _ = _api()
    c = P["case"]
    if c.u16:
        data = torch.from_numpy(P["data"].view(np.int16).copy()).to(
            A.current_device())
    else:
        data = A.to_device(P["data"])
    assert data.element_size() == (2 if c.u16 else 4)
    mask = None if P["mask"] is None else A.to_device(
        P["mask"].astype(np.uint8))
    return data, mask


def _on(P):
    c = P["case"]
    return np.ones((c.det, c.det), bool) if P["mask"] is None else P["mask"]


def _check_factor(entry, P, model, got, R, ums):
    on = _on(P)
    np.testing.assert_array_equal(got[:, ~on], np.float32(ums) -
                                  np.float32(1))
    worst = _note(entry + " factor", P["case"], model,
                  np.abs(got - R["factor"])[:, on], R["factor_bound"][:, on])
    assert worst <= 1.0


def _check_costs(entry, P, model, got, R):
    worst = _note(entry + " costs", P["case"], model,
                  np.abs(got - R["costs"]), R["costs_bound"])
    assert worst <= 1.0, (got, R["costs"])


def _check_steps(entry, P, got, R, key):
    err, bound = np.abs(got - R[key]), R[key + "_bound"]
    print("PATTERNS {} {}".format(entry, " ".join(
        "{}={:.3f}".format(k, r) for k, r in zip(
            P["kinds"], (err / bound).max(axis=1)))))
    worst = _note(entry, P["case"], 1, err, bound)
    assert worst <= 1.0, (got, R[key])


def _check_intensity(entry, P, model, got, R):
    assert _note(entry + " intensity", P["case"], model,
                 np.abs(got - R["I"]), R["dI"]) <= 1.0


def _check_gradient(entry, P, model, got, R, ums, sign=1.0):
    """F factor: measured pixels within the bound; unmeasured ones the single
    float32 product F (unmeasured_scaling - 1), bit for bit."""
    on = _on(P)
    if not on.all():
        g = np.float32(ums) - np.float32(1)
        F32 = np.asarray(P["F32"])
        want = (F32.real * g + 1j * (F32.imag * g)).astype(np.complex64)
        np.testing.assert_array_equal(got[..., ~on], want[..., ~on])
    worst = _note(entry + " gradient", P["case"], model,
                  np.abs(got - sign * R["gradient"])[..., on],
                  R["gradient_bound"][..., on])
    assert worst <= 1.0


# --------------------------------------------------------- stored-input entries
@pytest.mark.parametrize("name", STORED)
def test_stored_input_entries_vs_model(name):
    """tike_gradient_scale, tike_farplane_gradient and, without a mask,
    tike_cost_each_pattern and tike_objective_grad, under both noise models."""
    A, check, lib = _api()
    P = nm.inputs(name)
    c = P["case"]
    N, S, det, npix = c.N, c.S, c.det, c.det * c.det
    ums, nmeas = nm.UNMEASURED, P["num_measured"]
    data, mask = _device_data(P)
    I32, F32 = A.to_device(P["I32"]), A.to_device(P["F32"])
    st = A.stream_ptr()
    for model in (0, 1):
        R = nm.reference(name, model, ums, True)  # reads the stored intensity
        gs, costs = _garbage((N, det, det)), _garbage(N)
        check(lib.tike_gradient_scale(
            A.ptr(I32), A.ptr(data), A.ptr(mask), gs.ptr(), costs.ptr(), N,
            det, model, ums, nmeas, st), "tike_gradient_scale")
        _check_factor("tike_gradient_scale", P, model, gs.get(), R, ums)
        _check_costs("tike_gradient_scale", P, model, costs.get(), R)
        R = nm.reference(name, model, ums)  # forms the intensity itself
        far = Guarded(np.asarray(P["F32"]))
        inten, costs = _garbage((N, det, det)), _garbage(N)
        check(lib.tike_farplane_gradient(
            far.ptr(), A.ptr(data), A.ptr(mask), inten.ptr(), costs.ptr(), N,
            S, det, model, 1, ums, nmeas, st), "tike_farplane_gradient")
        _check_intensity("tike_farplane_gradient", P, model, inten.get(), R)
        _check_costs("tike_farplane_gradient", P, model, costs.get(), R)
        _check_gradient("tike_farplane_gradient", P, model, far.get(), R, ums)
        # ... and without the gradient: the far plane comes back bit for bit
        far = Guarded(np.asarray(P["F32"]))
        costs = _garbage(N)
        check(lib.tike_farplane_gradient(
            far.ptr(), A.ptr(data), A.ptr(mask), None, costs.ptr(), N, S, det,
            model, 0, ums, nmeas, st), "tike_farplane_gradient")
        np.testing.assert_array_equal(far.get(), P["F32"])
        _check_costs("tike_farplane_gradient (costs only)", P, model,
                     costs.get(), R)
        if c.masked:
            continue
        R = nm.reference(name, model, ums, True)
        costs = _garbage(N)
        check(lib.tike_cost_each_pattern(
            A.ptr(data), A.ptr(I32), costs.ptr(), N, npix, model, st),
            "tike_cost_each_pattern")
        _check_costs("tike_cost_each_pattern", P, model, costs.get(), R)
        out = _garbage((N, S, det, det), np.complex64)
        check(lib.tike_objective_grad(
            A.ptr(data), A.ptr(F32), A.ptr(I32), out.ptr(), N, S, npix, model,
            st), "tike_objective_grad")
        _check_gradient("tike_objective_grad", P, model, out.get(), R, ums,
                        sign=-1.0)


@pytest.mark.parametrize("dominant", [0, 1])
@pytest.mark.parametrize("name", STORED)
def test_poisson_steps_vs_model(name, dominant):
    """tike_poisson_steps: S <= 8 with an even pixel count runs the
    one-workgroup kernel (24^2 inside its first trip, 48^2 several trips and
    a tail), S = 9 and 15^2 the per-tile one; dominant mode its own."""
    A, check, lib = _api()
    P = nm.inputs(name)
    c = P["case"]
    R = nm.reference(name, 1, nm.UNMEASURED, True)
    data, mask = _device_data(P)
    I32, F32 = A.to_device(P["I32"]), A.to_device(P["F32"])
    steps = _garbage((c.N, c.S))
    check(lib.tike_poisson_steps(
        A.ptr(F32), A.ptr(I32), A.ptr(data), A.ptr(mask), steps.ptr(), c.N,
        c.S, c.det, nm.STEP_START, nm.WEIGHT, dominant, A.stream_ptr()),
        "tike_poisson_steps")
    _check_steps("tike_poisson_steps " + ("dominant" if dominant else "all"),
                 P, steps.get(), R, "steps_dominant" if dominant else
                 "steps_all")


@pytest.mark.parametrize("name", [n for n in STORED if "x3n" in n or "x9n"
                                  in n])
def test_scale_modes_vs_model(name):
    """tike_scale_modes: one float32 product per component on measured
    pixels, nothing elsewhere."""
    A, check, lib = _api()
    P = nm.inputs(name)
    c = P["case"]
    on = _on(P)
    _, mask = _device_data(P)
    steps = nm.reference(name, 1)["steps_all"].astype(np.float32)
    far = Guarded(np.asarray(P["F32"]))
    steps_d = A.to_device(steps)
    check(lib.tike_scale_modes(far.ptr(), A.ptr(steps_d), A.ptr(mask),
                               c.N * c.S, c.det, A.stream_ptr()),
          "tike_scale_modes")
    got = far.get()
    np.testing.assert_array_equal(got[..., ~on], P["F32"][..., ~on])
    want = P["F"] * steps.astype(np.float64)[:, :, None, None]
    err = got.astype(np.complex128) - want
    bound = nm.U * np.abs(want)
    assert _note("tike_scale_modes", c, None,
                 np.maximum(np.abs(err.real), np.abs(err.imag))[..., on],
                 bound[..., on]) <= 1.0


# ------------------------------------------------------------ hand-off entries
@functools.lru_cache(maxsize=1)
def _scratch(det, S, N):
    """The forward hand-off of tike_fwd_pass1 for a shape: the object
    identically 1, whole-number positions, the case's per-position probes."""
    import torch
    A, check, lib = _api()
    name = "handoff-{}x{}n{}-all".format(det, S, N)
    P = nm.inputs(name)
    HW = det + 8
    psi = A.to_device(np.ones((1, HW, HW), np.complex64))
    scan = A.to_device(np.array([[1, 1], [2, 3], [4, 2]], np.float32)[:N])
    probe = A.to_device(P["probe"])
    scratch = torch.full((N, S, det, det), float("nan"), dtype=torch.complex64,
                         device=psi.device)
    check(lib.tike_fwd_pass1(
        A.ptr(psi), A.ptr(scan), A.ptr(probe), 1, None, None, None, 0, 0,
        A.ptr(scratch), None, N, S, det, det, HW, HW, A.stream_ptr()),
        "tike_fwd_pass1")
    torch.cuda.synchronize()
    return scratch


def _chi_from_work(P, work, steps=None):
    """chi (N, S, det, det) of a `work` buffer (a Guarded, or a tensor):
    tike_ifft2_pass2_gradients[_scaled] per position, patches identically 1."""
    A, check, lib = _api()
    c = P["case"]
    N, S, det = c.N, c.S, c.det
    ones = A.to_device(np.ones((1, det, det), np.complex64))
    out = []
    base = work.ptr() if isinstance(work, Guarded) else A.ptr(work)
    for n in range(N):
        mpu = Guarded(np.zeros((S, det, det), np.complex64))
        at = base + 8 * n * S * det * det
        if steps is None:
            check(lib.tike_ifft2_pass2_gradients(
                at, A.ptr(ones), None, None, None, 0, 0, None, None, mpu.ptr(),
                1.0, 1, S, det, P["scale"], A.stream_ptr()),
                "tike_ifft2_pass2_gradients")
        else:
            check(lib.tike_ifft2_pass2_gradients_scaled(
                at, A.ptr(ones), None, None, None, 0, 0, None, None, mpu.ptr(),
                1.0, 1, S, det, P["scale"], steps.ptr(n * S), A.stream_ptr()),
                "tike_ifft2_pass2_gradients_scaled")
        out.append(mpu.get())
    return np.stack(out)


def _check_chi(entry, P, model, got, ums, with_steps):
    want, bound = nm.chi_reference(P["case"].name, model, ums, with_steps)
    err = np.linalg.norm(got.astype(np.complex128) - want, axis=(-2, -1))
    assert _note(entry + " chi", P["case"], model, err, bound) <= 1.0, (
        err / bound)


@pytest.mark.parametrize("name", HANDOFF)
def test_fwd_gradient_scale_vs_model(name):
    """tike_fwd_gradient_scale with every optional output: the factor, the
    intensity, the costs and the far plane, under both noise models."""
    A, check, lib = _api()
    P = nm.inputs(name)
    c = P["case"]
    N, S, det = c.N, c.S, c.det
    ums = nm.UNMEASURED
    scratch = _scratch(det, S, N)
    data, mask = _device_data(P)
    for model in (0, 1):
        R = nm.reference(name, model, ums)
        gs, inten, costs = (_garbage((N, det, det)), _garbage((N, det, det)),
                            _garbage(N))
        far = _garbage((N, S, det, det), np.complex64)
        check(lib.tike_fwd_gradient_scale(
            A.ptr(scratch), A.ptr(data), int(c.u16), A.ptr(mask), gs.ptr(),
            inten.ptr(), costs.ptr(), far.ptr(), N, S, det, P["scale"], model,
            ums, P["num_measured"], A.stream_ptr()), "tike_fwd_gradient_scale")
        _check_intensity("tike_fwd_gradient_scale", P, model, inten.get(), R)
        _check_factor("tike_fwd_gradient_scale", P, model, gs.get(), R, ums)
        _check_costs("tike_fwd_gradient_scale", P, model, costs.get(), R)
        # the far plane: the forward error scale, and its own rounding
        e = P["e"][:, :, None, None]
        assert _note("tike_fwd_gradient_scale farplane", c, model,
                     np.abs(far.get() - P["F"]),
                     e + nm.U * np.abs(P["F"])) <= 1.0


@pytest.mark.parametrize("name", HANDOFF)
def test_one_launch_gradient_pass_vs_model(name):
    """tike_fwd_grad_ifft2_pass1: the costs, and chi through the fused pass
    2 (two sweeps for S <= 5, the resident kernel above; 512^2 its own)."""
    A, check, lib = _api()
    P = nm.inputs(name)
    c = P["case"]
    N, S, det = c.N, c.S, c.det
    ums = nm.UNMEASURED
    scratch = _scratch(det, S, N)
    data, mask = _device_data(P)
    for model in (0, 1):
        R = nm.reference(name, model, ums)
        costs = _garbage(N)
        work = _garbage((N, S, det, det), np.complex64)
        check(lib.tike_fwd_grad_ifft2_pass1(
            A.ptr(scratch), A.ptr(data), int(c.u16), A.ptr(mask), costs.ptr(),
            work.ptr(), N, S, det, P["scale"], model, ums, P["num_measured"],
            A.stream_ptr()), "tike_fwd_grad_ifft2_pass1")
        _check_costs("tike_fwd_grad_ifft2_pass1", P, model, costs.get(), R)
        work.get()  # (the guard)
        _check_chi("tike_fwd_grad_ifft2_pass1", P, model,
                   _chi_from_work(P, work), ums, False)


@pytest.mark.parametrize("name", HANDOFF)
def test_poisson_steps_handoff_vs_model(name):
    """tike_poisson_steps_handoff: the factor, the costs and the step lengths;
    then tike_grad_ifft2_pass1 with those steps, judged as chi."""
    A, check, lib = _api()
    P = nm.inputs(name)
    c = P["case"]
    N, S, det = c.N, c.S, c.det
    ums = nm.UNMEASURED
    R = nm.reference(name, 1, ums)
    scratch = _scratch(det, S, N)
    data, mask = _device_data(P)
    gs, costs, steps = _garbage((N, det, det)), _garbage(N), _garbage((N, S))
    sums = _garbage((N, S, 2))
    check(lib.tike_poisson_steps_handoff(
        A.ptr(scratch), A.ptr(data), int(c.u16), A.ptr(mask), gs.ptr(),
        costs.ptr(), steps.ptr(), sums.ptr(), N, S, det, P["scale"], ums,
        P["num_measured"], nm.STEP_START, nm.WEIGHT, A.stream_ptr()),
        "tike_poisson_steps_handoff")
    sums.get()
    _check_factor("tike_poisson_steps_handoff", P, 1, gs.get(), R, ums)
    _check_costs("tike_poisson_steps_handoff", P, 1, costs.get(), R)
    _check_steps("tike_poisson_steps_handoff steps", P, steps.get(), R,
                 "steps_all")
    work = _garbage((N, S, det, det), np.complex64)
    check(lib.tike_grad_ifft2_pass1(
        A.ptr(scratch), gs.ptr(), steps.ptr(), A.ptr(mask), S, work.ptr(),
        N * S, det, P["scale"], A.stream_ptr()), "tike_grad_ifft2_pass1")
    work.get()
    _check_chi("tike_grad_ifft2_pass1", P, 1, _chi_from_work(P, work), ums,
               True)


@pytest.mark.parametrize("name", [n for n in HANDOFF if "-256x" in n])
def test_one_launch_poisson_pass_vs_model(name):
    """tike_poisson_steps_grad_ifft2_pass1 (no mask, or the mask with scaling
    1; two sweeps for S <= 5, the resident route above), finished by
    tike_ifft2_pass2_gradients_scaled with the step lengths it left."""
    A, check, lib = _api()
    P = nm.inputs(name)
    c = P["case"]
    N, S, det = c.N, c.S, c.det
    ums = 1.0 if c.masked else nm.UNMEASURED
    R = nm.reference(name, 1, ums)
    scratch = _scratch(det, S, N)
    data, mask = _device_data(P)
    costs, steps, sums = _garbage(N), _garbage((N, S)), _garbage((N, S, 2))
    work = _garbage((N, S, det, det), np.complex64)
    check(lib.tike_poisson_steps_grad_ifft2_pass1(
        A.ptr(scratch), A.ptr(data), int(c.u16), A.ptr(mask), costs.ptr(),
        steps.ptr(), sums.ptr(), work.ptr(), N, S, det, P["scale"], ums,
        P["num_measured"], nm.STEP_START, nm.WEIGHT, A.stream_ptr()),
        "tike_poisson_steps_grad_ifft2_pass1")
    sums.get()
    work.get()
    _check_costs("tike_poisson_steps_grad_ifft2_pass1", P, 1, costs.get(), R)
    _check_steps("tike_poisson_steps_grad_ifft2_pass1 steps", P, steps.get(),
                 R, "steps_all")
    _check_chi("tike_poisson_steps_grad_ifft2_pass1", P, 1,
               _chi_from_work(P, work, steps), ums, True)


def test_refused_cases_are_unsupported():
    """512^2 with five modes (tike_poisson_steps_handoff holds |F_s|^2 of at
    most four), and a mask with scaling 0.7, or 512^2, for the one-launch
    poisson entry.  Nothing is written."""
    import torch
    A, _, lib = _api()
    from tike_amd._lib import ERR_UNSUPPORTED
    b = torch.zeros(1024, dtype=torch.float32, device=A.current_device())
    p, st = A.ptr(b), A.stream_ptr()
    assert lib.tike_poisson_steps_handoff(
        p, p, 0, None, p, p, p, p, 2, 5, 512, 1.0 / 512, 0.7, 512 * 512,
        nm.STEP_START, nm.WEIGHT, st) == ERR_UNSUPPORTED
    w = torch.zeros(1024, dtype=torch.float32, device=b.device)
    m = torch.ones(256 * 256, dtype=torch.uint8, device=b.device)
    args = (p, p, 0, A.ptr(m), p, p, p, A.ptr(w), 1, 3, 256, 1.0 / 256)
    assert lib.tike_poisson_steps_grad_ifft2_pass1(
        *args, 0.7, 256 * 256, nm.STEP_START, nm.WEIGHT, st) == ERR_UNSUPPORTED
    assert lib.tike_poisson_steps_grad_ifft2_pass1(
        p, p, 0, None, p, p, p, A.ptr(w), 2, 1, 512, 1.0 / 512, 0.7,
        512 * 512, nm.STEP_START, nm.WEIGHT, st) == ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert float(b.abs().sum()) == 0.0 and float(w.abs().sum()) == 0.0
