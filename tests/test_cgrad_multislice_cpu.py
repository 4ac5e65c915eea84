"""Multislice cgrad without a GPU: the float64 model (tests/cgrad_multislice.py)
against finite differences of its own cost, against tests/cgrad_models.py at
one slice and against the oracle's adjoint; how clearly the model's line
searches are decided on the problems the GPU test compares; the propagator's
phase spread; every refusal; the ABI."""
import numpy as np
import pytest

import cgrad_models as cm
import cgrad_multislice as ms
import fly_scan as fs
from oracle import operators as ops
from util import relerr

SMALL = dict(obj=72, pw=32, S=2, N=9, seed=4)


def _small(D):
    return ms.problem(D=D, **SMALL)


def _direction(rng, shape):
    return rng.standard_normal(shape) + 1j * rng.standard_normal(shape)


# --------------------------------------------------------- finite differences
@pytest.mark.parametrize("D", [1, 2, 3])
@pytest.mark.parametrize("model", ["gaussian", "poisson"])
@pytest.mark.parametrize("use_mask", [False, True])
def test_gradient_against_finite_differences(D, model, use_mask):
    """cost(x + h v) - cost(x - h v) over 2 h Re<grad, v> is 2 / (N n_measured)
    to 1e-4, for the object (all slices at once) and for the probe."""
    P = _small(D)
    pw, N = SMALL["pw"], SMALL["N"]
    mask = fs.block_mask(pw) if use_mask else None
    # counts of another object: the gradient is far from zero
    data = ms.simulate(P["probe"], P["scan"], P["psi"], P["H"])
    data = fs.masked(data, mask) if use_mask else data.astype(np.float32)
    psi = np.asarray(P["psi0"], np.complex128)
    probe = np.asarray(P["probe0"], np.complex128)
    gpsi, gprobe = ms.gradients(model, data, psi, P["scan"], probe, P["H"],
                                mask)
    assert gpsi.shape == psi.shape and gprobe.shape == probe.shape
    rng = np.random.default_rng(D)
    h = 1e-6
    want = 2.0 / (N * (mask.sum() if use_mask else pw * pw))
    f = lambda a, b: ms.cost(model, data, a, P["scan"], b, P["H"], mask)
    v = _direction(rng, psi.shape)
    ratio = ((f(psi + h * v, probe) - f(psi - h * v, probe)) / (2 * h)
             / np.sum(np.conj(gpsi) * v).real)
    print(f"D={D} {model} mask={use_mask}: object ratio / want "
          f"{ratio / want:.8f}")
    assert abs(ratio / want - 1) <= 1e-4
    v = _direction(rng, probe.shape)
    ratio = ((f(psi, probe + h * v) - f(psi, probe - h * v)) / (2 * h)
             / np.sum(np.conj(gprobe) * v).real)
    print(f"D={D} {model} mask={use_mask}: probe ratio / want "
          f"{ratio / want:.8f}")
    assert abs(ratio / want - 1) <= 1e-4


# ------------------------------------------------ one slice: the cgrad model
@pytest.mark.parametrize("model", ["gaussian", "poisson"])
def test_one_slice_is_the_cgrad_model(model):
    P = _small(1)
    pw = SMALL["pw"]
    mask = fs.block_mask(pw)
    data = fs.masked(P["data"], mask)
    a = ms.cost(model, data, P["psi0"], P["scan"], P["probe0"], P["H"], mask)
    b = cm.cost(model, data, P["psi0"], P["scan"], P["probe0"], pw, mask)
    assert abs(a - b) <= 1e-6 * abs(b)
    gpsi, gprobe = ms.gradients(model, data, P["psi0"], P["scan"],
                                P["probe0"], P["H"], mask)
    e_psi = relerr(gpsi, cm.grad_psi(model, data, P["psi0"], P["scan"],
                                     P["probe0"], pw, mask))
    e_probe = relerr(gprobe, cm.grad_probe(model, data, P["psi0"], P["scan"],
                                           P["probe0"], pw, mask))
    print(f"{model}: object {e_psi:.2e} probe {e_probe:.2e}")
    assert e_psi <= 1e-6 and e_probe <= 1e-6


# ------------------------------------------------------- the oracle's adjoint
@pytest.mark.parametrize("D", [2, 3])
def test_adjoint_against_the_oracle(D):
    """D x the oracle's object adjoint (it divides by D) and its probe
    adjoint, of the same far plane, to 1e-5 normwise."""
    P = _small(D)
    N = SMALL["N"]
    far, beams = ms.fwd(P["probe0"], P["scan"], P["psi0"], P["H"])
    far = far.astype(np.complex64)
    psi_adj, probe_adj = ms.adj(far, beams, P["scan"], P["psi0"], P["H"])
    uprobe = np.broadcast_to(P["probe0"], (N, *P["probe0"].shape[1:]))
    o_psi, o_probe = ops.ptycho_adj(far[:, None], uprobe, P["scan"],
                                    P["psi0"],
                                    propagator=P["H"].astype(np.complex64))
    e_psi = relerr(D * o_psi, psi_adj)
    e_probe = relerr(np.sum(o_probe, axis=0, keepdims=True), probe_adj)
    print(f"D={D}: object {e_psi:.2e} probe {e_probe:.2e}")
    assert e_psi <= 1e-5 and e_probe <= 1e-5


# ---------------------------------------------------------------- the margins
@pytest.mark.parametrize("case", sorted(ms.SOLVER_CASES))
def test_line_searches_of_the_solver_cases_are_clearly_decided(case):
    for variant in ms.SOLVER_VARIANTS:
        state, _, _ = ms.run_model(case, *variant)
        margin = min(state["margins"])
        print(case, variant, f"min margin {margin:.2e} over "
              f"{len(state['margins'])} comparisons, costs "
              f"{np.ravel(state['costs'])}")
        assert margin >= ms.MIN_MARGIN, (case, variant, margin)
        assert len(state["costs"]) == 2


@pytest.mark.parametrize("case", sorted(ms.SOLVER_CASES))
def test_propagator_is_not_trivial(case):
    spread = np.ptp(np.angle(ms.propagator(ms.SOLVER_CASES[case]["pw"])))
    print(case, f"phase spread {spread:.2f} rad")
    assert spread > 1


def test_propagator_phase_spread_at_32():
    assert abs(np.ptp(np.angle(ms.propagator(32))) - 2.9) < 0.1


def test_problem_positions_reach_both_corners():
    for kw in ms.SOLVER_CASES.values():
        P = ms.problem(**kw)
        floors = np.floor(P["scan"])
        assert floors[0].tolist() == [1, 1]
        assert floors[-1].tolist() == [kw["obj"] - kw["pw"] - 1] * 2
        assert np.any(P["scan"] != floors)  # fractional
        # the slices differ
        assert relerr(P["psi"][0], P["psi"][1]) > 0.1


# -------------------------------------------------------------- the refusals
def _parameters(tp, scan, options=None, slices=2, pw=16, **kw):
    return tp.PtychoParameters(
        probe=np.ones((1, 1, 1, pw, pw), np.complex64),
        psi=np.ones((slices, 64, 64), np.complex64), scan=scan,
        algorithm_options=options or tp.CgradOptions(num_batch=1),
        object_options=tp.ObjectOptions(), **kw)


def test_every_refusal():
    import tike_amd.ptycho as tp
    from tike_amd.ptycho.solvers.cgrad import _refuse_multislice
    rng = np.random.default_rng(2)
    scan = (2 + 40 * rng.random((12, 2))).astype(np.float32)
    data = np.zeros((12, 16, 16), np.float32)
    with_positions = _parameters(
        tp, scan, position_options=tp.PositionOptions(scan.copy()))
    with_eigen = _parameters(
        tp, scan, eigen_probe=np.ones((1, 1, 1, 16, 16), np.complex64),
        eigen_weights=np.ones((12, 2, 1), np.float32))
    for params, match in ((with_positions, "several slices.*position_options"),
                          (with_eigen, "several slices.*eigen probes")):
        with pytest.raises(NotImplementedError, match=match):
            tp.Reconstruction(data, params)
        with pytest.raises(NotImplementedError, match=match):
            _refuse_multislice(params)
    _refuse_multislice(_parameters(tp, scan))
    _refuse_multislice(_parameters(
        tp, scan, slices=1,
        position_options=tp.PositionOptions(scan.copy())))
    # fly scans keep their own message
    with pytest.raises(NotImplementedError,
                       match="fly=3 with several slices"):
        tp.Reconstruction(np.zeros((4, 16, 16), np.float32),
                          _parameters(tp, scan), fly=3)
    # probe window != detector: Multislice._check_slices' ValueError
    with pytest.raises(ValueError,
                       match="detector_shape == probe_shape"):
        tp.Reconstruction(np.zeros((12, 32, 32), np.float32),
                          _parameters(tp, scan))
    # lstsq_grad still takes one slice only
    with pytest.raises(NotImplementedError, match="psi.shape\\[0\\] > 1"):
        tp.Reconstruction(data, _parameters(
            tp, scan, options=tp.LstsqOptions(num_batch=1)))


# ------------------------------------------------------------------- the ABI
def test_abi_has_the_new_entry():
    """The entry is declared, exported and bound, and checks its arguments
    before it touches a device."""
    import ctypes

    import tike_amd._lib as L
    name = "tike_slice_step_back"
    assert L.ABI_VERSION >= 18
    assert name in L.declared_symbols()
    assert len(L._PROTOTYPES[name]) == 13
    assert hasattr(ctypes.CDLL(L.LIB_PATH), name)
    # argument checks come before any launch: no GPU needed
    fn = L.lib.tike_slice_step_back
    bufs = [ctypes.create_string_buffer(64) for _ in range(6)]
    p = [ctypes.cast(b, ctypes.c_void_p) for b in bufs]
    ok = (*p, 1, 1, 128, 200, 200, 1.0, None)

    def call(**change):
        args = list(ok)
        for k, v in change.items():
            args[int(k[1:])] = v
        return fn(*args)

    for i in (0, 1, 2, 3, 5):  # (objproj alone may be NULL)
        assert call(**{f"a{i}": None}) == L.ERR_ARG
    assert call(a4=p[0]) == L.ERR_ARG  # objproj aliases work
    assert call(a7=0) == L.ERR_ARG  # S
    assert call(a5=p[0]) == L.ERR_ARG  # farplane1 aliases work
    assert call(a7=9) == L.ERR_UNSUPPORTED
    assert call(a8=64) == L.ERR_UNSUPPORTED
    assert call(a8=512) == L.ERR_UNSUPPORTED  # (register budget)
    assert call(a6=0) == 0  # no position: no launch
