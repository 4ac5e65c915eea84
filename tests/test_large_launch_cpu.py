"""The large-launch helpers (tests/large_launch.py) on the CPU: the float64
chunk model against oracle/ on the base problem of every case, the aliasing
property of the replica construction, `positions_for`, and a model of the
chunk policy (every case really is one launch)."""
import functools

import numpy as np
import pytest

import large_launch as ll
from util import COST_RTOL, OP_NORMWISE, assert_close

IDS = [c["name"] for c in ll.CHUNK_CASES]


def _mask(det, on, seed=9):
    m = np.ones((det, det), dtype=bool)
    if on:
        m = np.random.default_rng(seed).random((det, det)) > 0.1
    return m


@functools.lru_cache(maxsize=None)
def _base(det, S, n0):
    return ll.base_problem(det, S, n0, seed=3 * det + S)


# (the case under the deterministic switch shares its base problem with the
# case without it)
MODEL_CASES = [c for c in ll.CHUNK_CASES if not c.get("deterministic")]


@pytest.mark.parametrize("case", MODEL_CASES,
                         ids=[c["name"] for c in MODEL_CASES])
def test_chunk_model_agrees_with_the_oracle(case):
    """The float64 model and the float32 oracle, written separately from the
    same reference lines, agree on the n0 base positions to the operator
    bars: patches OP_NORMWISE, chi and both gradients 2e-5, costs COST_RTOL,
    position sums as `_minibatch_vs_oracle` holds them."""
    from oracle import solvers as osol
    det, S, n0 = case["det"], case["S"], case["n0"]
    b = _base(det, S, n0)
    mask = _mask(det, case.get("u16_mask"))
    noise = case.get("noise_model", "gaussian")
    m = ll.chunk_model(b["psi"], b["scan"], b["probe"], b["eigen"],
                       b["weights"], b["data"], mask, det, noise_model=noise)
    o = osol.get_nearplane_gradients(
        b["data"], b["psi"], b["scan"], b["probe"], b["eigen"], b["weights"],
        0, n0, num_batch=1, detector_shape=det, measured_pixels=mask,
        noise_model=noise, recover_positions=True)
    assert_close(o["patches"][:, 0, 0], m["patches"], OP_NORMWISE,
                 what="patches")
    assert_close(o["chi"][:, 0], m["chi"], 2e-5, what="chi")
    assert_close(o["object_upd_sum"][0], m["object_upd_sum"], 2e-5,
                 what="object_upd_sum")
    assert_close(o["m_probe_update"][0, 0], m["m_probe_update"], 2e-5,
                 what="m_probe_update")
    np.testing.assert_allclose(np.ravel(o["costs"]), m["costs"],
                               rtol=COST_RTOL)
    np.testing.assert_allclose(
        o["position_numerator"], m["position_numerator"], rtol=2e-3,
        atol=1e-4 * np.abs(m["position_numerator"]).max())
    np.testing.assert_allclose(o["position_denominator"],
                               m["position_denominator"], rtol=2e-3)


def test_operator_models_agree_with_the_oracle():
    from oracle import operators as oop
    det, S, n0 = 64, 3, 5
    b = ll.base_problem(det, S, n0, seed=1, eigen=False)
    far = ll.ptycho_fwd(b["probe"], b["scan"], b["psi"][0], det)
    assert_close(oop.ptycho_fwd(b["probe"], b["scan"], b["psi"], det)[:, 0],
                 far, what="ptycho_fwd")
    rng = np.random.default_rng(2)
    f = (rng.standard_normal((n0, 1, S, det, det)) +
         1j * rng.standard_normal((n0, 1, S, det, det))).astype(np.complex64)
    bprobe = np.broadcast_to(b["probe"], (n0, 1, S, det, det)).copy()
    o_psi, o_probe = oop.ptycho_adj(f, bprobe, b["scan"], b["psi"])
    psi_adj, probe_adj = ll.ptycho_adj(f[:, 0], bprobe[:, 0], b["scan"],
                                       b["psi"][0])
    assert_close(o_psi[0], psi_adj, what="psi_adj")
    assert_close(o_probe[:, 0], probe_adj, what="probe_adj")
    x = f[0, 0]
    np.testing.assert_allclose(ll.ifft2(ll.fft2(x)), x, atol=1e-12)
    np.testing.assert_allclose(np.linalg.norm(ll.fft2(x)), np.linalg.norm(x))


# ------------------------------------------------------------- replicas
@pytest.mark.parametrize("case", ll.CHUNK_CASES, ids=IDS)
def test_no_wrap_distance_is_a_whole_number_of_replicas(case):
    strides, tiles = ll.case_strides(case)
    ll.assert_no_aliasing(strides, tiles, case["n0"])
    # the property is computed: the far plane of 256^2 x 8 modes wraps 2^32
    # bytes onto the position 1024 behind
    if (case["det"], case["S"]) == (256, 8):
        assert ("far / mid", "2^32 bytes", 1024) in ll.aliasing_distances(
            strides, tiles, case["n0"])
    assert case["N"] % case["n0"] == 0


def test_aliasing_is_detected(monkeypatch):
    """The distances are computed: a 4 MiB far plane wraps 2^32 bytes onto the
    position 1024 behind.  Powers of two never divide into odd replicas; a
    distance that does (5 x 2^30 bytes = 1280 such positions, n0 = 5) is
    refused, and so is an even or a small n0."""
    strides = {"far": 1 << 22}
    assert ("far", "2^32 bytes", 1024) in ll.aliasing_distances(
        strides, (1,), 5)
    ll.assert_no_aliasing(strides, (1, 8), 5)
    for n0 in (4, 3, 8):
        with pytest.raises(AssertionError):
            ll.assert_no_aliasing(strides, (1,), n0)
    monkeypatch.setitem(ll.WRAP_BYTES, "5 x 2^30 bytes", 5 << 30)
    with pytest.raises(AssertionError, match="identical replica"):
        ll.assert_no_aliasing(strides, (1,), 5)
    ll.assert_no_aliasing(strides, (1,), 7)


def test_positions_for():
    # the issue's byte axis: 256^2 x 8 modes, n0 = 5, just over 4 GiB
    assert ll.positions_for(8 * 256 * 256 * 8, 5, 1 << 32) == 1030
    assert ll.positions_for(1, 7, 1 << 16) == 65548
    for span, n0, thr in [(8 * 256 * 256 * 8, 5, 1 << 32),
                          (12 * 65536 * 8, 5, 1 << 32), (1, 7, 1 << 16),
                          (8 * 65536, 5, 1 << 32), (300 * 300 * 16, 5, 1 << 32),
                          (3, 7, 10), (5, 5, 0)]:
        N = ll.positions_for(span, n0, thr)
        assert N % n0 == 0
        assert N * span >= thr + n0 * span      # one whole replica beyond
        assert (N - n0) * span < thr + n0 * span  # ... and the smallest such


# ------------------------------------------------------------ the policy
@pytest.mark.parametrize("case", ll.CHUNK_CASES, ids=IDS)
def test_chunk_policy_puts_every_case_into_one_launch(case):
    """`chunk_positions` without an override admits the whole batch of every
    case (the GPU tests assert the same on the plan they ran)."""
    from tike_amd.ptycho.solvers import lstsq as L
    assert not L.CHUNK_POSITIONS_OVERRIDE
    position_major = case["route"] != "unfused"
    assert L.chunk_positions(case["S"], case["det"],
                             position_major) >= case["N"]
    if case["axis"] == "bytes":
        assert case["N"] * case["S"] * case["det"] ** 2 * 8 > 1 << 32
    else:
        assert case["N"] > 1 << 16


def test_multislice_rpie_model_agrees_with_the_oracle():
    """Two slices, 64^2 x 3 modes: costs, both numerators of both slices."""
    from oracle import operators as oop
    from oracle import solvers as osol
    det, S, n0, D = 64, 3, 5, 2
    b = ll.base_problem(det, S, n0, seed=5, eigen=False)
    rng = np.random.default_rng(6)
    psi = np.concatenate([b["psi"], (1 + 0.1 * (rng.standard_normal(
        b["psi"].shape) + 1j * rng.standard_normal(b["psi"].shape))).astype(
            np.complex64)])
    prop = oop.fresnel_spectrum_propagator((det, det), (2e-6, 2e-6), 1e-6,
                                           1e-10)
    m = ll.multislice_rpie_model(psi, b["scan"], b["probe"], b["data"], prop)
    costs, psi_num, probe_num, _ = osol.rpie_gradients(
        b["data"], psi, b["scan"], b["probe"], None, None, 0, n0,
        np.zeros_like(psi), detector_shape=det,
        measured_pixels=np.ones((det, det), dtype=bool), propagator=prop)
    np.testing.assert_allclose(np.ravel(costs), m["costs"], rtol=COST_RTOL)
    assert_close(psi_num, m["psi_num"], 2e-5, what="psi_num")
    assert_close(probe_num[:, 0, 0], m["probe_num"], 2e-5, what="probe_num")
