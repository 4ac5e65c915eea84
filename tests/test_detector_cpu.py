"""`operators.detector`: the table of what goes with what has one definition;
this is its one test, under the naming of each of the four entries
(`simulate`, `autograd.cost`, `Ptycho.cost`, `Reconstruction`).  CPU only."""
import itertools

import numpy as np
import pytest

from tike_amd.operators import detector as D

# a model -> the keywords that say it is there
MODELS = dict(binning=dict(binning=2), background=dict(background=True),
              blur=dict(blur=True), nearfield=dict(nearfield=True),
              slices=dict(slices=2), eigen=dict(eigen=True))

# (the model that refuses, what it refuses): everything else goes together as
# far as the detector is concerned (binned data with several slices or eigen
# probes is the solver's to refuse: cgrad's `_REFUSALS`)
REFUSED = {
    ("nearfield", "binning"), ("nearfield", "background"),
    ("nearfield", "blur"), ("nearfield", "slices"), ("nearfield", "eigen"),
    ("blur", "binning"), ("blur", "background"), ("blur", "slices"),
    ("blur", "eigen"),
    ("background", "binning"), ("background", "slices"),
    ("background", "eigen"),
}

# what the other side is called: by simulate / autograd.cost / Ptycho.cost,
# and by Reconstruction
OTHER = dict(binning=("binning=2", "binning=2"),
             background=("a background", "background_options"),
             blur=("a blur", "blur_options"),
             slices=("several slices", "several slices"),
             eigen=("eigen probes", "eigen probes"))

# (naming, exception, the stem the tests of the four features match)
ENTRIES = [
    (D.SIMULATE, NotImplementedError, "{a} with {b}", 0),
    (D.entry("cost"), NotImplementedError, "cost: {a} with {b}", 0),
    (D.OPERATOR, ValueError, "{a} together with {b}", 0),
    (D.RECONSTRUCTION, NotImplementedError, "{a}_options with {b}", 1),
]


def _build(naming, names):
    kw = {}
    for name in names:
        kw.update(MODELS[name])
    values = dict(background=np.zeros((16, 16), np.float32),
                  blur=np.ones((3, 3), np.float32),
                  nearfield=np.ones((16, 16), np.complex64))
    kw = {k: values[k] if k in values else v for k, v in kw.items()}
    return D.build(naming, 16, **kw)


@pytest.mark.parametrize("naming,error,stem,column", ENTRIES,
                         ids=["simulate", "autograd", "operator",
                              "reconstruction"])
def test_every_pair(naming, error, stem, column):
    for pair in itertools.combinations(MODELS, 2):
        refusals = [(a, b) for a, b in (pair, pair[::-1]) if (a, b) in REFUSED]
        if not refusals:
            # (what is left goes together: at most binning beside slices or
            # eigen probes)
            assert _build(naming, pair).kind == (
                "binned" if "binning" in pair else "far"), pair
            continue
        (a, b), = refusals
        text = stem.format(a=a, b=OTHER[b][column])
        with pytest.raises(error) as raised:
            _build(naming, pair)
        assert text in str(raised.value), (pair, str(raised.value))
        # the same row through `refuse`, as the solver entries ask it
        with pytest.raises(error) as raised:
            D.refuse(a, naming, **MODELS[b])
        assert text in str(raised.value), (pair, str(raised.value))


def test_single_kinds_and_the_data_width():
    for name, kind in (("binning", "binned"), ("background", "background"),
                       ("blur", "blur"), ("nearfield", "nearfield")):
        assert _build(D.SIMULATE, (name,)).kind == kind
    assert D.build(D.SIMULATE, 16) == D.Detector("far", 1, None)
    assert D.Detector("binned", 4).width(32) == 8
    assert D.Detector("blur", 1, None).width(32) == 32
    # several slices or eigen probes alone are no business of the detector
    assert D.build(D.SIMULATE, 16, slices=3, eigen=True).kind == "far"
    assert D.build(D.SIMULATE, 16, binning=2, slices=3).kind == "binned"


def test_probe_window_in_the_near_field():
    H = np.ones((16, 16), np.complex64)
    for naming, error, stem, _ in ENTRIES:
        text = stem.format(a="nearfield", b="probe window 8 != detector 16")
        with pytest.raises(error) as raised:
            D.build(naming, 16, nearfield=H, window=8)
        assert text in str(raised.value)
        assert D.build(naming, 16, nearfield=H, window=16).kind == "nearfield"
    # (no other kind asks)
    assert D.build(D.SIMULATE, 16, blur=np.ones((3, 3), np.float32),
                   window=8).kind == "blur"


def test_value_checks_are_stated_once():
    """The host form and the device form of each value's checks, by the
    stems the tests of the features match."""
    import torch
    b = np.zeros((16, 16), np.float32)
    assert D.checked_background(b, 16) is b
    for bad, match in ((np.zeros((8, 8), np.float32), "background has shape"),
                       (np.zeros((16, 16)), "expected float32"),
                       (b - 1, "finite and >= 0"),
                       (b + np.float32("nan"), "finite and >= 0")):
        with pytest.raises(ValueError, match=match):
            D.checked_background(bad, 16)
    checked = D.checked(D.Detector("blur", 1, np.full((3, 3), 2, np.float32)),
                        16)
    np.testing.assert_allclose(checked.value, 1 / 9, rtol=1e-6)
    assert D.checked(D.Detector("binned", 2), 16) == D.Detector("binned", 2)
    for kind, good, dtype in (
            ("background", torch.zeros(16, 16), "torch.float32"),
            ("blur", torch.ones(3, 3), "torch.float32"),
            ("nearfield", torch.ones(16, 16, dtype=torch.complex64),
             "torch.complex64")):
        with pytest.raises(TypeError, match=f"{kind} must be a torch"):
            D.device_value("cost", kind, good.numpy(), 16)
        with pytest.raises(TypeError, match=f"{kind} must be {dtype}"):
            D.device_value("cost", kind, good.to(torch.complex128), 16)
        with pytest.raises(ValueError, match=f"cost: {kind} must be "):
            D.device_value("cost", kind, good[:2, :1], 16)
        with pytest.raises(TypeError, match="no CPU fallback"):
            D.device_value("cost", kind, good, 16)
    with pytest.raises(ValueError, match="wider than the detector"):
        D.device_value("cost", "blur", torch.ones(5, 5), 4)
    with pytest.raises(NotImplementedError, match="requires a gradient"):
        D.device_value("cost", "nearfield", torch.ones(
            16, 16, dtype=torch.complex64).requires_grad_(True), 16)
