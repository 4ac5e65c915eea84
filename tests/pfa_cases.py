"""Inputs shared by test_pfa_entries_cpu.py, test_pfa_entries_gpu.py and
_pfa_entries_child.py: scan positions that reach every selection of the gather
and the probe arguments of the five probe forms."""
import numpy as np

import pfa_model as pm


def rc(rng, *shape):
    return (rng.random((*shape, 2), dtype=np.float32) - 0.5).view(
        np.complex64)[..., 0]


def object_shape(pw):
    """Non-square, a little larger than the window."""
    return pw + 9, pw + 14


def positions(pw, nscan, first=0):
    """`nscan` positions (y, x) f32 on an object of object_shape(pw), taken in a
    ring from the list below starting at `first`: integer positions, (0, 0),
    fractional ones, the last legal corner (H - pw - 1, W - pw - 1) with
    fractions, one row past it (sy = H - pw), one column past it (sx = W - pw,
    the last of the list), and windows hanging over each
    of the four sides, a coordinate of -0.5 among them."""
    H, W = object_shape(pw)
    special = [
        (3.0, 5.0),                          # integer
        (0.0, 0.0),
        (2.25, 7.625),                       # fractional
        (H - pw - 1 + 0.375, W - pw - 1 + 0.75),  # the last legal corner
        (H - pw + 0.5, 3.25),                # one row past it
        (-0.5, 4.5),                         # over the top, floor(-0.5) = -1
        (-3.0, 2.0),                         # ... by whole rows
        (H - pw + 4.25, 1.5),                # over the bottom
        (4.5, -0.5),                         # over the left
        (1.0, -6.75),
        (5.75, W - pw + 3.5),                # over the right
        (H - pw, W - pw),                    # integer, last row and column taps outside
        (-2.5, W - pw + 2.25),               # over a corner
        (6.0, 9.0),
        (0.5, 0.0),
        (8.125, 13.0625),
        (7.0, 0.9375),
        (3.25, W - pw + 0.5),                # one column past the last legal corner
    ]
    return np.array([special[(first + i) % len(special)] for i in range(nscan)],
                    np.float32).reshape(nscan, 2)


def probe_case(form, nscan, S, pw, seed, C=1, Sm=1):
    """Arrays of one probe form: dict(form, probe, weights, eigen, unique, C,
    Sm) as float32 / complex64 (None where the form has none), and `probes`,
    the float64 probe of every position."""
    rng = np.random.default_rng(seed)
    c = dict(form=form, weights=None, eigen=None, unique=None, C=0, Sm=0)
    if form == "per_scan":
        c["probe"] = rc(rng, nscan, S, pw, pw)
    else:
        c["probe"] = rc(rng, S, pw, pw)
    if form in ("weights", "eigen", "unique"):
        nC = C if form == "eigen" else 0
        w = (0.5 * rng.standard_normal((nscan, nC + 1, S))).astype(np.float32)
        w[:, 0] += 1.0
        c["weights"] = w
        c["C"] = nC
    if form == "eigen":
        c["eigen"], c["Sm"] = rc(rng, C, Sm, pw, pw), Sm
    if form == "unique":
        c["unique"], c["Sm"] = rc(rng, nscan, Sm, pw, pw), Sm
    c["probes"] = pm.probe_of_positions(form, nscan, c["probe"], c["weights"],
                                        c["eigen"], c["unique"])
    return c


# (det, S, positions) of the combine cases, seed det + S: p = 3 either side of
# the resident four modes, p = 5, 7, and the Cooley-Tukey sizes -- 2048 reads
# the far end of the twiddle table
COMBINE = [(96, 4, 2), (96, 5, 2), (160, 2, 2), (224, 2, 2), (1024, 1, 2),
           (2048, 1, 1)]


def combine_case(det, S, nscan):
    c = pm.combine_case(det, nscan, S, seed=det + S)
    pm.check_combine_case(c)
    return c


def random_object(pw, seed):
    H, W = object_shape(pw)
    return rc(np.random.default_rng(seed), H, W)
