"""A float64 / complex128 model of the overlap sums every solver ends in --
the bilinear patch gather with its sums over positions and modes, and the
footprint scatter back into the object -- and the table of cases both test
files walk.  NumPy only: it imports without torch or a GPU.

The model restates include/tike_amd.h and the header comments of
csrc/lstsq_gradients.hip and csrc/scatter.hip, not the kernels.  For an object
psi (H, W), positions scan (N, 2) float32 (y, x), chi (N, S, pw, pw) and the
probe P[n, s] of every position:

  corner   sy, sx = floor(scan), fy, fx = scan - floor(scan), both taken in
           float32 as tk_corner does; everything after that in float64
  weights  w00, w01, w10, w11 = (1-fx)(1-fy), fx(1-fy), (1-fx)fy, fx fy on the
           taps (y, x), (y, x+1), (y+1, x), (y+1, x+1)
  patches  O[n][y][x] = sum of the four weighted taps at (sy + y, sx + x)
  objproj  [n]  = sum_s conj(P[n, s]) chi[n, s]
  m_probe_update[s] += sum_n conj(O[n]) chi[n, s]
  probe preconditioner   out.real += sum_n |O[n]|^2, out.imag untouched
  scatter  image[sy + y + dy][sx + x + dx] += w_dydx v[n][y][x]: the adjoint
           of the gather, (pw + 1)^2 object pixels per position; a pixel
           outside the object is dropped.  One model for tike_scatter_patches
           (complex values), tike_psi_preconditioner (one real patch for every
           position) and tike_scatter_amplitudes (a real patch per position).

The probe of a position (TkProbe::at): `shared`; `weights`: probe_s x
weights[n][0][s]; `eigen`: that plus sum_c weights[n][c+1][s] eigen[c][s] on
the modes s < Sm only (the modes s >= Sm get the weight row 0 and nothing
else); `unique`: the modes s < Sm as given, the others as `weights`.  Without
weights the probe is the shared one whatever else is passed.

Out of scope: gather positions outside check_allowed_positions (1 <=
floor(scan) <= shape - pw - 1).  What a tap outside the object counts as
differs between kernels there -- tk_gather follows the reference's linear
addressing, the strip kernels take zero -- and check_allowed_positions keeps
every solver away from it; no gather case of the table leaves the range.
tike_eigen_pixel_update belongs to the minibatch tail (tests/lstsq_tail.py).

Bounds (the rule of cgrad_search.widened and tests/noise_models.py: never
from a kernel's output).  Every sum comes back as a `Sum`: its value, the same
sum with every term replaced by its modulus (`abs_terms`) and k, the number of
float32 roundings on the longest path to an element:

  a bilinear pixel     7   (1 - fx, 1 - fy, their product, the tap's product,
                            three additions); the footprint value of the
                            scatter, (1-fy)((1-fx) v + fx v') + fy (...), has
                            no longer a path
  a probe value        0 shared or unique, 1 with a weight, 1 + 2 C with C
                       eigen probes (a product and an addition each)
  a complex product    4 more (the moduli of both components' errors together
                            stay below 4 roundings of |a| |b|)
  a sum                1 per term added, and 1 for the contents added to
  |O|^2                2 x 7 for the square of a rounded pixel, 3 for re^2 + im^2

  patches 7;  objproj kP + 4 + S;  m_probe_update 7 + 4 + N (+ 1);
  probe preconditioner 17 + N (+ 1);  scatter 7 + the number of footprints
  that reach the pixel (+ 1)

The bound of an element is the larger of k 2^-24 (abs_terms + |contents|) and
MARGIN = 4 x the error of the float32 restatement: the same functions run with
dt = float32, products and sums in float32 and in index order (the margin,
because atomics and wave reductions add in another order).  An element whose
abs_terms is 0 must be exactly 0, or exactly its previous contents: footprint
column x' = pw at a whole-pixel position, every object pixel no footprint
reaches.  Errors of complex elements are moduli.

`mut` names a mutant of the model (MUTANTS): tests/test_overlap_sums_cpu.py
shows that each leaves the bound somewhere on the table."""
import collections
import functools

import numpy as np

F4, F8, C8, C16 = np.float32, np.float64, np.complex64, np.complex128
U = 2.0**-24
MARGIN = 4.0
MAX_MODES = 16    # TK_MAX_MODES of tike_lstsq_gradients / tike_probe_grad
CHUNK_MIN = 8     # probe_chunk: at least 8 positions per chunk, 32 chunks
GROUP = 8         # TK_GROUP: consecutive positions summed in one box
GSPREAD = 112     # TK_GSPREAD: box width / height beyond one footprint
ERR_ARG = 1000001
TAPS = ((0, 0), (0, 1), (1, 0), (1, 1))
MUTANTS = ("w01_w10", "shift_column", "no_last_column", "no_last_row",
           "no_conj", "chunk_last", "eigen_on_Sm", "no_w0_rest", "H_W",
           "no_duplicate")

Sum = collections.namedtuple("Sum", "value abs_terms k")


def _ct(dt):
    return C16 if dt is F8 else C8


def corners(scan):
    """(integer corner (N, 2), fraction (N, 2) float32), in float32."""
    s = np.asarray(scan, F4).reshape(-1, 2)
    fl = np.floor(s)
    return fl.astype(np.int64), (s - fl).astype(F4)


def weights_of(frac, dt=F8, mut=None):
    """(N, 4): w00, w01, w10, w11 in the arithmetic of `dt`."""
    fy, fx = np.asarray(frac, F4).astype(dt).T
    one = dt(1)
    w = np.stack([(one - fx) * (one - fy), fx * (one - fy), (one - fx) * fy,
                  fx * fy], axis=-1)
    return w[:, [0, 2, 1, 3]] if mut == "w01_w10" else w


def chunk_of(nscan):
    """Positions per chunk of the sums over positions (probe_chunk)."""
    return max(CHUNK_MIN, (nscan + 31) // 32)


def num_chunks(nscan):
    c = chunk_of(nscan)
    return (nscan + c - 1) // c


def dropped(scan, mut):
    """(N,) bool: the positions a mutant leaves out of the sums over n."""
    scan = np.asarray(scan, F4).reshape(-1, 2)
    skip = np.zeros(len(scan), bool)
    if mut == "chunk_last":
        skip[min(len(scan), chunk_of(len(scan))) - 1] = True
    elif mut == "no_duplicate":
        for n in range(1, len(scan)):
            skip[n] = bool(np.any(np.all(scan[:n] == scan[n], axis=1)))
    return skip


# ------------------------------------------------------------------- gather
def patches_of(psi, scan, pw, dt=F8, mut=None):
    """Sum of (N, pw, pw): the bilinear patches with the weights of tk_corner."""
    psi = np.asarray(psi, _ct(dt))
    H, W = psi.shape
    stride = H if mut == "H_W" else W
    flat = psi.ravel()
    corner, frac = corners(scan)
    w = weights_of(frac, dt, mut)
    yy, xx = np.arange(pw)[:, None], np.arange(pw)[None, :]
    shift = 1 if mut == "shift_column" else 0
    out = np.zeros((len(corner), pw, pw), _ct(dt))
    mag = np.zeros((len(corner), pw, pw), dt)
    for n, (sy, sx) in enumerate(corner):
        for k, (dy, dx) in enumerate(TAPS):
            idx = (sy + dy + yy) * stride + (sx + shift + dx + xx)
            tap = flat[np.clip(idx, 0, flat.size - 1)]  # (clipped: mutants only)
            out[n] += w[n, k] * tap
            mag[n] += w[n, k] * np.abs(tap)
    return Sum(out, mag, 7)


def probe_of_positions(form, nscan, probe, weights=None, eigen=None,
                       unique=None, dt=F8, mut=None):
    """Sum of (nscan, S, pw, pw): the probe of every position (k: roundings
    of the longest path, that of a mode with every eigen probe)."""
    ct = _ct(dt)
    probe = np.asarray(probe, ct)
    S = probe.shape[0]
    if form == "shared" or weights is None:
        P = np.broadcast_to(probe, (nscan, *probe.shape)).copy()
        return Sum(P, np.abs(P), 0)
    w = np.asarray(weights, F4).astype(dt)
    Sm = {"weights": 0, "eigen": None if eigen is None else eigen.shape[1],
          "unique": None if unique is None else unique.shape[1]}[form]
    w0 = w[:, 0, :].copy()
    if mut == "no_w0_rest":
        w0[:, Sm:] = 1
    P = (w0[:, :, None, None] * probe[None]).astype(ct)
    mag = np.abs(w0)[:, :, None, None] * np.abs(probe)[None]
    k = 1
    if form == "eigen":
        e = np.asarray(eigen, ct)
        C = e.shape[0]
        rows = e.reshape(C * Sm, *e.shape[2:])
        top = Sm + (1 if mut == "eigen_on_Sm" and Sm < S else 0)
        for c in range(C):
            for s in range(top):
                E = rows[(c * Sm + s) % (C * Sm)]  # (the kernel's addressing)
                wc = w[:, c + 1, s, None, None]
                P[:, s] += wc * E[None]
                mag[:, s] += np.abs(wc) * np.abs(E)[None]
        k = 1 + 2 * C
    elif form == "unique":
        u = np.asarray(unique, ct)
        P[:, :Sm], mag[:, :Sm] = u, np.abs(u)
    return Sum(P, mag, k)


def gradients(chi, scan, psi, probes, dt=F8, mut=None):
    """{patches, objproj, m_probe_update}, each a Sum; `probes` is the Sum of
    probe_of_positions.  m_probe_update is the sum alone: the entry adds it
    to what the buffer holds."""
    ct = _ct(dt)
    chi = np.asarray(chi, ct)
    N, S, pw = chi.shape[:3]
    achi = np.abs(chi)
    O = patches_of(psi, scan, pw, dt, mut)
    conj = (lambda a: a) if mut == "no_conj" else np.conj
    proj, pmag = np.zeros((N, pw, pw), ct), np.zeros((N, pw, pw), dt)
    for s in range(S):
        proj += conj(probes.value[:, s]) * chi[:, s]
        pmag += probes.abs_terms[:, s] * achi[:, s]
    mpu, mmag = np.zeros((S, pw, pw), ct), np.zeros((S, pw, pw), dt)
    skip = dropped(scan, mut)
    for n in range(N):
        if not skip[n]:
            mpu += conj(O.value[n])[None] * chi[n]
            mmag += O.abs_terms[n][None] * achi[n]
    return dict(patches=O, objproj=Sum(proj, pmag, probes.k + 4 + S),
                m_probe_update=Sum(mpu, mmag, 7 + 4 + N))


def probe_preconditioner(scan, psi, pw, dt=F8, mut=None):
    """Sum of (pw, pw) real: sum_n |O_n|^2."""
    O = patches_of(psi, scan, pw, dt, mut)
    out, mag = np.zeros((pw, pw), dt), np.zeros((pw, pw), dt)
    skip = dropped(scan, mut)
    for n in range(len(skip)):
        if not skip[n]:
            v = O.value[n]
            out += v.real * v.real + v.imag * v.imag
            mag += O.abs_terms[n] * O.abs_terms[n]
    return Sum(out, mag, 2 * 7 + 3 + len(skip))


# ------------------------------------------------------------------ scatter
def scatter(values, scan, H, W, dt=F8, mut=None):
    """Sum of (H, W): the footprint scatter-add of values (N, pw, pw), or of
    one patch (pw, pw) for every position; complex or real."""
    values = np.asarray(values)
    vt = _ct(dt) if np.iscomplexobj(values) else dt
    values = values.astype(vt)
    pw = values.shape[-1]
    corner, frac = corners(scan)
    w = weights_of(frac, dt, mut)
    stride = H if mut == "H_W" else W
    total = H * W
    out, mag, cnt = np.zeros(total, vt), np.zeros(total, dt), np.zeros(total, int)
    yy, xx = np.arange(pw)[:, None], np.arange(pw)[None, :]
    keep = np.ones((2, 2, pw, pw), bool)
    if mut == "no_last_column":
        keep[:, 1, :, pw - 1] = False
    if mut == "no_last_row":
        keep[1, :, pw - 1, :] = False
    skip = dropped(scan, mut)
    for n, (sy, sx) in enumerate(corner):
        if skip[n]:
            continue
        v = values[n] if values.ndim == 3 else values
        reach = np.zeros(total, bool)
        for k, (dy, dx) in enumerate(TAPS):
            Y, X = sy + dy + yy, sx + dx + xx
            idx = Y * stride + X
            ok = ((Y >= 0) & (Y < H) & (X >= 0) & (X < W) & (idx >= 0)
                  & (idx < total) & keep[dy, dx])
            out[idx[ok]] += (w[n, k] * v)[ok]
            mag[idx[ok]] += (w[n, k] * np.abs(v))[ok]
            reach[idx[ok]] = True
        cnt += reach
    return Sum(out.reshape(H, W), mag.reshape(H, W), 7 + cnt.reshape(H, W))


# ------------------------------------------------------------------- bounds
def bound(want, f32, prev=None):
    """(bound of every element, where the restatement term sets it): `want`
    and `f32` are the Sums of the model and of its float32 restatement, prev
    the contents the entry adds to."""
    mag = want.abs_terms + (0 if prev is None else np.abs(prev))
    base = (want.k + (prev is not None)) * U * mag
    wide = MARGIN * np.abs(np.asarray(f32.value, _ct(F8)) - want.value)
    return np.maximum(base, wide), wide > base


def restatement_ratio(want, f32):
    """The float32 restatement's error over k 2^-24 abs_terms (0 / 0 = 0)."""
    err = np.abs(np.asarray(f32.value, _ct(F8)) - want.value)
    base = want.k * U * want.abs_terms
    assert np.all(err[base == 0] == 0)
    return np.where(base > 0, err / np.where(base > 0, base, 1), 0.0)


def ratio(got, want, bnd, prev=None):
    """The worst error / bound of an output; elements without a term must
    hold 0 or their previous contents exactly (else: infinite)."""
    got = np.asarray(got)
    err = np.abs(got.astype(_ct(F8) if np.iscomplexobj(got) else F8)
                 - (want.value + (0 if prev is None else prev)))
    err = np.where(np.isnan(err), np.inf, err)
    still = want.abs_terms == 0
    exact = got == (0 if prev is None else np.asarray(prev).astype(got.dtype))
    with np.errstate(invalid="ignore", divide="ignore"):
        r = np.where(still, np.where(exact, 0.0, np.inf),
                     np.where(bnd > 0, err / np.where(bnd > 0, bnd, 1),
                              np.where(err == 0, 0.0, np.inf)))
    return float(np.max(r))


# ----------------------------------------------------------------- the cases
def rc(rng, *shape):
    """Complex normal values, exactly representable in complex64."""
    return (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)
            ).astype(C8)


def positions(rng, H, W, pw, nscan, specials_at=0, whole=False):
    """The position list of a case: a generic position, the smallest allowed
    (1, 1), the largest (H - pw - 1, W - pw - 1), a whole-pixel position,
    fractions just above 0 and just below 1, and the first one again -- from
    index `specials_at`, as many as nscan leaves room for -- among neighbours
    drawn from the 19 x 32 pixels next to (1, 1)."""
    ymax, xmax = H - pw - 1, W - pw - 1
    scan = np.stack([1 + rng.random(nscan) * min(ymax, 19),
                     1 + rng.random(nscan) * min(xmax, 32)], -1).astype(F4)
    y0, x0 = min(4, ymax - 1), min(6, xmax - 1)
    near = F4(2.0**-20)
    special = np.array([(y0 + 0.37, x0 + 0.61), (1, 1), (ymax, xmax),
                        (y0, x0 + 1), (y0 + near, x0 + 1 - near),
                        (y0 + 0.37, x0 + 0.61)], F4)
    m = max(0, min(len(special), nscan - specials_at))
    scan[specials_at:specials_at + m] = special[:m]
    if whole:
        scan = np.floor(scan)
    assert np.all(np.floor(scan) >= 1) and np.all(np.floor(scan) <= (ymax, xmax))
    return scan


def overhanging(rng, H, W, pw, nscan):
    """Positions over each of the four borders and over a corner (scatter
    only: the header says those pixels are dropped), then neighbours."""
    scan = positions(rng, H, W, pw, nscan)
    over = np.array([(-3.4, 5.2), (H - pw + 2.3, 4.7), (4.5, -2.6),
                     (5.1, W - pw + 3.7), (-1.5, -2.25)], F4)
    m = max(0, min(len(over), nscan - 6))  # behind the list's own six
    scan[6:6 + m] = over[:m]
    return scan


def boxed_groups(scan, nscan=None):
    """Per group of GROUP consecutive positions: whether the footprints'
    bounding box stays within pw + 1 + GSPREAD on both axes (summed on chip),
    else the group falls back to per-position atomics."""
    corner, _ = corners(scan)
    out = []
    for n0 in range(0, len(corner), GROUP):
        c = corner[n0:n0 + GROUP]
        out.append(bool(np.all(c.max(axis=0) - c.min(axis=0) <= GSPREAD)))
    return tuple(out)


# probe forms of the gather cases: (form, what is passed besides)
#   shared+   shared, with eigen probes and a unique probe passed but no weights
#   unique+   unique, with the eigen probes passed as well (they are not read)
Gather = collections.namedtuple("Gather", "name pw nscan S form C Sm outputs")
GATHER = [
    Gather("pw15-n1-S1-shared", 15, 1, 1, "shared", 0, 0, "all"),
    Gather("pw15-n8-S2-eigen22", 15, 8, 2, "eigen", 2, 2, "all"),
    Gather("pw17-n9-S3-eigen11", 17, 9, 3, "eigen", 1, 1, "all"),
    Gather("pw17-n70-S5-eigen25", 17, 70, 5, "eigen", 2, 5, "all"),
    Gather("pw40-n9-S6-unique2", 40, 9, 6, "unique", 0, 2, "all"),
    Gather("pw17-n9-S3-unique1+", 17, 9, 3, "unique+", 1, 1, "all"),
    Gather("pw40-n8-S8-weights", 40, 8, 8, "weights", 0, 0, "objproj"),
    Gather("pw17-n9-S7-weights", 17, 9, 7, "weights", 0, 0, "m_probe_update"),
    Gather("pw15-n70-S9-eigen29", 15, 70, 9, "eigen", 2, 9, "all"),
    Gather("pw15-n9-S16-shared", 15, 9, 16, "shared", 0, 0, "m_probe_update"),
    Gather("pw40-n70-S3-shared", 40, 70, 3, "shared", 0, 0, "all"),
    Gather("pw15-n9-S3-shared+", 15, 9, 3, "shared+", 1, 1, "objproj"),
    # S = 4, the compile-time count the list above leaves out, at a width the
    # row kernel of the probe preconditioner takes (256 % pw == 0)
    Gather("pw32-n9-S4-shared", 32, 9, 4, "shared", 0, 0, "all"),
]
OUTPUTS = {"all": ("patches", "m_probe_update", "objproj"),
           "objproj": ("objproj",), "m_probe_update": ("m_probe_update",)}

# layouts of the scatter cases: (H - pw, W - pw, first special position,
# whole, the groups' expected route).  With (1, 1) and the largest position in
# one group its box is W - pw - 2 (H - pw - 2) wider than a footprint.
Scatter = collections.namedtuple("Scatter", "name pw H W layout nscan boxed")
_LAYOUT = {
    "neighbours": (21, 34, 0), "whole": (21, 34, 0), "over": (21, 34, 0),
    "wide_in": (21, GSPREAD + 2, 0), "wide_out": (21, GSPREAD + 3, 0),
    "tall_in": (GSPREAD + 2, 34, 0), "tall_out": (GSPREAD + 3, 34, 0),
    "mixed": (21, GSPREAD + 3, 7),
}


def _scatter(pw, layout, nscan, boxed, H=None, W=None):
    dh, dw, _ = _LAYOUT[layout]
    H, W = H or pw + dh, W or pw + dw
    name = "pw{}-{}-n{}".format(pw, layout, nscan) + (
        "" if W == pw + dw else "-W{}".format(W))
    return Scatter(name, pw, H, W, layout, nscan, boxed)


SCATTER = [
    _scatter(7, "neighbours", 8, (True,)),
    _scatter(7, "neighbours", 9, (True, True), W=20),
    _scatter(7, "wide_out", 8, (False,)),
    _scatter(31, "neighbours", 1, (True,)),
    _scatter(31, "wide_in", 8, (True,)),
    _scatter(31, "wide_out", 8, (False,)),
    _scatter(32, "tall_out", 9, (False, True)),
    _scatter(32, "whole", 8, (True,)),
    _scatter(63, "neighbours", 13, (True, True)),
    _scatter(63, "wide_out", 9, (False, True)),
    _scatter(64, "tall_in", 8, (True,)),
    _scatter(64, "mixed", 13, (True, False)),
    _scatter(65, "wide_in", 13, (True, True)),
    _scatter(65, "wide_out", 13, (False, True)),
    _scatter(65, "over", 13, (True, True)),
    _scatter(65, "whole", 9, (True, True)),
    _scatter(130, "neighbours", 13, (True, True)),
    _scatter(130, "wide_out", 13, (False, True)),
]
# the reduced table of the deterministic forms (tests/_overlap_sums_child.py)
DET_GATHER = ("pw17-n9-S3-eigen11", "pw17-n70-S5-eigen25")
DET_SCATTER = ("pw31-wide_in-n8", "pw31-wide_out-n8", "pw65-wide_in-n13",
               "pw65-wide_out-n13")
SCATTER_ENTRIES = ("tike_scatter_patches", "tike_psi_preconditioner",
                   "tike_scatter_amplitudes")


def _seed(name):
    return int.from_bytes(name.encode(), "little") % (2**32)


@functools.lru_cache(maxsize=None)
def gather_inputs(name):
    """The float32 / complex64 arrays of a gather case, as the entries take
    them, and `call`: the form and arrays of probe_of_positions."""
    c = {g.name: g for g in GATHER}[name]
    rng = np.random.default_rng(_seed(name))
    H, W = c.pw + 21, c.pw + 34
    form = c.form.rstrip("+")
    I = dict(case=c, H=H, W=W, psi=rc(rng, H, W),
             scan=positions(rng, H, W, c.pw, c.nscan),
             chi=rc(rng, c.nscan, c.S, c.pw, c.pw),
             probe=rc(rng, c.S, c.pw, c.pw), eigen=None, weights=None,
             unique=None, mpu0=rc(rng, c.S, c.pw, c.pw),
             pre0=rc(rng, c.pw, c.pw))
    if form != "shared":
        I["weights"] = (1 + 0.3 * rng.standard_normal(
            (c.nscan, c.C + 1, c.S))).astype(F4)
    if form == "eigen" or c.form.endswith("+"):
        I["eigen"] = rc(rng, c.C, c.Sm, c.pw, c.pw)
    if form == "unique" or c.form == "shared+":
        I["unique"] = rc(rng, c.nscan, c.Sm, c.pw, c.pw)
    I["call"] = dict(form=form, nscan=c.nscan, probe=I["probe"],
                     weights=I["weights"],
                     eigen=I["eigen"] if form == "eigen" else None,
                     unique=I["unique"] if form == "unique" else None)
    for v in I.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return I


@functools.lru_cache(maxsize=None)
def gather_reference(name, mut=None, dt=F8):
    """{patches, objproj, m_probe_update, probe_preconditioner}: Sums."""
    I = gather_inputs(name)
    c = I["case"]
    P = probe_of_positions(dt=dt, mut=mut, **I["call"])
    R = gradients(I["chi"], I["scan"], I["psi"], P, dt, mut)
    R["probe_preconditioner"] = probe_preconditioner(I["scan"], I["psi"],
                                                     c.pw, dt, mut)
    return R


@functools.lru_cache(maxsize=None)
def scatter_inputs(name):
    c = {s.name: s for s in SCATTER}[name]
    rng = np.random.default_rng(_seed(name))
    if c.layout == "over":
        scan = overhanging(rng, c.H, c.W, c.pw, c.nscan)
    else:
        scan = positions(rng, c.H, c.W, c.pw, c.nscan,
                         _LAYOUT[c.layout][2], c.layout == "whole")
    I = dict(case=c, scan=scan, proj=rc(rng, c.nscan, c.pw, c.pw),
             amp=np.abs(rc(rng, c.pw, c.pw)).astype(F4),
             amps=rng.standard_normal((c.nscan, c.pw, c.pw)).astype(F4),
             acc0=rc(rng, c.H, c.W),
             out0=rng.standard_normal((c.H, c.W)).astype(F4))
    for v in I.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return I


def scatter_values(I, entry):
    """(the values an entry scatters, the contents it adds to)."""
    return {"tike_scatter_patches": (I["proj"], I["acc0"]),
            "tike_psi_preconditioner": (I["amp"], I["out0"]),
            "tike_scatter_amplitudes": (I["amps"], I["out0"])}[entry]


@functools.lru_cache(maxsize=None)
def scatter_reference(name, entry, mut=None, dt=F8):
    I = scatter_inputs(name)
    c = I["case"]
    return scatter(scatter_values(I, entry)[0], I["scan"], c.H, c.W, dt, mut)


def gather_bound(name, key, prev=None):
    return bound(gather_reference(name)[key],
                 gather_reference(name, None, F4)[key], prev)


def scatter_bound(name, entry):
    I = scatter_inputs(name)
    return bound(scatter_reference(name, entry),
                 scatter_reference(name, entry, None, F4),
                 scatter_values(I, entry)[1])
