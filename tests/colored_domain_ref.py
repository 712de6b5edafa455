"""Inputs and statements of the colored GICP factor-domain sweep (tests/test_colored_domain_gpu.py, tests/test_colored_domain_ref_cpu.py).  A helper, not a test.

The scene, the placements and the poses are tests/factor_domain_ref.py's (scan_to_map / both_far / scaled, with its face-margin filter and DROP_CAP); the f64
statements are tests/colored_ref.py's.  Target normals and both sides' covariances are the scene's own (move, plane_covs): no estimator is involved.

Intensities.  field() is colored_ref.two_plane_cloud's field with its arguments divided by FIELD_LENGTH and the whole multiplied by FIELD_AMPLITUDE, evaluated on
the scene's sensor-frame f64 coordinates BEFORE placement and scaling, so every placement of the scene carries the same intensities; the source's are the field
at the source point plus N(0, 0.01).  intensity_scale (1, 255, 65535) multiplies both sides before the rounding to f32.  The amplitude is what puts the photometric
term's share of the reference's error at weight 0.25 into [0.05, 0.95] at every placement (tests/test_colored_domain_ref_cpu.py; measured there: see FIELD_AMPLITUDE).

Gradients far from the origin.  The reference (and the kernel) form a row as a = (t - along n) - p.  At |p| = 10 km each component of `a` is a difference of two
numbers of size 1e4: t - along n is rounded to ulp64(|p|), the subtraction of p is then exact, so `a` carries an ABSOLUTE error of about 2^-53 |p|, that is a
relative one of 2^-53 |p| / |a|.  The rows enter H = n n^T + sum a a^T and e = sum a (I_j - I) linearly and quadratically, the largest row (rho = max_j |a_j|_2)
setting the size of both, so two f64 evaluations that round that difference differently (another order, a fused multiply-add) differ in g = H^-1 e by
cond(H) 2^-52 |g| times |p| / rho instead of times 1:
    gradient_bound_far = 2^-23 |g|_inf + GRADIENT_C cond(H) 2^-52 |g|_inf max(1, |p|_inf / rho)
A derivation, not a measurement: tests/test_colored_domain_ref_cpu.py holds the f64 reference to a QUARTER of it against the same statement in long double at
every placement of the gradient sweep, and colored_ref.reorder_ratio (the rule by which GRADIENT_C was chosen) to GRADIENT_C / 4 on the same inputs.

At the origin of a 23 m scene |p| / rho is already 10 .. 60, so the second term is that much larger than colored_ref.gradient_bound's; it stays below 1e-10 |g|
there and the two bounds agree to that.

Measured on the CPU (tests/test_colored_domain_ref_cpu.py -s; the host's exact neighbour tables, where k = 32 with k_photo = 10 reads the same ten slots as k = 10):
  largest |g_f64 - g_longdouble|_inf / gradient_bound_far over a placement's points (held to 0.25), 0.4 rad | pi - 1e-3: 3.3e-7 | 4.7e-7 at 0 m, 8.9e-6 | 1.8e-6
  at 100 m, 6.9e-5 | 1.2e-5 at 1000 m, 2.1e-4 | 7.7e-4 at 10 km; both far 6.9e-5; units of 0.01 / 1 / 100 m: 3.5e-5 / 1.1e-7 / 2.0e-3; intensities x 255 and
  x 65535: 3.3e-7 .. 3.6e-7 at 0 m, 2.1e-4 .. 7.7e-4 at 10 km; strips at the origin 4.4e-6 / 1.5e-4 / 2.3e-3 at cond(H) 1e4 / 1e6 / 2.5e7, at 10 km 6.0e-7 / 5.8e-8.
  largest reorder ratio (held to GRADIENT_C / 4 = 4): 2.2 .. 2.9 at every placement but (10 km, pi - 1e-3), where it is 3.88; 0.05 and 0.25 in units of 0.01 and
  100 m; at most 0.48 in the strips.

strip_scene(): 257 isolated clusters 5 m apart along x.  A cluster is a centre point and 9 neighbours in the plane x = const (the normal is (1, 0, 0)), at m_j v
along a grid vector v of that plane (m = -8 .. 8 without 0, 60 <= |v| / 2^-10 <= 62.5, so L = 8 |v| = 0.47 .. 0.49 m: "0.5 m") plus w c_j across it with
sum c_j^2 = 1 / 0.25 and sum m_j c_j = 0: H has the eigenvalues 1 (the normal row), |v|^2 sum m_j^2 = 0.83 .. 0.90 and 4 w^2, so with w = 0.5 / sqrt(cond_target)
cond(H) = cond_target = (0.5 / w)^2.  The centre and the offsets along v lie on the 2^-10 m grid f32 holds exactly at |x| < 8192; the small offset across lies in
the y-z plane where the origin placement resolves 6e-8 m.  Translated by 10 km along factor_domain_ref.DIRECTION (6000, -6400, 4800: integers) that offset meets
the 2^-11 m f32 grid, which is what realised() reports: 9.0e3 .. 1.05e4 for 1e4, 5.3e5 .. 1.0e6 for 1e6, and 1.8e16 and beyond for 2.5e7 (w = 1e-4 m: every
cluster collinear to rounding, none within COND_CAP -- STRIP_COMPARED).  Intensities are a linear field plus a quadratic term in the cluster's own coordinates
(the same at both placements).  Only a centre has all nine neighbours within RADIUS: searched with that cut-off every other point has a short list.
collinear_scene(): the same with w = 0 exactly in the plane z = const, normal (0, 0, 1), every coordinate and intensity a small multiple of 2^-10: every product
in H and in the cofactor inverse is exact in f64 (with or without fused multiply-adds), det H = 0 exactly and every component of the gradient has a 0 * inf in it:
NaN on any correct f64 evaluation."""
import numpy as np

import colored_ref
import factor_domain_ref as fd

PARITY_TOL = 1e-7  # tests/test_colored_gicp_gpu.py
GATE = 1e-5        # the north-star gate
MARGIN = 1e-9      # tests/test_colored_gicp_gpu.py's input condition
NEARBY = np.array([0.002, -0.001, 0.003, 0.01, 0.02, -0.01])
CUTOFFS = [1.0, 0.5]
WEIGHTS = [0.25, 1.0]
INTENSITY_SCALES = [1.0, 255.0, 65535.0]
CASES_A = [(t, r) for t in fd.DISTANCES for r in fd.ROTATIONS]
FIELD_LENGTH = 2.0
# The field's amplitude.  The placements are 0.1 .. 0.4 m out of alignment: that costs the geometric term d^T M_g d with M_g up to 500 along the normal, and the
# photometric term only (|grad I| x that distance)^2, so at an amplitude of 40 the photometric share of the error at weight 0.25 was 0.009 .. 0.014.  At 250 it is
# 0.352 / 0.336 at the cut-offs 1 / 0.5 of every scan-to-map placement and in every unit, 0.258 with both clouds far (tests/test_colored_domain_ref_cpu.py).
# Intensities then reach 650: "8 bit" is 1.7e5 and "16 bit" 4.3e7, where f32 resolves 4.
FIELD_AMPLITUDE = 250.0
INTENSITY_NOISE = 0.01
K_GRADIENTS = [(10, 10), (32, 10)]  # (k of the table, k_photo)


def tolerance(far):
    """what the GPU tests assert: the project's own tolerance at |t| = 0, in the controls and in other units; the gate further out"""
    return GATE if far else PARITY_TOL


def field(x):
    """colored_ref.two_plane_cloud's intensity field on x / FIELD_LENGTH, times FIELD_AMPLITUDE"""
    x = np.asarray(x, dtype=np.float64) / FIELD_LENGTH
    return FIELD_AMPLITUDE * (0.5 + 0.3 * np.sin(1.3 * x[:, 0] + 0.4 * x[:, 2]) * np.cos(0.9 * x[:, 1]) + 0.05 * x[:, 2] ** 2)


def placements():
    """every placement of the sweep: (name, maker in factor_domain_ref, its arguments, far)"""
    for t, r in CASES_A:
        yield f"a {t:g} m {r}", "scan_to_map", (t, r), t > 0
    yield "b both far", "both_far", (), False
    for s in fd.SCALES:
        yield f"c scale {s:g}", "scaled", (s,), False


def sweep():
    """every factor case of (F-a) .. (F-c): (name, maker, its arguments, cut-off in the case's units, photometric weight, far)"""
    for name, maker, args, far in placements():
        unit = args[0] if maker == "scaled" else 1.0
        for c in CUTOFFS if maker == "scan_to_map" else [1.0]:
            for w in WEIGHTS:
                yield f"{name} cutoff {c:g} weight {w:g}", maker, args, c * unit, w, far


# what tests/test_colored_domain_gpu.py runs beyond placements() x K_GRADIENTS and sweep(); tests/test_colored_domain_ref_cpu.py::test_case_list holds the lists
# to the items of the sweep
HIGH_RANGE = [(s, t, r) for s in INTENSITY_SCALES[1:] for t, r in ((0.0, "0.4rad"), (10000.0, "pi-1e-3"))]  # (F-h); (G2) takes its scales and distances
STRIP_CONDS = [1e4, 1e6, 1e8 / 4]
STRIP_CASES = [(c, far) for c in STRIP_CONDS for far in (False, True)]
# the centres whose realised cond(H) is within COND_CAP (tests/test_colored_domain_ref_cpu.py::test_strip_scene): at 10 km the 2^-11 m f32 grid swallows the
# 1e-4 m offsets of the last target and no centre is left to compare
STRIP_COMPARED = {(c, far): 0 if (far and c == STRIP_CONDS[-1]) else 257 for c, far in STRIP_CASES}
GENERAL_WEIGHTS = [0.0, 0.25, 1.0]  # (F-e)
HASHED_CASES = [(10000.0, r) for r in fd.ROTATIONS]  # (F-s)
FAR = 10000.0

_CASES = {}


def _same_points(kept, d, key):
    assert kept.shape == d[key].shape and np.array_equal(kept, d[key]), f"{key}: the face-margin filter is not the one factor_domain_ref applied"


def case(maker, args, intensity_scale=1.0):
    """(inputs with target_intensities / source_intensities f32, delta, nearby pose, dropped share, unit of length) of one placement, made once and shared (never
    written to).  The filters of factor_domain_ref are applied to the intensities by recomputing their masks, which is asserted on the points."""
    key = (maker,) + tuple(args) + (float(intensity_scale),)
    if key not in _CASES:
        d, delta, _, dropped = getattr(fd, maker)(*args)
        assert dropped <= fd.DROP_CAP
        unit = args[0] if maker == "scaled" else 1.0
        s = fd.scene()
        W = np.eye(4) if maker == "scaled" else d["W"]
        tp = fd.move(s["target_points"], s["target_normals"], s["target_covs"], W, unit)[0]
        tkeep = fd.face_margins(tp, np.eye(4), d["leaf"]) > fd.MARGIN
        _same_points(tp[tkeep], d, "target_points")
        sp = fd.move(s["source_points"], s["source_normals"], s["source_covs"], W if maker == "both_far" else np.eye(4), unit)[0]
        skeep = fd.face_margins(sp, delta, d["leaf"]) > fd.MARGIN
        _same_points(sp[skeep], d, "source_points")
        noise = np.random.default_rng(fd.SEED + 1).normal(0.0, INTENSITY_NOISE, len(sp))
        d = dict(d)
        d["target_intensities"] = (float(intensity_scale) * field(s["target_points"]))[tkeep].astype(np.float32)
        d["source_intensities"] = (float(intensity_scale) * (field(s["source_points"]) + noise))[skeep].astype(np.float32)
        step = fd.expmap(NEARBY)
        step[:3, 3] *= unit
        _CASES[key] = (d, delta, delta @ step, dropped, unit)
    return _CASES[key]


def with_margin(d, delta):
    """factor_domain_ref.with_margin on inputs that carry intensities -> (inputs, dropped share)"""
    out, dropped = fd.with_margin(d, delta)
    keep = fd.face_margins(d["source_points"], delta, d["leaf"]) > fd.MARGIN
    _same_points(d["source_points"][keep], out, "source_points")
    out["source_intensities"] = d["source_intensities"][keep]
    return out, dropped


def make_ref(d, gradients, cutoff, weight):
    return colored_ref.ColoredGICPFactorRef(d["target_points"], d["target_covs"], d["target_normals"], d["target_intensities"], gradients, d["source_points"],
                                            d["source_covs"], d["source_intensities"], max_correspondence_distance=cutoff, photometric_term_weight=weight)


def conditioned(ref, delta, what):
    """test_colored_gicp_gpu._conditioned: tie and cut-off margins > MARGIN (relative, squared distances) -> the two smallest margins"""
    tie, cut = ref.margins(delta)
    low = (float(tie.min()), float(cut.min()))
    print(f"[colored domain] {what}: smallest tie gap {low[0]:.3e}, smallest cut-off gap {low[1]:.3e}")
    assert low[0] > MARGIN and low[1] > MARGIN, f"{what}: a correspondence two f64 implementations could decide differently (tie {low[0]:.2e}, cut-off {low[1]:.2e})"
    return low


def photometric_share(ref, delta):
    """the share of sum w_p r_p^2 in the reference's error at `delta` (on the correspondences stored, searched at `delta` if there are none)"""
    _, _, _, _, _, rp, _ = ref._terms(delta)
    total = ref.evaluate(delta, derivatives=False)["error"]
    return float(ref.photometric_term_weight * (rp * rp).sum() / total) if total else 0.0


def gradient_bound_far(g_ref, cond, p, rho):
    """per point: 2^-23 |g|_inf + GRADIENT_C cond(H) 2^-52 |g|_inf max(1, |p|_inf / rho) (the module docstring); inf where cond(H) is"""
    a = np.abs(np.asarray(g_ref, dtype=np.float64)).max(axis=1)
    p = np.abs(np.asarray(p, dtype=np.float32).reshape(-1, 3).astype(np.float64)).max(axis=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        amp = np.maximum(1.0, p / rho)
        return 2.0**-23 * a + colored_ref.GRADIENT_C * cond * 2.0**-52 * a * amp


def gradient_reference(points, normals, intensities, table, k_photo, dtype=np.float64):
    """(g (N,3) in `dtype`, cond(H) (N,), rho (N,): 0 where the list is short) -- what a gradient comparison needs"""
    g, cond = colored_ref.intensity_gradients(points, normals, intensities, table, k_photo, dtype=dtype)
    rows, _, _, r = colored_ref.gradient_systems(points, normals, intensities, table, k_photo)
    rho = np.zeros(len(g))
    rho[rows] = r
    return g, cond, rho


# ---- near-degenerate neighbourhoods -----------------------------------------------------------------------------------------------------------------------------------
CLUSTERS = 257  # a workgroup plus one lane
SPACING = 5.0
GRID = 2.0**-10
LENGTH = 0.5
RADIUS = 0.52   # a search cut-off between the centre's furthest neighbour (8 |v| <= 0.49 m) and every other point's (9 |v| >= 0.527 m)
K_CLUSTER = 10
_M = np.array([-8, -6, -4, -2, 1, 2, 4, 6, 8])  # the neighbours stand at m_j v, v on the grid with 60 <= |v| / 2^-10 <= 62.5: L = 8 |v| = 0.47 .. 0.49 m
_C = np.array([1.0, -1.0, -1.0, 1.0, 0.0, 1.0, -1.0, -1.0, 1.0]) / np.sqrt(8.0) / LENGTH  # sum c^2 = 1 / L^2, sum m c = 0
_V = np.array([(36, 48), (48, 36), (40, 46), (44, 42), (50, 34), (56, 24), (30, 53), (60, 10), (20, 58), (62, 8)])


def _clusters(rng, normal_axis):
    """(centres (n,3) on the grid, v (n,3) on the grid in the plane across `normal_axis`, e2 (n,3): the unit vector across v in that plane)"""
    n = CLUSTERS
    base = np.stack([SPACING * np.arange(n), rng.integers(-300, 300, n) * GRID, rng.integers(-300, 300, n) * GRID], 1)
    uv = _V[rng.integers(0, len(_V), n)] * rng.choice([-1, 1], (n, 2))
    first, second = [a for a in range(3) if a != normal_axis]
    v, e2 = np.zeros((n, 3)), np.zeros((n, 3))
    v[:, first], v[:, second] = uv[:, 0] * GRID, uv[:, 1] * GRID
    e2[:, first], e2[:, second] = -v[:, second], v[:, first]
    return base, v, e2 / np.linalg.norm(e2, axis=1)[:, None]


def _assemble(rng, base, local, intensities, normal_axis, shift):
    pts = (base[:, None, :] + local).reshape(-1, 3)
    order = rng.permutation(len(pts))  # (a cluster's points are not consecutive in the cloud)
    where = np.empty(len(pts), dtype=np.int64)
    where[order] = np.arange(len(pts))
    normal = np.zeros(3, dtype=np.float32)
    normal[normal_axis] = 1.0
    return dict(points=(pts[order] + shift).astype(np.float32), normals=np.tile(normal, (len(pts), 1)), intensities=intensities.reshape(-1)[order].astype(np.float32),
                centres=where[np.arange(CLUSTERS) * K_CLUSTER], exact_points=pts[order], exact_intensities=intensities.reshape(-1)[order])


def strip_scene(cond_target, far, seed=91):
    """-> dict(points f32 (2570,3), normals f32, intensities f32, centres (257,) indices): cond(H) of a centre about cond_target; far: translated by 10 km along
    fd.DIRECTION"""
    rng = np.random.default_rng(seed)
    base, v, e2 = _clusters(rng, 0)
    w = LENGTH / np.sqrt(cond_target)
    local = np.concatenate([np.zeros((CLUSTERS, 1, 3)), _M[None, :, None] * v[:, None, :] + w * _C[None, :, None] * e2[:, None, :]], axis=1)  # (n, 10, 3)
    slope = rng.uniform(0.3, 1.0, (CLUSTERS, 3)) * rng.choice([-1.0, 1.0], (CLUSTERS, 3))
    along = (local * v[:, None, :]).sum(axis=2) / np.linalg.norm(v, axis=1)[:, None]
    intensities = 0.5 + (local * slope[:, None, :]).sum(axis=2) + 0.8 * along**2
    return _assemble(rng, base, local, intensities, 0, FAR * fd.DIRECTION if far else np.zeros(3))


def collinear_scene(seed=92):
    """the clusters with w = 0 exactly in the plane z = const, normal (0, 0, 1), intensities multiples of 2^-10: a_j = m_j v, so H, its cofactors and det H = 0
    are exact in f64 -> the same dict as strip_scene"""
    rng = np.random.default_rng(seed)
    base, v, _ = _clusters(rng, 2)
    local = np.concatenate([np.zeros((CLUSTERS, 1, 3)), _M[None, :, None] * v[:, None, :]], axis=1)
    intensities = 0.5 + GRID * np.concatenate([np.zeros((CLUSTERS, 1)), rng.integers(-200, 200, (CLUSTERS, len(_M)))], axis=1)
    out = _assemble(rng, base, local, intensities, 2, np.zeros(3))
    assert np.array_equal(out["points"].astype(np.float64), out["exact_points"]) and np.array_equal(out["intensities"].astype(np.float64), out["exact_intensities"])
    return out


def realised(scene, table):
    """what the f32 inputs realise over the centres: (smallest, largest) cond(H), inf for a centre whose neighbours the f32 grid made collinear"""
    _, cond = colored_ref.intensity_gradients(scene["points"], scene["normals"], scene["intensities"], table)
    c = cond[scene["centres"]]
    return float(c.min()), float(c.max())


def host_table(points, k, radius=None):
    """the exact (N, k) neighbour table of tests/knn_ref.py with the point itself in slot 0; radius: -1 beyond it"""
    import knn_ref

    d2, idx = knn_ref.neighbours(points, points, k - 1)
    idx = np.array(idx, dtype=np.int64)
    if radius is not None:
        idx[d2 > radius * radius] = -1
    return idx
