"""Edge tests of the code around the voxel map against tests/cloud_ref.py (numpy f64 on the f32 inputs): lookup_kernel (gp_voxelmap_lookup / gp_voxelmap_overlap),
overlap_jobs_kernel (gp_voxelmap_overlap_multi / _batch), transform_frames_kernel (gp_transform_frames) and gp_merge_frames -- at lane (64), workgroup / tile (256)
and multi-tile sizes, on voxel faces, at and below zero, with non-finite points, empty sources and empty frames.

Every parity test asserts first that its input lies further than MARGIN (1e-9, relative) from a voxel face or from the surface-validation threshold
(tests/test_cloud_ref_cpu.py asserts the same without a GPU), unless the arithmetic is exact.  Each test prints its worst figure."""
import ctypes as C

import numpy as np
import pytest

import cloud_ref as cr
from helpers import expmap

pytestmark = pytest.mark.gpu

PAD = 64  # rows in front of and behind every output of gp_transform_frames
SENTINEL = -123456.0


def _pose(name):
    return np.eye(4) if name == "identity" else expmap(cr.XIS[name])


def _dev(a):
    """numpy float32 -> device tensor, or None for an empty array (an empty cloud has no device array)"""
    import torch

    a = np.ascontiguousarray(a, dtype=np.float32)
    return torch.from_numpy(a).to("cuda:0") if a.size else None


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _rows(t):
    return 0 if t is None else int(t.shape[0])


def _build_map(gpu, points, covs, res):
    cloud = gpu.PointCloudGPU(points, covs)
    vm = gpu.GaussianVoxelMapGPU(res, target_points_drop_rate=0.0)
    vm.insert(cloud)
    coords = vm.download_f64()[0]
    return vm, coords, cr.coord_index(coords), cloud


def _unit_covs(n):
    return np.tile(np.eye(3, dtype=np.float32).reshape(1, 9), (n, 1))


def _hits_single(gpu, vm, pts, T):
    hits = C.c_int(-1)
    gpu._capi.check(gpu.load().gp_voxelmap_overlap(vm._h, _p(pts), _rows(pts), gpu.types._pose16(T), C.byref(hits), None), "gp_voxelmap_overlap")
    return hits.value


def _hits_multi(gpu, vms, Ts, pts):
    handles = (C.c_void_p * len(vms))(*[vm._h.value for vm in vms])
    deltas = gpu.types._poses_flat(Ts) if vms else np.zeros((1, 16))
    hits = C.c_int(-1)
    gpu._capi.check(gpu.load().gp_voxelmap_overlap_multi(handles, deltas.ctypes.data, len(vms), _p(pts), _rows(pts), C.byref(hits), None), "gp_voxelmap_overlap_multi")
    return hits.value


def _hits_batch(gpu, vms, pts_list, Ts):
    K = len(vms)
    handles = (C.c_void_p * K)(*[vm._h.value for vm in vms])
    pts = (C.c_void_p * K)(*[(t.data_ptr() if t is not None else None) for t in pts_list])
    ns = (C.c_int * K)(*[_rows(t) for t in pts_list])
    hits = (C.c_int * K)(*([-1] * K))
    deltas = gpu.types._poses_flat(Ts)
    gpu._capi.check(gpu.load().gp_voxelmap_overlap_batch(handles, pts, ns, deltas.ctypes.data, K, hits, None), "gp_voxelmap_overlap_batch")
    return [hits[k] for k in range(K)]


class _World:
    """the kitti00 pair on the device, its maps per resolution and the restatement's lookups per (pose, resolution): built once, read by every test"""

    def __init__(self, gpu, kitti00):
        self.gpu = gpu
        self.tp, self.tc = kitti00["target_points"], kitti00["target_covs"]
        self.sp = kitti00["source_points"]
        self.normals = cr.unit_normals(len(self.sp))
        self.src = gpu.PointCloudGPU(self.sp, normals=self.normals)
        self._maps, self._want = {}, {}

    def map_at(self, res):
        if res not in self._maps:
            self._maps[res] = _build_map(self.gpu, self.tp, self.tc, res)
        return self._maps[res]

    def want(self, pose, res, surface=False):
        """cloud_ref.lookup of the whole source scan, after the margin assertions"""
        key = (pose, res, surface)
        if key not in self._want:
            T = _pose(pose)
            if pose != "identity":
                m = cr.face_margin(self.sp, T, res)
                assert m > cr.MARGIN, f"{pose} pose at {res} m: a coordinate lies {m:.2e} from a voxel face"
            if surface:
                s = cr.surface_margin(self.sp, self.normals, T)
                assert s > cr.MARGIN, f"{pose} pose: a cosine lies {s:.2e} from the threshold"
            self._want[key] = cr.lookup(self.map_at(res)[2], self.sp, T, res, self.normals if surface else None)
        return self._want[key]

    def view(self, start, n):
        """n points of the scan from `start`, as a view into the device array (or None for n = 0)"""
        return self.src.points_gpu[start : start + n] if n else None


@pytest.fixture(scope="module")
def world(gpu, kitti00):
    return _World(gpu, kitti00)


@pytest.fixture(scope="module")
def lattice_maps(gpu):
    """maps at leaf 0.5 of the whole exact lattice and of its y < 0 half"""
    pts = cr.lattice()
    half = cr.lattice_half(pts)
    return pts, _build_map(gpu, pts, _unit_covs(len(pts)), 0.5), _build_map(gpu, half, _unit_covs(len(half)), 0.5)


# ---- lookup ----------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("res", [0.5, 0.3])
@pytest.mark.parametrize("pose", ["identity", "small", "large"])
def test_lookup_names_the_voxel(world, pose, res):
    """vm.lookup(src, T) equals the restatement for every point, index for index: the whole scan, slices of 1 .. 513 points at odd offsets, and no point at all"""
    gpu = world.gpu
    vm, coords, _, _ = world.map_at(res)
    T = _pose(pose)
    want = world.want(pose, res)
    got = vm.lookup(world.src, T)
    assert got.dtype == np.int32 and got.shape == want.shape
    wrong = int((got != want).sum())
    print(f"lookup {pose} {res} m: {len(want)} points, {int((want >= 0).sum())} hits, {wrong} differ from the restatement")
    np.testing.assert_array_equal(got, want)
    assert (want >= 0).sum() > 100 and (want < 0).sum() > 100  # both outcomes occur
    q = cr.transform_points(T, world.sp)
    np.testing.assert_array_equal(coords[got[got >= 0]], np.floor(q[got >= 0] * (1.0 / res)).astype(np.int64))
    for n in cr.SIZES:
        start = 1000 + 3 * n
        part = vm.lookup(gpu.PointCloudGPU.from_device(world.view(start, n)), T)
        np.testing.assert_array_equal(part, want[start : start + n], err_msg=f"slice of {n} points")
    # n = 0: an empty array (an empty cloud has no device array: the pointers are null), and no hit in any overlap form
    empty = gpu.PointCloudGPU(np.zeros((0, 3), np.float32))
    got0 = vm.lookup(empty, T)
    assert empty.size() == 0 and got0.shape == (0,) and got0.dtype == np.int32
    assert _hits_single(gpu, vm, None, T) == 0 and gpu.overlap_gpu(vm, empty, T) == 0.0 and gpu.overlap_gpu([vm], empty, [T]) == 0.0


def test_faces_and_signs_in_exact_arithmetic(gpu, lattice_maps):
    """leaf 0.5, points on the lattice k * 0.25 (half of the coordinates on a voxel face), -0.0 and the smallest negative f32 normal: every product and sum is exact,
    so the voxel is the floor's, with no margin to assert.  Identity, then a 90 degree axis permutation with a translation by whole cells."""
    pts, (vm, coords, index, _), (hvm, hcoords, hindex, _) = lattice_maps
    src = gpu.PointCloudGPU(pts)
    got = vm.lookup(src, np.eye(4))
    assert (got >= 0).all(), f"{int((got < 0).sum())} lattice points are not found in the map built from them"
    np.testing.assert_array_equal(coords[got], np.floor(pts.astype(np.float64) / 0.5).astype(np.int64))
    np.testing.assert_array_equal(got, cr.lookup(index, pts, np.eye(4), 0.5))
    n0 = 17**3
    assert (coords[got[n0 : n0 + 289], 0] == 0).all() and (coords[got[n0 + 289 :], 0] == -1).all()  # -0.0 -> cell 0, -tiny -> cell -1
    assert _hits_single(gpu, vm, src.points_gpu, np.eye(4)) == len(pts)
    worst = 0
    for T in (np.eye(4), cr.PERM_POSE):
        for m, idx in ((vm, index), (hvm, hindex)):
            want = cr.lookup(idx, pts, T, 0.5)
            got = m.lookup(src, T)
            worst = max(worst, int((got != want).sum()))
            np.testing.assert_array_equal(got, want)
            assert _hits_single(gpu, m, src.points_gpu, T) == int((want >= 0).sum())
            assert _hits_multi(gpu, [m], [T], src.points_gpu) == int((want >= 0).sum())
        assert (want >= 0).any() and (want < 0).any()  # the half map misses some
    print(f"exact lattice: {len(pts)} points, {worst} differ from the restatement")


def test_non_finite_points_have_no_voxel(gpu, lattice_maps):
    """the map holds voxel (0, 0, 0), which is where a NaN converts to: NaN, +inf, -inf in each coordinate, alone and combined, every case in turn at the indices
    0, 63, 64 and the last, all of them between 200 and 270 as well -- lookup gives -1 for exactly those, and no overlap form counts them"""
    pts, (vm, coords, index, _), (hvm, _, hindex, _) = lattice_maps
    assert (0, 0, 0) in index
    bad = cr.nonfinite_cases()
    n = 321
    special = [0, 63, 64, n - 1]
    for r in range(len(bad)):
        p = pts[1000 : 1000 + n].copy()
        where = special + [200 + 5 * i for i in range(len(bad))]
        p[special] = bad[[(r + k) % len(bad) for k in range(4)]]
        p[where[4:]] = bad
        src_t = _dev(p)
        for T in (np.eye(4), cr.PERM_POSE):
            want = cr.lookup(index, p, T, 0.5)
            assert (want[where] == -1).all()
            got = vm.lookup(gpu.PointCloudGPU.from_device(src_t), T)
            np.testing.assert_array_equal(got, want)
            if np.array_equal(T, np.eye(4)):
                assert ((got == -1) == np.isin(np.arange(n), where)).all()  # exactly those
            hits = int((want >= 0).sum())
            assert _hits_single(gpu, vm, src_t, T) == hits
            union = cr.overlap_hits([(hindex, 0.5, T), (index, 0.5, T)], p)
            assert _hits_multi(gpu, [hvm, vm], [T, T], src_t) == union == hits
            assert _hits_batch(gpu, [vm, hvm], [src_t, src_t], [T, T]) == [hits, cr.overlap_hits([(hindex, 0.5, T)], p)]
    print(f"non-finite points: {len(bad)} cases x {len(special)} positions, 0 found, 0 counted")


@pytest.mark.parametrize("pose", ["small", "large"])
def test_surface_validation_matches_the_restatement(world, pose):
    vm = world.map_at(0.5)[0]
    want = world.want(pose, 0.5, surface=True)
    plain = world.want(pose, 0.5)
    got = vm.lookup(world.src, _pose(pose), surface_validation=True)
    rejected = int(((plain >= 0) & (want < 0)).sum())
    print(f"surface validation {pose}: {rejected} of {int((plain >= 0).sum())} hits rejected, {int((got != want).sum())} differ from the restatement")
    np.testing.assert_array_equal(got, want)
    assert rejected > 100 and (want >= 0).sum() > 100  # the validation decides something, and not everything
    for n in (1, 65, 257):
        start = 2000 + n
        part = world.gpu.PointCloudGPU.from_device(world.view(start, n))
        part.normals_gpu = world.src.normals_gpu[start : start + n]
        np.testing.assert_array_equal(vm.lookup(part, _pose(pose), surface_validation=True), want[start : start + n])


def test_surface_validation_at_the_origin_and_without_normals(gpu, lattice_maps):
    """|q| = 0: the cosine is a NaN on the device and a zero in the reference, neither is > 0.174 -- the point is kept.  Validation asked of a frame without normals
    raises instead of being skipped."""
    _, (vm, coords, index, _), _ = lattice_maps
    p = np.float32([[0.0, 0.0, 0.0], [0.1, 0.2, 0.3], [1.1, 1.2, 1.3], [0.1, 0.2, -0.3]])
    nrm = np.tile(np.float32([0.0, 0.0, 1.0]), (len(p), 1))
    want = cr.lookup(index, p, np.eye(4), 0.5, nrm)
    assert want[0] == index[(0, 0, 0)] and want[1] == -1 and want[2] == -1 and want[3] >= 0
    got = vm.lookup(gpu.PointCloudGPU(p, normals=nrm), np.eye(4), surface_validation=True)
    np.testing.assert_array_equal(got, want)
    with pytest.raises(gpu.GPError):
        vm.lookup(gpu.PointCloudGPU(p), np.eye(4), surface_validation=True)
    np.testing.assert_array_equal(vm.lookup(gpu.PointCloudGPU(p), np.eye(4)), cr.lookup(index, p, np.eye(4), 0.5))
    print("surface validation: the origin is kept; a frame without normals raises")


# ---- overlap ---------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("res", [0.5, 0.3])
def test_single_overlap_counts_are_exact(world, res):
    gpu = world.gpu
    vm = world.map_at(res)[0]
    checked = 0
    for pose in ("small", "large"):
        want = world.want(pose, res)
        T = _pose(pose)
        assert _hits_single(gpu, vm, world.src.points_gpu, T) == int((want >= 0).sum())
        for n in cr.SIZES:
            for start in (0, 4000 + 7 * n):
                hits = int((want[start : start + n] >= 0).sum())
                assert _hits_single(gpu, vm, world.view(start, n), T) == hits, f"{n} points from {start}, {pose} pose"
                assert _hits_multi(gpu, [vm], [T], world.view(start, n)) == hits
                rate = gpu.overlap_gpu(vm, gpu.PointCloudGPU.from_device(world.view(start, n)), T)
                assert round(rate * n) == hits and abs(rate - hits / n) < 1e-15
                checked += 1
    print(f"single overlap at {res} m: {checked} (size, offset, pose) combinations, every count equal")


def test_union_overlap_counts_are_exact(world):
    """0 targets, 1 target, 5 targets at five poses and four resolutions, the same map twice, and a subset that only the LAST target holds"""
    gpu = world.gpu
    sp, src = world.sp, world.src.points_gpu
    assert _hits_multi(gpu, [], [], src) == 0
    assert gpu.overlap_gpu([], world.src, []) == 0.0
    vm5, _, idx5, _ = world.map_at(0.5)
    small, large = _pose("small"), _pose("large")
    one = int((world.want("small", 0.5) >= 0).sum())
    assert _hits_multi(gpu, [vm5], [small], src) == one == _hits_single(gpu, vm5, src, small)
    assert _hits_multi(gpu, [vm5, vm5], [small, small], src) == one  # the same map twice adds nothing
    both = cr.overlap_hits([(idx5, 0.5, small), (idx5, 0.5, large)], sp)
    assert _hits_multi(gpu, [vm5, vm5], [small, large], src) == both > one
    Ts = [expmap(xi) if np.any(xi) else np.eye(4) for xi in cr.UNION_XIS]
    for xi, T, res in zip(cr.UNION_XIS, Ts, cr.UNION_RES):
        assert not np.any(xi) or cr.face_margin(sp, T, res) > cr.MARGIN
    targets = [(world.map_at(res)[2], res, T) for res, T in zip(cr.UNION_RES, Ts)]
    masks = [cr.overlap_mask([t], sp) for t in targets]
    union = int(np.logical_or.reduce(masks).sum())
    assert union > max(int(m.sum()) for m in masks)  # no single target explains the union
    got = _hits_multi(gpu, [world.map_at(res)[0] for res in cr.UNION_RES], Ts, src)
    assert got == union
    assert round(gpu.overlap_gpu([world.map_at(res)[0] for res in cr.UNION_RES], world.src, Ts) * len(sp)) == union
    for n in (1, 64, 257):  # the union over slices too
        assert _hits_multi(gpu, [world.map_at(res)[0] for res in cr.UNION_RES], Ts, world.view(500, n)) == int(np.logical_or.reduce(masks)[500 : 500 + n].sum())
    # found only by the last target
    us, far = cr.union_source(sp)
    assert cr.face_margin(us, small, 0.5) > cr.MARGIN and cr.face_margin(us, large, 1.0) > cr.MARGIN
    fvm, _, fidx, _ = _build_map(gpu, us[far], _unit_covs(len(far)), 0.5)
    near = [(idx5, 0.5, small), (world.map_at(1.0)[2], 1.0, large)]
    near_mask = cr.overlap_mask(near, us)
    far_mask = cr.overlap_mask([(fidx, 0.5, np.eye(4))], us)
    assert not near_mask[far].any() and far_mask[far].all() and not far_mask[:400].any()
    us_t = _dev(us)
    near_vms = [vm5, world.map_at(1.0)[0]]
    assert _hits_multi(gpu, near_vms, [small, large], us_t) == int(near_mask.sum())
    assert _hits_multi(gpu, near_vms + [fvm], [small, large, np.eye(4)], us_t) == int(near_mask.sum()) + len(far)
    assert _hits_multi(gpu, [fvm] + near_vms, [np.eye(4), small, large], us_t) == int(near_mask.sum()) + len(far)
    print(f"union overlap: 5 targets {got} == {union}; {len(far)} points found by the last target alone")


def test_batch_overlap_counts_are_exact(world):
    """one call over seven pairs: sources of 257, 0, 1, 256, 0 and 513 points (the empty ones with a null pointer, between others), the first source in two pairs
    with different poses and maps; every count equals the single form's and the restatement's"""
    gpu = world.gpu
    srcs = cr.batch_sources(world.sp)
    dev = [_dev(s) for s in srcs]
    assert dev[1] is None and dev[4] is None
    vms, pts, Ts, want = [], [], [], []
    for k, pose, res in cr.BATCH_PAIRS:
        T = _pose(pose)
        if pose != "identity" and len(srcs[k]):
            assert cr.face_margin(srcs[k], T, res) > cr.MARGIN
        vms.append(world.map_at(res)[0])
        pts.append(dev[k])
        Ts.append(T)
        want.append(cr.overlap_hits([(world.map_at(res)[2], res, T)], srcs[k]) if len(srcs[k]) else 0)
    got = _hits_batch(gpu, vms, pts, Ts)
    print(f"batch overlap: sizes {[len(srcs[k]) for k, _, _ in cr.BATCH_PAIRS]}, hits {got}, restatement {want}")
    assert got == want
    assert want[0] != want[6] and want[2] == 1 and sum(want) > 100  # the shared source is counted under two poses; the single point is a hit
    for vm, t, T, h in zip(vms, pts, Ts, got):
        assert _hits_single(gpu, vm, t, T) == h
    clouds = [gpu.PointCloudGPU(srcs[k]) for k, _, _ in cr.BATCH_PAIRS]
    rates = gpu.overlap_gpu(vms, clouds, Ts)
    for (k, _, _), r, h in zip(cr.BATCH_PAIRS, rates, got):
        assert r == (h / len(srcs[k]) if len(srcs[k]) else 0.0)
    assert rates[1] == 0.0 and rates[4] == 0.0 and got[1] == 0 and got[4] == 0
    with pytest.raises(gpu.GPError):
        gpu.overlap_gpu(vms[:2], clouds[:3], Ts[:2])  # size mismatch (gaussian_voxelmap_gpu_funcs.cu:342-345)


# ---- gp_transform_frames ---------------------------------------------------------------------------------------------------------------------------------------------
def _transform_frames(gpu, poses, dev_frames, covs=True, ints=True):
    """gp_transform_frames into arrays that are PAD rows longer on each side than the total, filled with SENTINEL.
    dev_frames: [(points, covs, intensities)] of device tensors or None.  -> (points (N,3), covs (N,9) or None, intensities [N] or None), after the sentinel check"""
    import torch

    F = len(dev_frames)
    ns = [_rows(f[0]) for f in dev_frames]
    total = sum(ns)
    outs = {w: torch.full((total + 2 * PAD, w), SENTINEL, dtype=torch.float32, device="cuda:0") for w in (3, 9, 1)}
    arr = lambda k: (C.c_void_p * F)(*[(f[k].data_ptr() if f[k] is not None else None) for f in dev_frames])  # noqa: E731
    inner = lambda w, on: C.c_void_p(outs[w].data_ptr() + 4 * w * PAD) if on else None  # noqa: E731
    flat = gpu.types._poses_flat(poses)  # (kept alive across the call)
    torch.cuda.synchronize()
    gpu._capi.check(gpu.load().gp_transform_frames(flat.ctypes.data, arr(0), arr(1), arr(2), (C.c_int * F)(*ns), F, inner(3, True), inner(9, covs),
                                                   inner(1, ints), None), "gp_transform_frames")
    host = {w: o.cpu().numpy() for w, o in outs.items()}
    for w, h in host.items():
        assert (h[:PAD] == np.float32(SENTINEL)).all() and (h[PAD + total :] == np.float32(SENTINEL)).all(), f"a write outside the {total} rows of the width-{w} output"
    if not covs:
        assert (host[9] == np.float32(SENTINEL)).all()
    if not ints:
        assert (host[1] == np.float32(SENTINEL)).all()
    return host[3][PAD : PAD + total], host[9][PAD : PAD + total] if covs else None, host[1][PAD : PAD + total, 0] if ints else None


def _upload_frames(frames):
    return [(_dev(p), _dev(c), _dev(i) if i is not None else None) for p, c, i in frames]


def test_transform_frames_holds_its_bound_and_its_rows(gpu):
    """gp_transform_frames on frames of 0, 1, 255, 256, 257, 0, 513 and 0 points (the empty ones with null pointers): three rigid poses, one general 3x3 block, one
    translation of order 1e4; random NON-symmetric covariances (a transposed product or a row-major read shows); intensities for some frames.

    Bounds (cloud_ref.transform_bounds): both sides evaluate every sum of three terms left to right in f64.  A term of a point passes its product and at most three
    additions: four roundings, 2 * 4 = 8 for two evaluations, each 2^-53 of |R||p| + |t|.  A term R_ri C_ij R_cj of a covariance passes a product and at most two
    additions in R C and the same in (R C) R^T: six roundings, 2 * 6 = 12 for two evaluations (the issue's estimate was 16; a fused multiply-add only removes
    roundings), each 2^-53 of |R||C||R^T|.  The store rounds once to f32: half a spacing of float32 at max(|got|, |ref|).
    Row begin_i + j is frame i's point j (the points are random: no two rows could be confused); the PAD rows either side of every output keep their sentinel."""
    poses, frames = cr.transform_case(expmap)
    assert [len(f[0]) for f in frames] == cr.FRAME_SIZES
    dev = _upload_frames(frames)
    assert dev[0][0] is None and dev[5][1] is None and dev[3][2] is None and dev[2][2] is not None
    ref = cr.transform(poses, frames)
    gp, gc, gi = _transform_frames(gpu, poses, dev)
    bp, bc = cr.transform_bounds(ref, gp, gc)
    ep, ec = np.abs(gp.astype(np.float64) - ref["points"]), np.abs(gc.astype(np.float64) - ref["covs"])
    off = int((gp != ref["points"].astype(np.float32)).sum())
    print(f"gp_transform_frames: worst error / bound: points {float((ep / bp).max()):.3f}, covariances {float((ec / bc).max()):.3f}; "
          f"point components that differ from the f32-rounded restatement: {off} of {gp.size}")
    assert (ep <= bp).all(), f"point row {int(np.argmax((ep > bp).any(axis=1)))}"
    assert (ec <= bc).all(), f"covariance row {int(np.argmax((ec > bc).any(axis=1)))}"
    np.testing.assert_array_equal(gi.view(np.uint32), ref["intensities"].view(np.uint32))
    for (p, c, it), b, n in zip(frames, ref["begin"], cr.FRAME_SIZES):
        if it is None:
            assert (gi[b : b + n] == 0).all()
    # without the covariances, without the intensities: the rest is the same, bit for bit
    p2, c2, i2 = _transform_frames(gpu, poses, dev, covs=False)
    assert c2 is None and np.array_equal(p2.view(np.uint32), gp.view(np.uint32)) and np.array_equal(i2.view(np.uint32), gi.view(np.uint32))
    p3, c3, i3 = _transform_frames(gpu, poses, dev, ints=False)
    assert i3 is None and np.array_equal(p3.view(np.uint32), gp.view(np.uint32)) and np.array_equal(c3.view(np.uint32), gc.view(np.uint32))
    # nothing but empty frames: nothing is written
    _transform_frames(gpu, poses[:1], dev[:1])


# ---- gp_merge_frames -------------------------------------------------------------------------------------------------------------------------------------------------
def _merge(gpu, poses, frames, res):
    """gp_merge_frames on host frames [(points (n,3), covs (n,9) column-major, intensities or None)] against cloud_ref.merge of the device's own transformed arrays
    (which test_transform_frames_holds_its_bound_and_its_rows holds to their bound: a one-ulp difference in the transform cannot move a point across a face here).
    Same coordinate set, each once; exact counts; f64 means within 1e-7 max(res, 1) and f64 covariances within 1e-13 max(1, max|C|) -- the gates of
    test_voxel_statistics_match_cpu_map; intensity = max over the voxel.  The map keeps the symmetric part of a covariance (gp_voxelmap.hip), the restatement the
    matrix as given: the symmetric part of its mean is compared.  merge_frames_gpu returns the map's f32 arrays bit for bit, in the map's order.
    -> (coords, counts, restatement, worst mean error / gate, worst covariance error / gate)"""
    dev = _upload_frames(frames)
    F = len(frames)
    tp, tc, ti = _transform_frames(gpu, poses, dev)
    ref = cr.merge(tp, tc, ti, res)
    arr = lambda k: (C.c_void_p * F)(*[(f[k].data_ptr() if f[k] is not None else None) for f in dev])  # noqa: E731
    h = C.c_void_p()
    flat = gpu.types._poses_flat(poses)
    gpu._capi.check(gpu.load().gp_merge_frames(flat.ctypes.data, arr(0), arr(1), arr(2), (C.c_int * F)(*[len(f[0]) for f in frames]), F, float(res),
                                               0.0, None, C.byref(h)), "gp_merge_frames")
    vm = gpu.GaussianVoxelMapGPU(res, _handle=h)
    coords, counts, means, covs = vm.download_f64()
    order = {tuple(k): i for i, k in enumerate(ref["coords"].tolist())}
    assert len(coords) == len(ref["coords"]), f"{len(coords)} voxels, the restatement has {len(ref['coords'])}"
    idx = np.array([order[tuple(k)] for k in coords.tolist()])  # KeyError = a voxel the restatement does not have
    assert len(set(idx.tolist())) == len(coords)
    np.testing.assert_array_equal(counts, ref["counts"][idx])
    assert counts.sum() == len(tp)
    gate_m = 1e-7 * max(res, 1.0)
    gate_c = 1e-13 * max(1.0, float(np.abs(tc).max()))
    em = float(np.abs(means - ref["means"][idx]).max())
    want_c = cr.symmetric_part(ref["covs"])[idx].reshape(-1, 3, 3).transpose(0, 2, 1)
    ec = float(np.abs(covs - want_c).max())
    assert em < gate_m and ec < gate_c, f"means {em:.3e} (gate {gate_m:.1e}), covariances {ec:.3e} (gate {gate_c:.1e})"
    dl = vm.download()
    np.testing.assert_array_equal(dl["intensities"], ref["intensities"][idx])
    np.testing.assert_array_equal(dl["num_points"], counts)
    clouds = [gpu.PointCloudGPU.from_device(*f) if f[0] is not None else gpu.PointCloudGPU(np.zeros((0, 3), np.float32), np.zeros((0, 9), np.float32)) for f in dev]
    merged = gpu.merge_frames_gpu(poses, clouds, res, target_points_drop_rate=0.0)
    assert merged.size() == len(coords)
    assert np.array_equal(merged.points_gpu.cpu().numpy().view(np.uint32), dl["means"].view(np.uint32))
    assert np.array_equal(merged.download("covs").view(np.uint32), dl["covs"].view(np.uint32))
    assert np.array_equal(merged.intensities_gpu.cpu().numpy().reshape(-1).view(np.uint32), dl["intensities"].view(np.uint32))
    return coords, counts, ref, em / gate_m, ec / gate_c


def _kitti_frames(kitti07, sizes, with_intensities=(2, 4, 5)):
    rng = np.random.default_rng(17)
    poses, frames = [], []
    for i, n in enumerate(sizes):
        j = i % 5
        start = 100 * i
        it = rng.uniform(0.0, 255.0, n).astype(np.float32) if i in with_intensities else None
        frames.append((kitti07[f"points_{j}"][start : start + n], cr.covs9(kitti07[f"covs_{j}"][start : start + n]), it))
        poses.append(np.asarray(kitti07["poses"][j], dtype=np.float64))
    return poses, frames


@pytest.mark.parametrize("res", [0.2, 1.0])
def test_merge_frames_by_coordinate(gpu, kitti07, res):
    """frames of 0, 1, 255, 256, 257, 0, 513 and 0 kitti07 points under the scans' poses, intensities for some"""
    poses, frames = _kitti_frames(kitti07, cr.FRAME_SIZES)
    coords, counts, ref, rm, rc = _merge(gpu, poses, frames, res)
    print(f"gp_merge_frames at {res} m: {len(coords)} voxels of {counts.sum()} points, largest {counts.max()}; worst error / gate: means {rm:.3f}, covariances {rc:.3f}")
    assert 1 < len(coords) < counts.sum()
    assert (ref["intensities"] > 0).any() and (ref["intensities"] == 0).any()


def test_merge_frames_corner_cases(gpu, kitti07):
    """identical frames (counts multiply, means stay), every point in one voxel, one frame of one point, the exact lattice (counts in closed form), no point at all"""
    # the same frame three times under the identity
    p, c = kitti07["points_0"][:257], cr.covs9(kitti07["covs_0"][:257])
    eye = [np.eye(4)] * 3
    c1, n1, r1, _, _ = _merge(gpu, eye[:1], [(p, c, None)], 1.0)
    c3, n3, r3, rm, rc = _merge(gpu, eye, [(p, c, None)] * 3, 1.0)
    np.testing.assert_array_equal(r3["coords"], r1["coords"])
    np.testing.assert_array_equal(r3["counts"], 3 * r1["counts"])
    assert np.abs(r3["means"] - r1["means"]).max() < 1e-12
    o1 = {tuple(k): i for i, k in enumerate(c1.tolist())}
    np.testing.assert_array_equal(n3, 3 * n1[[o1[tuple(k)] for k in c3.tolist()]])
    worst = [rm, rc]
    # every point in one voxel, over two frames and more than one statistics batch
    rng = np.random.default_rng(23)
    one = [(rng.uniform(0.01, 0.49, size=(n, 3)).astype(np.float32), rng.normal(size=(n, 9)).astype(np.float32), rng.uniform(0, 9, n).astype(np.float32)) for n in (600, 257)]
    coords, counts, _, rm, rc = _merge(gpu, eye[:2], one, 0.5)
    assert coords.tolist() == [[0, 0, 0]] and counts.tolist() == [857]
    worst += [rm, rc]
    # one frame of one point (and an empty frame either side)
    pt = (np.float32([[-0.3, 7.9, 0.0]]), np.arange(9, dtype=np.float32).reshape(1, 9), np.float32([3.5]))
    nothing = (np.zeros((0, 3), np.float32), np.zeros((0, 9), np.float32), None)
    for frames, ps in (([pt], eye[:1]), ([nothing, pt, nothing], eye)):
        coords, counts, _, rm, rc = _merge(gpu, ps, frames, 0.5)
        assert coords.tolist() == [[-1, 15, 0]] and counts.tolist() == [1]
        worst += [rm, rc]
    # the lattice under the exact pose: 2^(axes not in the last cell) points per voxel
    grid = cr.lattice()[: 17**3]
    coords, counts, _, rm, rc = _merge(gpu, [cr.PERM_POSE], [(grid, _unit_covs(len(grid)), None)], 0.5)
    np.testing.assert_array_equal(counts, cr.lattice_counts(coords))
    assert len(coords) == 9**3
    worst += [rm, rc]
    print(f"gp_merge_frames corner cases: worst error / gate {max(worst):.3f}")
    # no point at all
    empty = gpu.PointCloudGPU(np.zeros((0, 3), np.float32), np.zeros((0, 9), np.float32))
    with pytest.raises(gpu.GPError):
        gpu.merge_frames_gpu([np.eye(4)], [empty], 0.5)
    h = C.c_void_p()
    flat = gpu.types._poses_flat([np.eye(4)])
    assert gpu.load().gp_merge_frames(flat.ctypes.data, (C.c_void_p * 1)(None), (C.c_void_p * 1)(None), (C.c_void_p * 1)(None), (C.c_int * 1)(0), 1, 0.5,
                                      0.0, None, C.byref(h)) != 0 and not h.value
