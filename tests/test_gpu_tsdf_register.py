"""GPU: the field at a point and the registration against it (csrc/tsdf_map.hip: dpm_tsdf_sample, dpm_tsdf_register;
deeppointmap_amd/tsdf.py: TsdfMap.sample, TsdfMap.register, TsdfTracker) against the numpy restatement
(tests/tsdf_register_restated.py, checked on the CPU by tests/test_tsdf_register_host.py).

  sample         byte for byte the float32 restatement read from the GPU's own export(): a ray map and a plane map, min_count 1
                 and 2, a general pose and a lattice of v/2 (f exactly 0 and 0.5: voxel centres, faces, corners), cells with 7
                 of 8 corners, a point outside the 21 bits, NaN rows, a map origin 1 km out, an empty table; capacities 0, 1, 63,
                 64, 65, 257 with the count below the capacity.
  sums           the 29 values on the kernel's own rows against the float64 restatement, per entry max(3 |r32 - r64|, floor),
                 unweighted and with kernel_scale 0.1, a gross outlier among the rows; 255, 256, 257 and 1100 rows in a capacity
                 of 1300; the row count exact; fitness, rmse and the one-iteration pose from the sums.
  known answers  three patches in the plane form: CONVERGED, fitness > 0.8, 1e-4 m / 1e-4 at the origin and 1e-3 m 1 km out; the
                 ray form within max(3 |r32 - r64|, 1e-4) of the float64 restatement on the GPU's exported field (nothing is
                 claimed against the truth); one patch: SINGULAR, bytes kept; max_dist > truncation: refused.
  workspace      no byte outside [workspace, workspace + dpm_tsdf_register_scratch_bytes(cap)) is written.
  determinism    the same bytes twice and after one replay of a captured graph; the table's export unchanged by sample and
                 register.
  tracker        the box room: every pose within 1 mm of the restatement's tracker, one host synchronisation a step, lost == 0,
                 the final translation error <= 2 x the float64 restatement's own (the factor covers fp32 fields and poses); a
                 frame registered against an empty region is counted in `lost` and leaves the export's bytes alone.
Every figure goes to test_logs/tsdf_register_errors.log.
"""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import icp_restated as I  # noqa: E402
import tsdf_register_restated as TR  # noqa: E402
import tsdf_restated as R  # noqa: E402
from test_tsdf_register_host import BOX_KW, FAR, box_tracker, log  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32 = np.float32
ZERO = (0.0, 0.0, 0.0)


def dev(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).to(DEV)


def buffer(xyz, cap=None, fill=np.nan):
    """(xyz (cap,3) on the GPU whose first len(xyz) rows are the given ones and the rest `fill`, count (1,) int32)"""
    xyz = np.asarray(xyz, F32).reshape(-1, 3)
    buf = np.full((len(xyz) if cap is None else cap, 3), fill, F32)
    buf[:len(xyz)] = xyz
    return dev(buf), torch.tensor([len(xyz)], dtype=torch.int32, device=DEV)


_MAPS = {}


def gpu_case(origin=ZERO, which=(0, 1, 2), distance="plane"):
    """the patches fused once on the GPU, with the sorted export; made once and never written again"""
    key = (tuple(origin), tuple(which), distance)
    if key not in _MAPS:
        from deeppointmap_amd.tsdf import TsdfMap
        c = TR.patches_case(origin, which)
        m = TsdfMap(c.voxel, max_voxels=1 << 15, origin=c.origin, device=DEV, distance=distance)
        m.integrate(dev(c.xyz), c.pose, normals=dev(c.normals) if distance == "plane" else None)
        c.map, c.exported, c.tau = m.check(), m.export(), m.truncation
        _MAPS[key] = c
    return _MAPS[key]


def field_of(c, min_count=1, dtype=F32):
    return R.field(c.exported, max(1, int(round(min_count * c.map.unit))), dtype)


def same(got, want, what):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    assert got.tobytes() == want.tobytes(), (what, int((got.view(np.int32) != want.view(np.int32)).sum()) if got.itemsize == 4 else None)


# ---------------------------------------------------------------------------------------------------------------------- sample
def queries(c, rng):
    """rows round the surface under the start pose, with two NaN rows and a row outside the 21 bits among them"""
    pts = np.concatenate([c.xyz[::3], c.xyz[::2] + rng.normal(0, 0.35, c.xyz[::2].shape).astype(F32)])
    pts[5] = np.nan
    pts[40, 1] = np.nan
    pts[41] = (6.0e5, 0.0, 0.0)            # 6e5 / 0.5 > 2^20
    return pts


@pytest.mark.parametrize("distance,min_count,origin", [("plane", 1, ZERO), ("plane", 2, ZERO), ("ray", 1, ZERO), ("ray", 2, ZERO),
                                                       ("plane", 1, FAR), ("ray", 2, FAR)])
def test_sample_is_the_float32_restatement_byte_for_byte(distance, min_count, origin):
    c = gpu_case(origin, distance=distance)
    before = [a.tobytes() for a in c.exported]
    fld = field_of(c, min_count)
    pts = queries(c, np.random.default_rng(7))
    d, grad, flag = c.map.sample(dev(pts), c.start, min_count=min_count)
    want = TR.sample(fld, c.voxel, pts, c.start, c.origin, F32)
    same(flag, want.flag, "flag"), same(d, want.d, "d"), same(grad, want.grad, "grad")
    assert want.flag[5] == 0 and want.flag[40] == 0 and want.flag[41] == 0
    seven = int(((want.corners == 7) & (want.flag == 0)).sum())
    # voxel centres, faces and corners: a pure translation by the origin and rows on a lattice of v / 2
    shift = np.eye(4)
    shift[:3, 3] = c.origin
    local = I.transform(I._shifted(c.pose, c.origin, -1), c.xyz, F32)
    lattice = np.unique(np.round(local / F32(c.voxel / 2)), axis=0).astype(F32) * F32(c.voxel / 2)
    d2, grad2, flag2 = c.map.sample(dev(lattice), shift, min_count=min_count)
    want2 = TR.sample(fld, c.voxel, lattice, shift, c.origin, F32)
    same(flag2, want2.flag, "lattice flag"), same(d2, want2.d, "lattice d"), same(grad2, want2.grad, "lattice grad")
    on = want2.flag == 1
    assert set(np.unique(want2.f).tolist()) <= {0.0, 0.5} and (want2.f[on] == 0).all(axis=1).any() and (want2.f[on] == 0.5).all(axis=1).any()
    assert [a.tobytes() for a in c.map.export()] == before, "sample wrote to the table"
    log(f"gpu: sample {distance} map, min_count {min_count}, origin {tuple(origin)}: {int((want.flag == 1).sum())} of {len(pts)} rows and "
        f"{int(on.sum())} of {len(lattice)} lattice rows have a value, all bytes equal; {seven} rows lack exactly one corner")
    assert (want.flag == 1).sum() > 100 and on.sum() > 100 and seven > 0


@pytest.mark.parametrize("cap", [0, 1, 63, 64, 65, 257])
def test_sample_capacities_and_the_rows_past_the_count(cap):
    c = gpu_case()
    n = max(cap - 2, 0)
    rows = c.xyz[100:100 + cap].copy()                      # valid rows everywhere, also past the count
    if n:
        rows[0] = np.nan
    xyz = dev(rows.reshape(-1, 3))
    d, grad, flag = c.map.sample(xyz, c.pose, length=torch.tensor([n], dtype=torch.int32, device=DEV))
    want = TR.sample(field_of(c), c.voxel, rows[:n], c.pose, c.origin, F32)
    assert tuple(d.shape) == (cap,) and tuple(grad.shape) == (cap, 3) and tuple(flag.shape) == (cap,)
    same(flag[:n], want.flag, "flag"), same(d[:n], want.d, "d"), same(grad[:n], want.grad, "grad")
    assert (flag[n:] == -1).all() and (d[n:] == 0).all() and (grad[n:] == 0).all()
    if cap:                                                  # a count beyond the capacity is clamped to it
        flag_all = c.map.sample(xyz, c.pose, length=torch.tensor([cap + 9], dtype=torch.int32, device=DEV))[2]
        assert (flag_all >= 0).all()


def test_sample_of_an_empty_table():
    from deeppointmap_amd.tsdf import TsdfMap
    c = gpu_case()
    m = TsdfMap(c.voxel, max_voxels=1 << 10, origin=ZERO, device=DEV)
    d, grad, flag = m.sample(dev(c.xyz[:300]), c.pose)
    assert (flag == 0).all() and (d == 0).all() and (grad == 0).all()
    res = m.register(dev(c.src), c.start)
    assert int(res.status) == TR.NO_MATCH and res.pose[0].cpu().numpy().tobytes() == c.start.tobytes()
    bare = TsdfMap(c.voxel, max_voxels=1 << 10, device=DEV).register(dev(c.src), c.start)      # no table at all
    assert int(bare.status) == TR.NO_MATCH and bare.pose[0].cpu().numpy().tobytes() == c.start.tobytes() and float(bare.fitness) == 0


# ------------------------------------------------------------------------------------------------------------------------ sums
@pytest.mark.parametrize("rows", [255, 256, 257, 1100])
@pytest.mark.parametrize("kernel_scale", [0.0, 0.1])
def test_the_29_sums_of_the_field_rows(kernel_scale, rows):
    c = gpu_case()
    rng = np.random.default_rng(17)
    src = (c.src[:rows] + rng.normal(0, 0.01, (rows, 3))).astype(F32)
    src[7] = c.xyz[2 * 1681 + 20 * 41 + 20] + F32(0.6) * c.normals[2 * 1681]      # a gross outlier: 0.6 m off the middle of a patch
    init = I.perturbed(c.pose, seed=5, trans=0.05, deg=0.2)
    xyz, count = buffer(src, 1300)
    res, (flag, system) = c.map.register(xyz, init, [(c.tau, 1)], kernel_scale=kernel_scale, debug=True, length=count)
    flag, system = flag.cpu().numpy(), system.cpu().numpy()
    give = flag[:rows] == 1
    assert (flag[rows:] == -1).all() and set(np.unique(flag[:rows]).tolist()) <= {0, 1} and give[7]
    s32 = TR.sample(field_of(c), c.voxel, src, init, c.origin, F32)
    s64 = TR.sample(field_of(c, dtype=np.float64), c.voxel, src, init, c.origin, np.float64)
    assert np.array_equal(TR.gate(s32, c.tau, 0.5, F32), give), "the kernel's rows are the float32 restatement's gate"
    assert (s64.flag[give] == 1).all()
    S32 = TR.system(s32, c.tau, 0.5, kernel_scale, F32, rows=give)[0]
    S64, J, e, w, _ = TR.system(s64, c.tau, 0.5, kernel_scale, np.float64, rows=give)
    floor = TR.system_floor(J, e, w, kernel_scale, s64.q[give], *TR.input_deltas(s32, field_of(c), c.voxel, c.tau))
    bound = np.maximum(3 * np.abs(S32 - S64), floor)
    err = np.abs(system - S64)
    assert system[27] == S64[27] == give.sum() and 0.6 * rows < give.sum() < rows
    ratio = float(np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1), np.where(err > 0, np.inf, 0))))
    out_w = float(w[int(give[:7].sum())])
    log(f"gpu: field sums kernel_scale {kernel_scale}, {rows} rows in 1300: rows given {int(system[27])}, max |gpu-r64| / bound over 29 sums "
        f"{ratio:.3e}, max |gpu-r32| / |r32| {float(np.max(np.abs(system - S32) / np.maximum(np.abs(S32), 1e-300))):.3e}, max |r32-r64| / |r64| "
        f"{float(np.max(np.abs(S32 - S64) / np.maximum(np.abs(S64), 1e-300))):.3e}, the outlier's weight {out_w:.3e}")
    assert (err <= bound).all(), (np.nonzero(err > bound)[0], err, bound)
    assert out_w == 1.0 if kernel_scale == 0 else out_w < 0.1
    x, bad = I.solve(system)
    assert bad is None and int(res.iterations) == 1
    assert np.abs(res.pose[0].cpu().numpy() - I.update(init, x)).max() <= 1e-12
    assert abs(float(res.fitness) - system[27] / rows) < 1e-6 and abs(float(res.rmse) - np.sqrt(system[28] / system[27])) < 1e-6


# --------------------------------------------------------------------------------------------------------------- known answers
@pytest.mark.parametrize("origin,bound_t", [(ZERO, 1e-4), (FAR, 1e-3)])
def test_three_patches_come_back_on_the_gpu(origin, bound_t):
    c = gpu_case(origin)
    before = [a.tobytes() for a in c.exported]
    xyz, count = buffer(c.src, len(c.src) + 11)
    res = c.map.register(xyz, c.start, [(c.tau, 40)], length=count)
    default = c.map.register(xyz, c.start, length=count)                 # schedule None: ((truncation, 30),)
    dt, dr = TR.pose_error(res.pose[0].cpu().numpy(), c.pose)
    log(f"gpu: three patches, plane form, map origin {tuple(origin)}: status {int(res.status)}, iterations {int(res.iterations)}, translation "
        f"error {dt:.3e} m, |R - R_true|_F {dr:.3e}, fitness {float(res.fitness):.3f}, rmse {float(res.rmse):.3e}")
    assert int(res.status) == TR.CONVERGED and float(res.fitness) > 0.8
    assert dt <= bound_t and dr <= 1e-4, (dt, dr)
    assert torch.equal(default.pose, res.pose) and int(default.status) == TR.CONVERGED
    assert [a.tobytes() for a in c.map.export()] == before, "register wrote to the table"


def test_the_ray_form_follows_the_restatement():
    c = gpu_case(distance="ray")
    xyz, count = buffer(c.src, len(c.src) + 11)
    res = c.map.register(xyz, c.start, [(c.tau, 40)], length=count)
    r = {dt: TR.register(field_of(c, dtype=dt), c.voxel, c.src, c.origin, c.start, [(c.tau, 40)], dtype=dt) for dt in (F32, np.float64)}
    pose = res.pose[0].cpu().numpy()
    diff, between = float(np.abs(pose - r[np.float64]["pose"]).max()), float(np.abs(r[F32]["pose"] - r[np.float64]["pose"]).max())
    dt, dr = TR.pose_error(pose, c.pose)
    log(f"gpu: three patches, RAY form: status {int(res.status)} (r64 {r[np.float64]['status']}), iterations {int(res.iterations)} (r64 "
        f"{r[np.float64]['iterations']}), |gpu - r64| {diff:.3e}, |r32 - r64| {between:.3e}, off the truth by {dt:.3e} m / {dr:.3e} (no bar)")
    assert int(res.status) in (TR.CONVERGED, TR.MAX_ITER)
    assert diff <= max(3 * between, 1e-4)


def test_one_patch_alone_is_singular_on_the_gpu():
    c = gpu_case(which=(0,))
    res = c.map.register(dev(c.src), c.start, [(c.tau, 40)])
    log(f"gpu: one patch alone: status {int(res.status)}, iterations {int(res.iterations)}, fitness {float(res.fitness):.3f}")
    assert int(res.status) == TR.SINGULAR and int(res.iterations) == 0
    assert res.pose[0].cpu().numpy().tobytes() == c.start.tobytes()


def test_a_stage_beyond_the_truncation_is_refused():
    from deeppointmap_amd import _lib, ops
    c = gpu_case()
    m = c.map
    xyz, count = buffer(c.src)
    with pytest.raises(ValueError):
        m.register(xyz, c.start, [(c.tau, 2), (c.tau * 1.001, 2)], length=count)
    init = dev(c.start)
    with pytest.raises(ValueError):
        ops.tsdf_register(*m._map(), m.truncation, xyz, count, init, [(c.tau + 0.1, 1)])
    # the entry point itself
    lib = _lib.load()
    n = len(c.src)
    ws = torch.zeros(lib.dpm_tsdf_register_scratch_bytes(n), dtype=torch.uint8, device=DEV)
    assert lib.dpm_tsdf_register_scratch_bytes(0) == 0 and ws.numel() == 512 + 256 * ((n + 255) // 256)
    call = lambda max_dist, truncation: c_register(c, xyz, count, init, max_dist, truncation, ws.data_ptr())[0]
    assert call(c.tau, c.tau) == 0 and call(c.tau * 1.001, c.tau) == -1                      # -1: invalid argument
    assert call(0.0, c.tau) == -1 and call(float("nan"), c.tau) == -1 and call(1.0, 65.0) == -1
    torch.cuda.synchronize()


def c_register(c, xyz, count, init, max_dist, truncation, ws_ptr, iters=1):
    """dpm_tsdf_register through the C ABI by hand with `ws_ptr` as its workspace -> (status, the outputs' bytes)"""
    from deeppointmap_amd import _lib
    m = c.map
    o = (ctypes.c_double * 3)(*c.origin)
    dist, its = (ctypes.c_double * 1)(max_dist), (ctypes.c_int32 * 1)(iters)
    pose = torch.zeros(16, dtype=torch.float64, device=DEV)
    f = torch.zeros(2, dtype=torch.float32, device=DEV)
    i = torch.zeros(2, dtype=torch.int32, device=DEV)
    system = torch.zeros(29, dtype=torch.float64, device=DEV)
    status = _lib.load().dpm_tsdf_register(m.table.data_ptr(), m.max_voxels, m.voxel_size, ctypes.addressof(o), truncation, m.unit, 0.5,
                                           xyz.data_ptr(), count.data_ptr(), xyz.shape[0], init.data_ptr(), ctypes.addressof(dist),
                                           ctypes.addressof(its), 1, 0.0, 1e-7, 1e-6, pose.data_ptr(), f[:1].data_ptr(), f[1:].data_ptr(),
                                           i[:1].data_ptr(), i[1:].data_ptr(), None, system.data_ptr(), ws_ptr, None)
    torch.cuda.synchronize()
    return status, [t.cpu().numpy().tobytes() for t in (pose, f, i, system)]


@pytest.mark.parametrize("cap", [257, 1300])
def test_the_workspace_stays_inside_its_bytes(cap):
    """tests/test_gpu_workspace_guard.py's check for this entry point: the call with `buffer + 4096` and with `buffer + 4096 + 80`
    (16-byte aligned, not 256) as its workspace leaves every byte outside [workspace, workspace + bytes) at 0xA5 and gives the
    outputs of a call with a workspace of its own"""
    from deeppointmap_amd import _lib
    c = gpu_case()
    xyz, count = buffer(c.src[:min(cap, len(c.src)) - 3], cap)
    init = dev(c.start)
    nbytes = _lib.load().dpm_tsdf_register_scratch_bytes(cap)
    own = torch.zeros(nbytes, dtype=torch.uint8, device=DEV)
    status, want = c_register(c, xyz, count, init, c.tau, c.tau, own.data_ptr(), iters=2)
    assert status == 0
    for shift in (0, 80):
        guard = torch.full((4096 + nbytes + 4096 + 256,), 0xA5, dtype=torch.uint8, device=DEV)
        status, got = c_register(c, xyz, count, init, c.tau, c.tau, guard.data_ptr() + 4096 + shift, iters=2)
        assert status == 0 and got == want, shift
        assert bool((guard[:4096 + shift] == 0xA5).all()) and bool((guard[4096 + shift + nbytes:] == 0xA5).all()), shift


# ------------------------------------------------------------------------------------------------------- determinism and capture
def as_bytes(res, extra=()):
    return [t.cpu().numpy().tobytes() for t in tuple(res) + tuple(extra)]


def test_same_bytes_twice_and_from_a_captured_graph():
    c = gpu_case()
    before = [a.tobytes() for a in c.exported]
    xyz, count = buffer(c.src, 1300)
    init = dev(c.start)
    first = as_bytes(*c.map.register(xyz, init, [(c.tau, 3)], kernel_scale=0.1, debug=True, length=count))
    again = as_bytes(*c.map.register(xyz, init, [(c.tau, 3)], kernel_scale=0.1, debug=True, length=count))
    assert first == again
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        c.map.register(xyz, init, [(c.tau, 1)], length=count)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = c.map.register(xyz, init, [(c.tau, 3)], kernel_scale=0.1, debug=True, length=count)
    graph.replay()
    torch.cuda.synchronize()
    assert as_bytes(*captured) == first, "replayed from a captured graph"
    assert [a.tobytes() for a in c.map.export()] == before


# --------------------------------------------------------------------------------------------------------------------- tracker
def test_the_tracker_in_the_box_room():
    from deeppointmap_amd import augment
    from deeppointmap_amd.tsdf import TsdfTracker
    xyz, nrm, true = TR.box_room()
    frames = [(dev(a), dev(b)) for a, b in zip(xyz, nrm)]
    tr = TsdfTracker(BOX_KW["voxel"], max_voxels=1 << 17, device=DEV, distance="plane", register_every=BOX_KW["register_every"])
    torch.cuda.synchronize()
    syncs = []
    for k, (a, b) in enumerate(frames):
        n = augment.host_syncs()
        pose, step = tr.step(a, b, pose=true[0] if k == 0 else None)
        syncs.append(augment.host_syncs() - n)
        assert step.integrated and np.array_equal(pose, tr.poses[-1])
    want, statuses, _, lost, _ = box_tracker("plane")
    got = np.stack(tr.poses)
    assert syncs == [0] + [1] * (len(frames) - 1), syncs
    assert tr.lost == 0 == lost and all(s.status in (TR.CONVERGED, TR.MAX_ITER) for s in tr.steps)
    err = np.linalg.norm(got[:, :3, 3] - true[:, :3, 3], axis=1)
    err64 = np.linalg.norm(want[:, :3, 3] - true[:, :3, 3], axis=1)
    worst = float(np.abs(got - want).max())
    log(f"gpu: box-room tracker, plane form: statuses {[s.status for s in tr.steps]}, iterations {[s.iterations for s in tr.steps]}, fitness "
        f"{min(s.fitness for s in tr.steps):.3f}..{max(s.fitness for s in tr.steps):.3f}, translation error per frame (mm) "
        f"{np.round(err * 1e3, 2).tolist()} (float64 restatement {np.round(err64 * 1e3, 2).tolist()}), worst |gpu - r64| {worst:.3e}")
    assert worst <= 1e-3
    assert err[-1] <= 2 * err64[-1], (err[-1], err64[-1])
    # a frame registered against an empty region: lost, and nothing is written
    tr.map.check()
    before = [a.tobytes() for a in tr.map.export()]
    away = true[-1].copy()
    away[:3, 3] += (40.0, 0.0, 0.0)
    pose, step = tr.step(*frames[-1], pose=away)
    assert tr.lost == 1 and not step.integrated and step.status == TR.NO_MATCH and np.array_equal(pose, away) and len(tr.poses) == len(frames) + 1
    assert [a.tobytes() for a in tr.map.export()] == before
