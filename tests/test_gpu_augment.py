"""GPU: the training transforms (csrc/augment.hip through deeppointmap_amd.augment) against the reference's outputs
(tests/golden/augment_*.npz) and the restatement (tests/augment_restated.py, itself held to those outputs on the CPU).

Selections are compared as exact index lists (GroundFilter as documented: sets + lowest-position representatives);
RandomShield leaves out the points inside the exclusion band of augment_restated.shield_band (device atan2f / sqrtf may sit
a couple of ulp from the host's) and fails when the band holds more than 0.1 % of the points.  Affine results are held
per component to 4 * 2^-24 * (sum_k |R_ik||x_k| + |t_i|): three products and three additions at half an ulp each, with
slack for the reference's unknown fma / summation order; the largest observed errors go to bench_out/augment_accuracy.log."""
import os
import random
import subprocess
import sys

import numpy as np
import pytest
import torch

import augment_restated as A
from conftest import ROOT, T, load_golden

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SIZES = [1, 63, 64, 65, 1023, 1024, 1025, 4097, 20000]


@pytest.fixture(scope="module")
def gold():
    g = load_golden("augment_ref.npz")
    g.update(load_golden("augment_scan.npz"))
    return g


@pytest.fixture(scope="module")
def aug():
    from deeppointmap_amd import augment
    return augment


def note(line):
    try:
        os.makedirs(os.path.join(ROOT, "bench_out"), exist_ok=True)
        with open(os.path.join(ROOT, "bench_out", "augment_accuracy.log"), "a") as f:
            f.write(line + "\n")
    except OSError:
        pass


def frame(aug, xyz, extra=0, **kw):
    """a frame with `extra` rows of NaN garbage past its count"""
    xyz = np.asarray(xyz, np.float32)
    pcd = aug.PointCloud(T(xyz), capacity=xyz.shape[0] + extra, **kw)
    if extra:
        pcd.xyz[xyz.shape[0]:] = float("nan")
    return pcd


def result(pcd):
    """(original indices, xyz) of the live rows, and the rows past the count must not have been counted"""
    n = int(pcd.count.item())
    assert 0 <= n <= pcd.cap
    return pcd.idx[:n].cpu().numpy().astype(np.int64), pcd.xyz[:n].cpu().numpy()


def check_selection(pcd, xyz, want):
    idx, out = result(pcd)
    assert np.array_equal(idx, np.asarray(want, np.int64))
    assert np.array_equal(out, np.asarray(xyz, np.float32)[idx])       # the rows moved with their indices, NaN-free


# ------------------------------------------------------------------------------------------------ kernels vs fixture
def test_ground_filter(gold, aug):
    for name, key in (("ground", "scan"), ("ground_edge", "ground_edge.in")):
        L, W, gw, gh = gold[name + ".params"]
        xyz = gold[key]
        pcd = aug.ground_filter(frame(aug, xyz, 37), int(L), int(W), float(gw), float(gh))
        idx, _ = result(pcd)
        A.check_ground(gold, name, xyz, idx)
        check_selection(pcd, xyz, A.ground_filter(xyz, int(L), int(W), float(gw), float(gh))["keep"])
        pcd = aug.ground_filter(frame(aug, xyz, 37), int(L), int(W), float(gw), float(gh), preserve_sparse_ground=False)
        check_selection(pcd, xyz, np.sort(gold[name + ".idx"][:int(gold[name + ".n_nonground"])]))
    pcd = aug.ground_filter(frame(aug, xyz, 5), 16, 16, 1.0, 0.0)                     # ground_height <= 0: the identity
    check_selection(pcd, xyz, np.arange(xyz.shape[0]))


def test_voxel_sample(gold, aug):
    from deeppointmap_amd.preprocess import preprocess_scan
    for name, key in (("voxel", "scan"), ("voxel_one", "voxel_one.in"), ("voxel_each", "voxel_each.in")):
        xyz, vs = gold[key], float(gold[name + ".voxel_size"])
        for ret in ("first", "center"):
            pcd = aug.voxel_sample(frame(aug, xyz, 37), vs, ret)
            check_selection(pcd, xyz, gold[f"{name}.{ret}"])
            assert np.array_equal(gold[f"{name}.{ret}"], A.voxel_sample(xyz, vs, ret))
            pcd.check()
        pts, pad, idx = preprocess_scan(T(xyz), vs, 0.0, float("inf"), 1.0, return_index=True)   # the crop and the division off
        first = aug.voxel_sample(frame(aug, xyz, 37), vs, "first")
        n = int(first.count.item())
        assert torch.equal(first.idx[:n], idx) and torch.equal(first.xyz[:n], pts[0].t().contiguous())
    pcd = aug.voxel_sample(frame(aug, gold["scan"]), 0.05, "center", max_cells=4096)
    with pytest.raises(ValueError, match="max_cells"):
        pcd.check()
    assert int(pcd.count.item()) == 0
    with pytest.raises(NotImplementedError):
        aug.voxel_sample(frame(aug, gold["scan"]), 0.5, "center", num=100)


def test_mask_selections(gold, aug):
    scan = gold["scan"]
    lo, hi = gold["distance.params"]
    check_selection(aug.distance_sample(frame(aug, scan, 37), float(lo), float(hi)), scan, gold["distance.idx"])
    u = torch.full((scan.shape[0] + 37,), float("nan"), device=DEV)
    u[:scan.shape[0]] = T(gold["drop.u"]).to(DEV)
    check_selection(aug.random_drop(frame(aug, scan, 37), float(gold["drop.ratio"]), u), scan, gold["drop.idx"])


def test_random_shield(gold, aug):
    scan, w = gold["scan"], gold["shield.wedges"]
    assert w.shape[0] == 4 and 0 < w[:, 2].sum() < 4                      # max_num wedges, one wraps past 180 degrees
    idx, out = result(aug.random_shield(frame(aug, scan, 37), w))
    assert np.all(np.diff(idx) > 0) and np.array_equal(out, scan[idx])
    band = A.shield_band(scan, w)
    assert band.mean() <= 1e-3, f"{band.mean():.2e} of the points lie in the exclusion band"
    got, want = np.zeros(scan.shape[0], bool), np.zeros(scan.shape[0], bool)
    got[idx], want[gold["shield.idx"]] = True, True
    assert np.array_equal(got[~band], want[~band])
    note(f"RandomShield: {int((got != want).sum())} of {scan.shape[0]} verdicts differ from the reference, {int(band.sum())} points in the band")
    with pytest.raises(ValueError):
        aug.random_shield(frame(aug, scan), np.zeros((17, 4), np.float32))


def mat_bound(a, b):
    return 4 * 2.0 ** -24 * (np.abs(a).astype(np.float64) @ np.abs(b).astype(np.float64))


def test_affine_transforms(gold, aug):
    small = gold["scan"][:4097]
    R_in, T_in = gold["rt.R_in"], gold["rt.T_in"]
    for k in (0, 1):
        R_aug, T_aug = gold[f"rt{k}.R_aug"], gold[f"rt{k}.T_aug"]
        pcd = aug.random_rt(frame(aug, small, 37, rotation=T(R_in), translation=T(T_in)), T(R_aug), T(T_aug))
        idx, out = result(pcd)
        assert np.array_equal(idx, np.arange(4097)) and bool(torch.isnan(pcd.xyz[4097:]).all())   # rows past the count untouched
        val, bound = A.affine(small, R_aug, T_aug)
        for what, ref in (("reference", gold[f"rt{k}.out"].astype(np.float64)), ("restatement", val)):
            err = np.abs(out - ref)
            note(f"RandomRT call {k} vs {what}: max error {err.max():.3e}, largest error / bound {np.max(err / bound):.3f}")
            assert np.all(err <= bound)
        # the pose algebra, same form of bound (T_new also carries R_new's error times |T_aug|)
        R_new, T_new, calib = pcd.R.numpy(), pcd.T.numpy(), pcd.calib.numpy()
        bR = mat_bound(R_in, R_aug.T)
        bT = 4 * 2.0 ** -24 * np.abs(T_in) + mat_bound(R_new, T_aug) + bR @ np.abs(T_aug)
        for what, got, ref, b in (("R_new", R_new, gold[f"rt{k}.R_new"], bR), ("T_new", T_new, gold[f"rt{k}.T_new"], bT),
                                  ("calib", calib, gold[f"rt{k}.calib"], 4 * 2.0 ** -24 * np.abs(gold[f"rt{k}.calib"]))):
            err = np.abs(got.astype(np.float64) - ref)
            note(f"RandomRT call {k} {what}: max error {err.max():.3e}")
            assert np.all(err <= b), what
    _, out = result(aug.vertical_correct(frame(aug, small, 37), float(gold["vc.angle"])))
    val, bound = A.vertical_correct(small, float(gold["vc.angle"]))
    for what, ref in (("reference", gold["vc.out"].astype(np.float64)), ("restatement", val)):
        err = np.abs(out - ref)
        note(f"VerticalCorrect vs {what}: max error {err.max():.3e}, largest error / bound {np.max(err / bound):.3f}")
        assert np.all(err <= bound)
    _, out = result(aug.vertical_correct(frame(aug, small), 0))
    assert np.array_equal(out, small)
    # jitter and normalisation are exact
    j = torch.full((4097 + 37, 3), float("nan"), device=DEV)
    j[:4097] = T(gold["jitter.j"]).to(DEV)
    assert np.array_equal(result(aug.random_pos_jitter(frame(aug, small, 37), j))[1], gold["jitter.out"])
    assert np.array_equal(result(aug.coordinates_normalization(frame(aug, small, 37), 60.0))[1], gold["norm.out"])


def test_index_transforms(gold, aug):
    small = gold["scan"][:4097]
    check_selection(aug.random_shuffle(frame(aug, small, 37), T(gold["shuffle.perm"]).to(DEV)), small, gold["shuffle.idx"])
    check_selection(aug.random_sample(frame(aug, small, 37), 1000, T(gold["sample.perm"]).to(DEV)), small, gold["sample.idx"])
    check_selection(aug.random_sample(frame(aug, small, 37), 5000, T(gold["sample.perm"]).to(DEV)), small, np.arange(4097))
    # FarthestPointSample: the encoder's FPS on the live rows, first pick = point 0; a short frame stays as it is
    from deeppointmap_amd import ops
    want = ops.fps(T(small).to(DEV).unsqueeze(0), torch.tensor([4097], device=DEV, dtype=torch.int32), 256)[0][0]
    check_selection(aug.farthest_point_sample(frame(aug, small, 37), 256), small, want.cpu().numpy())
    check_selection(aug.farthest_point_sample(frame(aug, small[:100], 400), 256), small[:100], np.arange(100))


# ------------------------------------------------------------------------------------------------ compaction shapes
@pytest.mark.parametrize("n", SIZES)
def test_compaction_shapes(gold, aug, n):
    """every selection at sizes around the wave, the block and the 4096-item chunk, count < capacity with NaN past it,
    nothing survives / everything survives"""
    xyz = gold["scan"][:n]
    g = torch.Generator().manual_seed(n)
    u = torch.rand(n + 37, generator=g)
    check_selection(aug.distance_sample(frame(aug, xyz, 37), 1.0, 20.0), xyz, A.distance_sample(xyz, 1.0, 20.0))
    check_selection(aug.distance_sample(frame(aug, xyz, 37), 0.0, 1e9), xyz, np.arange(n))
    check_selection(aug.distance_sample(frame(aug, xyz, 37), 1e8, 1e9), xyz, [])
    check_selection(aug.random_drop(frame(aug, xyz, 37), 0.4, u.to(DEV)), xyz, A.random_drop(u[:n].numpy(), 0.4))
    check_selection(aug.random_drop(frame(aug, xyz, 37), 2.0, u.to(DEV)), xyz, [])
    check_selection(aug.ground_filter(frame(aug, xyz, 37), 160, 160, 0.3, 0.25), xyz, A.ground_filter(xyz, 160, 160, 0.3, 0.25)["keep"])
    for ret in ("first", "center"):
        check_selection(aug.voxel_sample(frame(aug, xyz, 37), 0.5, ret), xyz, A.voxel_sample(xyz, 0.5, ret))
    perm = torch.randperm(n, generator=g)
    check_selection(aug.random_shuffle(frame(aug, xyz, 37), perm.to(DEV)), xyz, perm.numpy())
    # an emptied frame goes through every kind of kernel and stays empty
    empty = aug.distance_sample(frame(aug, xyz, 37), 1e8, 1e9)
    for f in (lambda p: aug.voxel_sample(p, 0.5, "center"), lambda p: aug.ground_filter(p, 160, 160, 0.3, 0.25),
              lambda p: aug.random_rt(p, torch.eye(3), torch.ones(3, 1)), lambda p: aug.random_shuffle(p, perm.to(DEV))):
        empty = f(empty)
        assert int(empty.count.item()) == 0
    empty.check()


def test_pack_and_collate(gold, aug):
    scan = gold["scan"]
    lens = [1000, 1, 257, 640]
    mk = lambda: [frame(aug, scan[100 * k: 100 * k + n], 11 * k) for k, n in enumerate(lens)]
    parts = [scan[100 * k: 100 * k + n] for k, n in enumerate(lens)]
    for P in (-1, 1000, 1300):                               # the longest frame (implicitly and explicitly), and longer
        pts, R, Tt, pad, calib = aug.collate_frames(mk(), P)
        wp, wm = A.pack(parts, P)
        assert np.array_equal(pts.cpu().numpy(), wp) and np.array_equal(pad.cpu().numpy(), wm) and pad.dtype == torch.bool
        assert tuple(R.shape) == (4, 3, 3) and tuple(Tt.shape) == (4, 3, 1) and tuple(calib.shape) == (4, 4, 4)
    with pytest.raises(RuntimeError, match=r"\(1000\) is greater than `padding_to` \(999\)"):
        aug.collate_frames(mk(), 999)                        # one point short
    one = aug.ToTensor(padding_to=1200, use_calib=True)(frame(aug, parts[0], 5))
    assert len(one) == 5 and np.array_equal(one[0].cpu().numpy(), A.pack(parts[:1], 1200)[0][0]) and tuple(one[3].shape) == (1200,)
    assert len(aug.ToTensor()(frame(aug, parts[2]))) == 4


# ------------------------------------------------------------------------------------------------ chains
def chain_specs():
    import json
    c = json.loads(str(load_golden("augment_chains.npz")["chains"]))
    return {k: v["spec"] for k, v in c.items()}


def split_records(records):
    out = []
    for name, kw in records:
        if name == "frame":
            out.append([])
        else:
            out[-1].append((name, kw))
    return out


def raw_frames(gold, aug, k=3):
    return [frame(aug, gold["scan"][5000 * b: 5000 * b + 4500 + 100 * b], 64) for b in range(k)]


def compare_batch(gold, aug, pcds, records):
    """every frame against the restatement's replay of its records, transform by transform: selections exact, coordinates
    within the bound.  After each transform the restatement continues from the DEVICE's coordinates (so a selection that
    follows an affine transform sees the same input on both sides: a coordinate one ulp apart may sit on the other side of a
    voxel face), and the functional layer's step-by-step result must be the class layer's result byte for byte."""
    for b, (pcd, recs, dev) in enumerate(zip(pcds, split_records(records), raw_frames(gold, aug))):
        host = A.Frame(gold["scan"][5000 * b: 5000 * b + 4500 + 100 * b])
        worst = 0.0
        for rec in recs:
            dev, host = aug.replay(dev, [rec]), A.replay(host, [rec])
            idx, out = result(dev)
            assert np.array_equal(idx, host.idx), (b, rec[0])
            err = np.abs(out.astype(np.float64) - host.xyz)
            assert np.all(err <= host.err + 2.0 ** -24 * np.abs(host.xyz)), (b, rec[0], float(err.max()))
            worst = max(worst, float(err.max()) if err.size else 0.0)
            host.xyz, host.err = out, np.zeros(out.shape)
            for what, got, ref in (("R", dev.R, host.R), ("T", dev.T, host.T), ("calib", dev.calib, host.calib)):
                assert np.all(np.abs(got.numpy() - ref) <= 8 * 2.0 ** -24 * np.maximum(1.0, np.abs(ref))), (what, rec[0])
        n = int(pcd.count.item())
        assert int(dev.count.item()) == n and torch.equal(dev.xyz[:n], pcd.xyz[:n]) and torch.equal(dev.idx[:n], pcd.idx[:n])
        assert torch.equal(dev.R, pcd.R) and torch.equal(dev.T, pcd.T) and torch.equal(dev.calib, pcd.calib)
        note(f"chain frame {b}: {len(recs)} transforms, {n} points, max coordinate error of a step {worst:.3e}")


@pytest.mark.parametrize("name", ["train", "choice"])
def test_chain_reference_rng_vs_restatement(gold, aug, name):
    """Compose chains (a RandomChoice in one, a paired RandomRT called for every frame in the other) through the class
    layer with the reference draw source, then through the restatement with the recorded draws"""
    random.seed(3)
    torch.manual_seed(3)
    chain = aug.get_transforms(chain_specs()[name])
    pcds, records = aug.transform_frames(raw_frames(gold, aug), chain, rng="reference", return_draws=True)
    names = [r[0] for r in records]
    assert names.count("frame") == 3 and ("random_rt" in names or name == "choice")
    compare_batch(gold, aug, pcds, records)
    pts, R, Tt, pad, calib = aug.collate_frames(pcds, 4096)
    for b, pcd in enumerate(pcds):                            # the batch equals the frames padded by hand
        idx, out = result(pcd)
        assert np.array_equal(pts[b].cpu().numpy(), A.pack([out], 4096)[0][0])
        assert np.array_equal(pad[b].cpu().numpy(), np.arange(4096) >= idx.shape[0])
        assert torch.equal(R[b].cpu(), pcd.R) and torch.equal(Tt[b].cpu(), pcd.T) and torch.equal(calib[b].cpu(), pcd.calib)


@pytest.mark.parametrize("name", ["train", "choice"])
def test_chain_generator_mode(gold, aug, name):
    """the training mode: identical bytes twice with the same generator seed, ONE host synchronisation per batch, and an
    exact replay through the functional layer from the returned draws"""
    def run():
        gen = torch.Generator(device=DEV)
        gen.manual_seed(11)
        chain = aug.get_transforms(chain_specs()[name])
        before = aug.host_syncs()
        pcds, records = aug.transform_frames(raw_frames(gold, aug), chain, rng=gen, return_draws=True)
        batch = aug.collate_frames(pcds, 4608)
        return pcds, records, batch, aug.host_syncs() - before
    pcds, records, batch, syncs = run()
    pcds2, _, batch2, _ = run()
    assert syncs == 1
    assert all(torch.equal(a, b) for a, b in zip(batch, batch2))
    assert all(torch.equal(a.count, b.count) and torch.equal(a.indices(), b.indices()) for a, b in zip(pcds, pcds2))
    compare_batch(gold, aug, pcds, records)                     # and it is the same computation as the restatement's
    for pcd, raw, recs in zip(pcds, raw_frames(gold, aug), split_records(records)):
        again = aug.replay(raw, recs)
        n = int(pcd.count.item())
        assert int(again.count.item()) == n and torch.equal(again.xyz[:n], pcd.xyz[:n]) and torch.equal(again.idx[:n], pcd.idx[:n])
        assert torch.equal(again.R, pcd.R) and torch.equal(again.T, pcd.T) and torch.equal(again.calib, pcd.calib)
    lengths = [int(p.count.item()) for p in pcds]
    assert min(lengths) > 0 and bool(batch[3].sum(1).cpu().eq(torch.tensor([4608 - n for n in lengths])).all())


# ------------------------------------------------------------------------------------------------ drop-in
def test_dropin_builds_the_shipped_inference_chain(gold):
    """dataloader.transforms.get_transforms on the transforms dict of the shipped inference configs (configs/infer/*.yaml:21-29)
    gives preprocess_scan's points: exactly for the stages with a reference pin (VoxelSample 'first', DistanceSample,
    CoordinatesNormalization), and for the whole chain, which runs the same filter kernels"""
    code = (
        "import sys; sys.path.insert(0, %r); sys.path.insert(1, %r); sys.path.insert(2, %r)\n"
        "import torch, numpy as np\n"
        "from dataloader.transforms import get_transforms, PointCloud, PointCloudTransforms\n"
        "from deeppointmap_amd.preprocess import preprocess_scan\n"
        "from conftest import load_golden\n"
        "xyz = torch.from_numpy(load_golden('augment_scan.npz')['scan']) * 2.5\n"
        "head = {'VoxelSample': {'voxel_size': 0.3, 'retention': 'first'}, 'ToGPU': {}, 'DistanceSample': {'min_dis': 1.0, 'max_dis': 60.0}}\n"
        "tail = {'CoordinatesNormalization': {'ratio': 60.0}, 'ToCPU': {}, 'ToTensor': {'padding_to': -1}}\n"
        "filt = {'OutlierFilter': {'nb_neighbors': 10, 'std_ratio': 3.0}, 'LowPassFilter': {'normals_radius': 0.5, 'normals_num': 16, 'filter_std': 2.0, 'flux': 4, 'max_remain': -1}}\n"
        "pts, R, T, pad = get_transforms({**head, **tail})(PointCloud(xyz.numpy()))\n"
        "want, wpad = preprocess_scan(xyz)\n"
        "assert torch.equal(pts, want[0]) and torch.equal(pad, wpad[0]) and pts.shape[1] > 5000\n"
        "class Args: transforms = {**head, **filt, **tail}\n"
        "pts, R, T, pad, orig = PointCloudTransforms(Args, mode='infer')(PointCloud(xyz.numpy()))\n"
        "want, wpad = preprocess_scan(xyz, outlier=(10, 3.0), lowpass=(0.5, 16, 2.0, 4))\n"
        "assert torch.equal(pts, want[0]) and torch.equal(orig.cpu(), xyz) and 0 < pts.shape[1] < 20000\n"
        "print('ok')\n") % (os.path.join(ROOT, "deeppointmap_amd", "dropin"), ROOT, os.path.join(ROOT, "tests"))
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stderr[-3000:]
