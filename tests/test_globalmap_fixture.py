"""ResultLogger.draw_trajectory / plot_data against the reference's own draw_trajectory (tests/golden/result_map.npz, made by
make_golden_map.py from recoder.py:99-203 on a 12-scan, two-agent graph with all four edge types and one key frame without
a cloud).  Our renderer's matplotlib calls are recorded the same way (tests/golden/map_calls.py):
  * draft (CPU): every call -- scan markers by type and agent colour, ground-truth dots, edges by type, in order -- equal;
  * the map inputs (CPU): the clouds and poses handed to the voxel map, transformed, are the points the reference hands to
    Vector3dVector, in the same order (its transform is a torch fp32 matmul, ours the kernel's fma chain: 1e-5 m);
  * non-draft (GPU): the scan and edge calls equal, the two map scatters equal as point sets within 1e-5 m.
The voxel semantics themselves are the restatement's (open3d is absent where the fixture was made)."""
import json
import os
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN, load_golden
from test_globalmap_host import transform_fp32

sys.path.insert(0, GOLDEN)
import map_calls  # noqa: E402


def _backend(device):
    from deeppointmap_amd.consumer import Rank0Consumer
    g = load_golden("result_map.npz")
    b = Rank0Consumer(None, device, slam_args=dict(result_maps=True))
    for i, (tok, ty) in enumerate(zip(g["scan_token"].tolist(), g["scan_type"].tolist())):
        b.type[tok] = ty
        b.poses[tok] = torch.from_numpy(g[f"scan{i}.SE3_pred"])
        b.gt[tok] = torch.from_numpy(g[f"scan{i}.SE3_gt"])
        if f"scan{i}.full_pcd" in g:
            b.map_clouds[tok] = torch.from_numpy(g[f"scan{i}.full_pcd"]).to(device)
        if ty == "full":
            b.desc[tok] = torch.from_numpy(g[f"scan{i}.key_points"]).to(device)
    for (src, dst), ty in zip(g["edges"].tolist(), g["edge_type"].tolist()):
        b.edges[(src, dst)] = dict(type=ty)
    return b, g


def _our_calls(b, tmp_path, draft):
    from deeppointmap_amd.system import ResultLogger
    with map_calls.recording() as calls:
        ResultLogger(b, str(tmp_path)).draw_trajectory("t", draft=draft)
    assert (tmp_path / "t.map.jpg").exists()
    return calls


def test_fixture_covers_what_it_should():
    g = load_golden("result_map.npz")
    assert set(g["edge_type"].tolist()) == {"odom", "locz", "loop", "prxy"}
    assert len(set((g["scan_token"] >> 16).tolist())) == 2 and "non-keyframe" in g["scan_type"].tolist()
    assert any(f"scan{i}.full_pcd" not in g for i in range(len(g["scan_token"])))
    assert g["voxel_size"].tolist() == [0.5, 0.5]


def test_draft_picture_equals_the_reference_s(tmp_path):
    b, g = _backend("cpu")
    want = json.loads(str(g["draft.calls"]))
    got = _our_calls(b, tmp_path, draft=True)
    assert len(got) == len(want)
    for i, (a, w) in enumerate(zip(got, want)):
        assert a == w, (i, a, w)


def test_map_inputs_are_the_reference_s_points():
    """which points go into each map, in which order, transformed how"""
    from deeppointmap_amd.system import ResultLogger
    b, g = _backend("cpu")
    (fc, fp), (kc, kp) = ResultLogger(b, None).map_inputs()
    for (clouds, poses), want in (((fc, fp), g["vector3d.full"]), ((kc, kp), g["vector3d.key"])):
        ours = np.concatenate([transform_fp32(c.numpy(), p.numpy()) for c, p in zip(clouds, poses)], axis=1).T
        assert ours.shape == want.shape
        np.testing.assert_allclose(ours, want, rtol=0, atol=1e-5)


@pytest.mark.gpu
def test_full_picture_equals_the_reference_s(tmp_path):
    from scipy.spatial import cKDTree
    b, g = _backend(torch.device("cuda:0"))
    want = json.loads(str(g["full.calls"]))
    got = _our_calls(b, tmp_path, draft=False)
    assert len(got) == len(want)
    for i, (a, w) in enumerate(zip(got, want)):
        if map_calls.is_map_layer(w):
            assert map_calls.is_map_layer(a) and a["style"] == w["style"], (i, a["style"], w["style"])
            pa, pw = np.array([a["x"], a["y"]]).T, np.array([w["x"], w["y"]]).T
            assert pa.shape == pw.shape, (i, pa.shape, pw.shape)
            d, _ = cKDTree(pw).query(pa)
            assert d.max() < 1e-5, (i, d.max())
            d, _ = cKDTree(pa).query(pw)
            assert d.max() < 1e-5, (i, d.max())
        else:
            assert a == w, (i, a, w)
