"""CPU: every dpm_*_workspace_bytes entry point returns, argument for argument, the number recorded from the library before
the workspace layouts moved onto csrc/workspace.h's cursor (size and carve one function).  The host entry points need no GPU.

PARENT holds that record.  Three entry points are allowed to differ from it, the dpm_knn_workspace_bytes family: their old
formula was never the end of their carve (a sum of unrounded slices plus 1024 + 256 bytes of slack, while the carve rounds
every slice), so their number is now the cursor's own.  It stays within 4 KiB of the record: 1280 bytes of fixed slack plus
at most five roundings of 255 bytes."""
import ctypes

import pytest

# arguments ("i": int, "L": long long) and shapes per entry point: the degenerate ones that give 0, one past a rounding
# boundary (N = 256 k + 1), and both sides of every branch of the layout
SHAPES = {
    # N <= 16384 (no packing), 16384 < N <= 65536 (Sort-Tile-Recursive packing), N > 65536; N = 256 k + 1; N no multiple of 16
    "dpm_fps_workspace_bytes": ("iii", [(0, 0, 0), (1, 1, 1), (2, 300, 8), (2, 257, 8), (1, 16384, 64), (2, 16385, 8), (3, 20001, 16),
        (1, 32768, 1024), (4, 65536, 2048), (2, 65537, 8), (1, 100000, 8)]),
    # N < 1024: no grid
    "dpm_knn_workspace_bytes": ("ii", [(1, 0), (2, 300), (8, 1023), (1, 1024), (2, 1024), (2, 1025), (3, 4097), (4, 8192), (12, 16384)]),
    "dpm_voxel_sampler_workspace_bytes": ("iiL", [(0, 16, 16), (2, 0, 16), (2, 16, 0), (1, 1, 1), (2, 200, 64), (1, 257, 1000),
        (3, 4097, 4095), (2, 8192, 4096), (2, 8192, 65536), (1, 20000, 100001)]),
    "dpm_attention_split_workspace_bytes": ("iiiii", [(0, 8, 1, 32, 2), (1, 8, 1, 32, 0), (1, 8, 1, 32, 2), (1, 1, 1, 32, 2),
        (2, 65, 4, 32, 3), (1, 257, 8, 32, 64), (12, 256, 4, 32, 4), (1, 8, 2, 16, 2)]),
    # one strip (M <= 64) and several; k below and above 64 N
    "dpm_match_workspace_bytes": ("iiii", [(0, 64, 64, 32), (2, 64, 64, 0), (1, 1, 1, 1), (2, 64, 64, 32), (2, 65, 64, 32),
        (1, 257, 256, 2048), (3, 129, 3, 1000), (12, 256, 256, 256)]),
    # M <= 512 (no slabs), M > 512 (slabs), M N >= 2^18 (grid-wide top-k), with and without slabs; the slab count saturates at 64
    "dpm_pairing_workspace_bytes": ("iii", [(1, 1, 1), (2, 64, 64), (2, 257, 257), (2, 512, 64), (2, 513, 64), (2, 640, 64),
        (1, 512, 511), (1, 512, 512), (3, 512, 513), (2, 1024, 256), (1, 1025, 257), (1, 8193, 33),
        (12, 256, 256)]),
    "dpm_kabsch_workspace_bytes": ("ii", [(1, 1), (2, 64), (2, 65), (12, 256), (3, 257), (1, 4096)]),
    "dpm_preprocess_workspace_bytes": ("L", [(4096,), (4097,), (8191,), (8192,), (100001,), (1 << 22,), (257,)]),
    # rows for at least 1024 points
    "dpm_knn_self_workspace_bytes": ("i", [(0,), (1,), (300,), (1023,), (1024,), (1025,), (4097,), (100000,)]),
    "dpm_filter_dc_workspace_bytes": ("ii", [(0, 0), (-1, -1), (300, 8), (257, 8), (1024, 16), (1025, 16), (4097, 30), (60000, 63)]),
    "dpm_augment_workspace_bytes": ("iL", [(-1, 0), (0, -1), (0, 0), (200, 64), (200, 4096), (257, 4097), (4096, 4095), (4097, 100001),
        (120000, 1 << 22)]),
    "dpm_infomat_workspace_bytes": ("iii", [(1, 1, 1), (2, 257, 257), (1, 256, 4096), (3, 4097, 4097), (1, 300, 20000), (12, 16384, 16384)]),
    "dpm_icp_workspace_bytes": ("ii", [(0, 16), (2, 0), (1, 1), (2, 257), (3, 256), (1, 4097), (12, 16384)]),
    "dpm_voxel_map_workspace_bytes": ("L", [(0,), (1 << 31,), (1,), (257,), (1024,), (32769,), (1000001,)]),
    "dpm_reg_loss_workspace_bytes": ("iiii", [(0, 1, 1, 64), (70000, 1, 1, 64), (1, 1, 1, 1), (2, 65, 70, 64), (1, 257, 256, 128),
        (3, 64, 64, 192), (4, 256, 256, 256)]),
    "dpm_attention_train_workspace_bytes": ("iiii", [(0, 1, 1, 1), (1, 1, 1, 70000), (1, 1, 1, 1), (2, 65, 70, 1), (1, 257, 9, 4),
        (3, 64, 64, 8), (12, 256, 256, 4)]),
    # Cout in {32 .. 512}, K in {16, 32}; the partials' cap depends on the width
    "dpm_group_train_workspace_bytes": ("iiiii", [(1, 64, 16, 16, 48), (1, 64, 16, 8, 32), (0, 64, 16, 16, 32), (1, 64, 16, 16, 32),
        (2, 257, 65, 32, 64), (1, 8192, 2048, 16, 128), (2, 4097, 1025, 32, 256),
        (1, 100000, 512, 16, 512), (3, 1, 1, 16, 512)]),
    # E = 256 only; the forward's tiles against the backward's partial dW1
    "dpm_loop_pool_workspace_bytes": ("iii", [(2, 3, 128), (0, 3, 256), (2, 3, 256), (1, 1, 256), (1, 65, 256), (3, 257, 256),
        (64, 4097, 256), (1024, 1000, 256)]),
    # up to DT_SPLITS row tiles and beyond (the size is constant from there on)
    "dpm_dense_train_workspace_bytes": ("Lii", [(-1, 8, 32), (130, 0, 32), (0, 8, 32), (1, 1, 1), (130, 8, 32), (130, 8, 12), (257, 65, 33),
        (4097, 64, 256), (100000, 259, 128), (1 << 22, 512, 512)]),
    "dpm_cloud_nn_workspace_bytes": ("ii", [(-1, 0), (0, -1), (0, 0), (65, 300), (1, 257), (100000, 1), (3, 1000001)]),
    # one block up to 4096 points, at most 1024 blocks
    "dpm_distance_stats_workspace_bytes": ("iii", [(-1, 0, 0), (1, 1000, 0), (1, 0, 1000), (0, 0, 0), (4096, 2, 3), (4097, 2, 3), (257, 0, 1),
        (1 << 22, 4, 8), ((1 << 22) + 4097, 1, 0)]),
    # rows per block double while Q ceil(D / rpb) > 1024
    "dpm_scan_context_search_workspace_bytes": ("iii", [(0, 70, 2), (2, 0, 2), (2, 70, 0), (2, 70, 1000), (2, 70, 2), (1, 1, 1),
        (1, 4097, 10), (64, 257, 5), (257, 100000, 3), (1000, 1000000, 1)]),
}

PARENT = {
    "dpm_fps_workspace_bytes": [512, 532, 12512, 10792, 328192, 3246112, 5041968, 1902336, 9964032, 2621992, 2000512],
    "dpm_knn_workspace_bytes": [0, 0, 0, 103716, 189768, 189808, 460200, 935312, 4736688],
    "dpm_voxel_sampler_workspace_bytes": [0, 0, 0, 1536, 9216, 17408, 345088, 361216, 1835776, 1520896],
    "dpm_attention_split_workspace_bytes": [0, 0, 2432, 528, 212416, 17895680, 6684928, 2560],
    "dpm_match_workspace_bytes": [0, 0, 2048, 3072, 5120, 95232, 18432, 221696],
    "dpm_pairing_workspace_bytes": [272, 2304, 8480, 9472, 14864, 16896, 8440, 58912, 175736, 154432, 79736, 133680, 49408],
    "dpm_kabsch_workspace_bytes": [328, 9472, 9616, 221440, 55768, 295168],
    "dpm_preprocess_workspace_bytes": [17420, 17424, 33800, 33808, 401132, 16782344, 2060],
    "dpm_knn_self_workspace_bytes": [103716, 103716, 103716, 103716, 103716, 103736, 165176, 2083236],
    "dpm_filter_dc_workspace_bytes": [104192, 104192, 119040, 117248, 186112, 186880, 723456, 17363968],
    "dpm_augment_workspace_bytes": [0, 0, 1040, 2064, 66580, 66596, 66564, 1601156, 67114116],
    "dpm_infomat_workspace_bytes": [1053440, 2123008, 1184512, 3563008, 1701888, 19065088],
    "dpm_icp_workspace_bytes": [0, 0, 1049600, 2107648, 3160576, 1119232, 15931648],
    "dpm_voxel_map_workspace_bytes": [0, 0, 5632, 18432, 54528, 1652224, 50255104],
    "dpm_reg_loss_workspace_bytes": [0, 0, 15104, 87808, 284416, 313600, 2142464],
    "dpm_attention_train_workspace_bytes": [0, 0, 512, 1024, 4608, 6400, 49408],
    "dpm_group_train_workspace_bytes": [0, 0, 0, 8192, 203776, 2957568, 3067136, 3489280, 32000],
    "dpm_loop_pool_workspace_bytes": [0, 0, 263424, 263424, 526592, 3421440, 8421632, 16777472],
    "dpm_dense_train_workspace_bytes": [0, 0, 256, 512, 4608, 2048, 45312, 2654464, 4522240, 34668800],
    "dpm_cloud_nn_workspace_bytes": [0, 0, 8389136, 8393936, 8393248, 8389152, 24389152],
    "dpm_distance_stats_workspace_bytes": [0, 0, 0, 296, 448, 640, 304, 532736, 82176],
    "dpm_scan_context_search_workspace_bytes": [0, 0, 0, 0, 864, 12, 0, 34560, 3617532, 46884000],
}

CURSOR_SIZED = {"dpm_knn_workspace_bytes", "dpm_knn_self_workspace_bytes", "dpm_filter_dc_workspace_bytes"}
CURSOR_BOUND = 1280 + 5 * 255   # < 4 KiB


def _call(lib, name, args):
    f = getattr(lib, name)
    f.restype, f.argtypes = ctypes.c_size_t, [ctypes.c_longlong if t == "L" else ctypes.c_int for t in SHAPES[name][0]]
    return int(f(*args))


@pytest.fixture(scope="module")
def lib():
    from deeppointmap_amd import _lib
    from deeppointmap_amd.csrc import build
    build.build()
    return ctypes.CDLL(_lib.LIB_PATH)


def test_table_covers_every_size_entry_point():
    from deeppointmap_amd import _lib
    assert sorted(SHAPES) == sorted(n for n in _lib.SIGNATURES if n.endswith("_workspace_bytes"))
    assert sorted(PARENT) == sorted(SHAPES)
    for name, (types, shapes) in SHAPES.items():
        assert len(shapes) >= 6 and len(PARENT[name]) == len(shapes), name
        assert all(len(s) == len(types) for s in shapes), name


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_workspace_bytes_match_the_record(lib, name):
    for args, want in zip(SHAPES[name][1], PARENT[name]):
        got = _call(lib, name, args)
        if name in CURSOR_SIZED:
            assert (got == 0) == (want == 0) and abs(got - want) <= CURSOR_BOUND, (name, args, got, want)
        else:
            assert got == want, (name, args, got, want)


def test_cursor_check_program_compiles_and_runs(tmp_path):
    """tests/c/ws_cursor_check.cpp (its own main, csrc/workspace.h and nothing else) with the host compiler: for base residues
    0, 16, 80 and 255 mod 256 a carve never ends behind bytes() of the measuring run, rounded slices are 256-byte aligned,
    and without align_base the first slice is the caller's pointer"""
    import os
    import shutil
    import subprocess
    from conftest import ROOT
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("needs a host C++ compiler")
    exe = str(tmp_path / "ws_cursor_check")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "deeppointmap_amd", "csrc"),
                           os.path.join(ROOT, "tests", "c", "ws_cursor_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, (out.returncode, out.stdout, out.stderr)
    assert "ws cursor ok" in out.stdout
