"""Thin torch-tensor wrappers over the C ABI (include/dpm_hip.h).

torch provides device memory and the stream; every computation happens inside libdpm_hip.so.
Tensors must live on a ROCm device ("cuda" in torch terms); layouts are point-major fp32,
indices int32.  Nothing here falls back to torch math.
"""
from __future__ import annotations

from typing import Optional, Tuple

import ctypes
import threading
import weakref

import torch

from . import _lib, knobs

ACT_NONE, ACT_RELU, ACT_SIGMOID = 0, 1, 2


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else t.data_ptr()


def _stream(t: torch.Tensor):
    return torch.cuda.current_stream(t.device).cuda_stream


def _chk(t: torch.Tensor, dtype, name: str):
    if not t.is_cuda:
        raise _lib.DpmError(f"{name}: expected a tensor on the GPU, got {t.device} (no CPU fallback)")
    if t.dtype != dtype:
        raise TypeError(f"{name}: expected {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise ValueError(f"{name}: must be contiguous")
    return t


def prepare_points(points_cf: torch.Tensor, padding: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """(B,C,N) f32 + (B,N) bool -> xyz (B,N,3), lengths (B,) int32."""
    _chk(points_cf, torch.float32, "points")
    pad = _chk(padding.view(torch.uint8) if padding.dtype == torch.bool else padding, torch.uint8, "padding")  # same bytes
    B, C, N = points_cf.shape
    xyz = torch.empty(B, N, 3, device=points_cf.device, dtype=torch.float32)
    lengths = torch.empty(B, device=points_cf.device, dtype=torch.int32)
    lib = _lib.load()
    _lib.check(lib.dpm_prepare_points(_ptr(points_cf), _ptr(pad), B, C, N, _ptr(xyz), _ptr(lengths),
                                      _stream(xyz)), "dpm_prepare_points")
    return xyz, lengths


def emit_descriptors(xyz: torch.Tensor, fea: torch.Tensor, lengths: torch.Tensor, coor_scale: float = 0.0,
                     spare_frames: int = 0):
    """Point-major last level -> the encoder's return triple (coor (B,3,S), feat (B,C,S), padding (B,S) bool) and, with
    coor_scale > 0, the unified descriptor (B,C+3,S) = [feat ; coor * coor_scale] (odometry.py:47-49); one launch."""
    _chk(xyz, torch.float32, "xyz"), _chk(fea, torch.float32, "fea"), _chk(lengths, torch.int32, "lengths")
    B, S, C = fea.shape
    dev = xyz.device
    coor = torch.empty(B, 3, S, device=dev, dtype=torch.float32)
    feat = torch.empty(B, C, S, device=dev, dtype=torch.float32)
    padding = torch.empty(B, S, device=dev, dtype=torch.bool)
    # spare_frames: extra descriptor slots behind the B written ones (a neighbour rank's hand-over frame goes there)
    desc = torch.empty(B + spare_frames, C + 3, S, device=dev, dtype=torch.float32) if coor_scale > 0 else None
    _lib.check(_lib.load().dpm_emit_descriptors(_ptr(xyz), _ptr(fea), _ptr(lengths), B, S, C, float(coor_scale), _ptr(coor),
                                                _ptr(feat), _ptr(padding), _ptr(desc), _stream(xyz)), "dpm_emit_descriptors")
    return coor, feat, padding, desc


def nested_levels(xyz0: torch.Tensor, len0: torch.Tensor, npoints):
    """Levels below the first as prefixes of its picks: -> [(idx (B,K) int32, xyz (B,K,3), lengths (B,)) per K in npoints],
    views of three packed buffers written by one launch."""
    _chk(xyz0, torch.float32, "xyz0"), _chk(len0, torch.int32, "len0")
    B, K0, _ = xyz0.shape
    npoints = [int(k) for k in npoints]
    tot = B * sum(npoints)
    dev = xyz0.device
    xyz = torch.empty(tot, 3, device=dev, dtype=torch.float32)
    idx = torch.empty(tot, device=dev, dtype=torch.int32)
    lens = torch.empty(len(npoints), B, device=dev, dtype=torch.int32)
    arr = (ctypes.c_int32 * len(npoints))(*npoints)
    _lib.check(_lib.load().dpm_nested_levels(_ptr(xyz0), _ptr(len0), B, K0, len(npoints), ctypes.cast(arr, ctypes.c_void_p),
                                             _ptr(xyz), _ptr(idx), _ptr(lens), _stream(xyz0)), "dpm_nested_levels")
    out, off = [], 0
    for i, K in enumerate(npoints):
        out.append((idx[off:off + B * K].view(B, K), xyz[off:off + B * K].view(B, K, 3), lens[i]))
        off += B * K
    return out


def gather_frames(src: torch.Tensor, index: torch.Tensor, rows: int, cols: int, ld: int = None, frame_stride: int = None,
                  offset: int = 0) -> torch.Tensor:
    """out (n, rows, cols) = rows [0, rows) x columns [offset, offset + cols) of the frames index[p] of `src`
    (frames `frame_stride` floats apart, rows `ld` floats apart; defaults: packed)."""
    _chk(index, torch.int32, "index")
    if ld is None:
        _chk(src, torch.float32, "src")
    elif not src.is_cuda or src.dtype != torch.float32 or src.stride(-1) != 1:   # an explicit row stride: a row view
        raise ValueError("src: expected an fp32 GPU tensor with unit column stride")
    ld = cols if ld is None else ld
    frame_stride = rows * ld if frame_stride is None else frame_stride
    n = index.numel()
    out = torch.empty(n, rows, cols, device=src.device, dtype=torch.float32)
    base = src.data_ptr() + 4 * offset
    _lib.check(_lib.load().dpm_gather_frames(ctypes.c_void_p(base), frame_stride, rows, ld, cols, _ptr(index), n, _ptr(out),
                                             _stream(src)), "dpm_gather_frames")
    return out


def to_channel_first(x: torch.Tensor, row_multiple: int = 1) -> torch.Tensor:
    """(B,R,C) -> (B,C,R).  row_multiple > 1: the output rows are padded to a multiple of that many floats and the result
    is the (B,C,R) view of the padded buffer (row stride > R)."""
    _chk(x, torch.float32, "x")
    B, R, C = x.shape
    ldo = -(-R // row_multiple) * row_multiple
    out = torch.empty(B, C, ldo, device=x.device, dtype=torch.float32)
    _lib.check(_lib.load().dpm_to_channel_first_ld(_ptr(x), B, R, C, _ptr(out), ldo, _stream(x)), "dpm_to_channel_first")
    return out[:, :, :R] if ldo != R else out


def fps(xyz: torch.Tensor, lengths: torch.Tensor, K: int, algo: int = 0, start: Optional[torch.Tensor] = None):
    """xyz (B,N,3), lengths (B,) -> idx (B,K) int32 (-1 = padding), new_xyz (B,K,3), new_lengths (B,).
    start (B,) int32: first pick of every frame (`random_start_point`); None = point 0."""
    _chk(xyz, torch.float32, "xyz")
    _chk(lengths, torch.int32, "lengths")
    B, N, _ = xyz.shape
    lib = _lib.load()
    if start is not None:
        _chk(start, torch.int32, "start")
        if tuple(start.shape) != (B,):
            raise ValueError(f"start must have shape ({B},)")
        idx = torch.empty(B, K, device=xyz.device, dtype=torch.int32)
        new_xyz = torch.empty(B, K, 3, device=xyz.device, dtype=torch.float32)
        new_len = torch.empty(B, device=xyz.device, dtype=torch.int32)
        ws = torch.empty(lib.dpm_fps_workspace_bytes(B, N, K), device=xyz.device, dtype=torch.uint8)
        _lib.check(lib.dpm_fps_start(_ptr(xyz), _ptr(lengths), _ptr(start), B, N, K, _ptr(idx), _ptr(new_xyz), _ptr(new_len),
                                     _ptr(ws), _stream(xyz)), "dpm_fps_start")
        return idx, new_xyz, new_len
    if algo == 0 and N > 16384 and knobs.FPS_ALGO is not None:  # A/B runs (scripts/); never set from the environment here
        algo = int(knobs.FPS_ALGO)
    idx = torch.empty(B, K, device=xyz.device, dtype=torch.int32)
    new_xyz = torch.empty(B, K, 3, device=xyz.device, dtype=torch.float32)
    new_len = torch.empty(B, device=xyz.device, dtype=torch.int32)
    ws = torch.empty(lib.dpm_fps_workspace_bytes(B, N, K), device=xyz.device, dtype=torch.uint8)
    _lib.check(lib.dpm_fps_ex(_ptr(xyz), _ptr(lengths), B, N, K, _ptr(idx), _ptr(new_xyz), _ptr(new_len),
                              _ptr(ws), algo, _stream(xyz)), "dpm_fps")
    return idx, new_xyz, new_len


GRID_MIN_N = 1024  # dpm_knn_hybrid searches a grid from this many points per frame on


def knn_grid(points: torch.Tensor, lengths: torch.Tensor, radius: float) -> torch.Tensor:
    """The point-only half of knn_hybrid (N >= GRID_MIN_N): sorts every frame into the search grid of `radius`.
    Returns the workspace to hand to ONE knn_hybrid(..., grid=...) call with the same points, lengths and radius."""
    _chk(points, torch.float32, "points"), _chk(lengths, torch.int32, "lengths")
    B, N, _ = points.shape
    lib = _lib.load()
    ws = torch.empty(lib.dpm_knn_workspace_bytes(B, N), device=points.device, dtype=torch.uint8)
    _lib.check(lib.dpm_knn_build_grid(_ptr(points), _ptr(lengths), B, N, float(radius), _ptr(ws), _stream(points)),
               "dpm_knn_build_grid")
    return ws


def knn_hybrid(points: torch.Tensor, lengths: torch.Tensor, centers: torch.Tensor, K: int,
               radius: float, brute: bool = False, reuse_idx: Optional[torch.Tensor] = None,
               center_src: Optional[torch.Tensor] = None, grid: Optional[torch.Tensor] = None) -> torch.Tensor:
    """points (B,N,3), centers (B,S,3) -> idx (B,S,K) int32.  brute=True forces the all-pairs scan.
    reuse_idx (B,N,K) + center_src (B,S): centres that are points of the frame (center_src >= 0) copy their row of
    the already computed self-query (same radius, same K); only padded centres are searched.
    grid: knn_grid(points, lengths, radius) built ahead of time -- only the search runs."""
    _chk(points, torch.float32, "points")
    _chk(centers, torch.float32, "centers")
    _chk(lengths, torch.int32, "lengths")
    B, N, _ = points.shape
    S = centers.shape[1]
    idx = torch.empty(B, S, K, device=points.device, dtype=torch.int32)
    lib = _lib.load()
    if grid is not None:
        if brute or reuse_idx is not None or grid.numel() != lib.dpm_knn_workspace_bytes(B, N):
            raise ValueError("grid= goes with a plain grid search of the (B, N) it was built for")
        _lib.check(lib.dpm_knn_hybrid_prebuilt(_ptr(points), _ptr(lengths), _ptr(centers), B, N, S, K, float(radius),
                                               _ptr(idx), _ptr(grid), _stream(points)), "dpm_knn_hybrid_prebuilt")
        return idx
    nbytes = 0 if brute else lib.dpm_knn_workspace_bytes(B, N)
    ws = torch.empty(nbytes, device=points.device, dtype=torch.uint8) if nbytes else None
    if reuse_idx is not None:
        _chk(reuse_idx, torch.int32, "reuse_idx"), _chk(center_src, torch.int32, "center_src")
        if tuple(reuse_idx.shape) != (B, N, K) or tuple(center_src.shape) != (B, S):
            raise ValueError("reuse_idx must be (B,N,K) and center_src (B,S)")
    _lib.check(lib.dpm_knn_hybrid_reuse(_ptr(points), _ptr(lengths), _ptr(centers), B, N, S, K, float(radius),
                                        _ptr(idx), _ptr(ws), _ptr(reuse_idx), _ptr(center_src), _stream(points)),
               "dpm_knn_hybrid")
    return idx


def knn_grid_census(grid: torch.Tensor, B: int, N: int) -> dict:
    """What the last knn_grid + knn_hybrid(..., grid=grid) on this workspace did (tests, debugging; one host read):
    {"frames": B dicts of the grid header (lox, loy, inv_cs, g, err2, H, h), "tie": tied rows offered to the tie queue,
    "todo": rows the fast search left to the full search}."""
    lib = _lib.load()
    if grid.dtype != torch.uint8 or not grid.is_cuda or grid.numel() != lib.dpm_knn_workspace_bytes(B, N) or N < GRID_MIN_N:
        raise ValueError("grid must be the knn_grid workspace of the (B, N) given")
    out = torch.empty(8 * B + 2, device=grid.device, dtype=torch.int32)
    _lib.check(lib.dpm_knn_debug_census(_ptr(grid), B, N, _ptr(out), _stream(grid)), "dpm_knn_debug_census")
    words = out.cpu()
    hdr_i, hdr_f = words[:8 * B].view(B, 8), words[:8 * B].view(torch.float32).view(B, 8)
    frames = [dict(lox=float(hdr_f[b, 0]), loy=float(hdr_f[b, 1]), inv_cs=float(hdr_f[b, 2]), g=int(hdr_i[b, 3]),
                   err2=float(hdr_f[b, 4]), H=int(hdr_i[b, 5]), h=int(hdr_i[b, 6])) for b in range(B)]
    return dict(frames=frames, tie=int(words[8 * B]), todo=int(words[8 * B + 1]))


def ball_query(points: torch.Tensor, lengths: torch.Tensor, centers: torch.Tensor, K: int, radius: float) -> torch.Tensor:
    """points (B,N,3), centers (B,S,3) -> idx (B,S,K) int32: first K indices within the radius, padded with the first."""
    _chk(points, torch.float32, "points"), _chk(centers, torch.float32, "centers"), _chk(lengths, torch.int32, "lengths")
    B, N, _ = points.shape
    S = centers.shape[1]
    idx = torch.empty(B, S, K, device=points.device, dtype=torch.int32)
    _lib.check(_lib.load().dpm_ball_query(_ptr(points), _ptr(lengths), _ptr(centers), B, N, S, K, float(radius),
                                          _ptr(idx), _stream(points)), "dpm_ball_query")
    return idx


VOXEL_SAMPLER_MAX_CELLS = 1 << 28   # 3 GB of grid per frame; finer grids than that are refused
VOXEL_SAMPLER_MAX_WORKSPACE = 64 << 30   # ... and so is a batch whose grids together exceed 64 GiB


def voxel_sample(points: torch.Tensor, padding: torch.Tensor, K: Optional[int], voxel_size: float = 0.3,
                 sample_range: float = 1.0):
    """Sampler.voxel (utils.py:150-207): points (B,N,D) float32, padding (B,N) bool -> (sel (B,cap) int32 original
    indices in the reference's output order, -1 = padding; n_unique (B,) int32 occupied voxels).  cap = K, or the number
    of occupied voxels for K=None (B must be 1 then, as in the reference).  One host read of the grid sizes (the
    reference walks every frame on the host), a second one for K=None."""
    _chk(points, torch.float32, "points")
    if padding.dtype != torch.bool or tuple(padding.shape) != tuple(points.shape[:2]):
        raise ValueError("points_padding must be a (B,N) bool tensor")
    B, N, D = points.shape
    if K is None and B != 1:
        raise ValueError("K=None takes one frame (utils.py:200)")
    lib, dev, st = _lib.load(), points.device, _stream(points)
    pad = padding.contiguous().view(torch.uint8)
    hdr = torch.empty(B, 8, device=dev, dtype=torch.float32)
    _lib.check(lib.dpm_voxel_sampler_bounds(_ptr(points), _ptr(pad), B, N, D, float(voxel_size), float(sample_range),
                                            _ptr(hdr), st), "dpm_voxel_sampler_bounds")
    dims = hdr[:, 3:6].double().cpu()
    if not bool(torch.isfinite(dims).all()):
        raise ValueError("voxel sampler: the frame's bounding box is not finite")
    cells = int(dims.prod(1).max().item())
    if cells > VOXEL_SAMPLER_MAX_CELLS:
        raise ValueError(f"voxel sampler: {cells} grid cells per frame exceed {VOXEL_SAMPLER_MAX_CELLS}")
    ws_bytes = lib.dpm_voxel_sampler_workspace_bytes(B, N, cells)
    if ws_bytes > VOXEL_SAMPLER_MAX_WORKSPACE:
        raise ValueError(f"voxel sampler: {B} frames x {cells} grid cells need {ws_bytes >> 20} MiB of grid "
                         f"(limit {VOXEL_SAMPLER_MAX_WORKSPACE >> 20} MiB): sample fewer frames per call or use a coarser grid")
    ws = torch.empty(ws_bytes, device=dev, dtype=torch.uint8)
    cap = N if K is None else int(K)
    sel = torch.empty(B, cap, device=dev, dtype=torch.int32)
    n_unique = torch.empty(B, device=dev, dtype=torch.int32)
    _lib.check(lib.dpm_voxel_sampler_select(_ptr(points), _ptr(pad), B, N, D, float(voxel_size), float(sample_range),
                                            _ptr(hdr), cells, -1 if K is None else int(K), _ptr(sel), cap,
                                            _ptr(n_unique), _ptr(ws), st), "dpm_voxel_sampler_select")
    if K is None:
        sel = sel[:, :int(n_unique[0].item())]
    return sel, n_unique


PROJECTED_COUT = (32, 64, 128, 256, 512)

# Tensors derived from weights alone (a packed copy of weight columns, the product of two weight matrices) are
# made once per weight version, not once per call.  An entry belongs to the very tensor OBJECTS it was made from
# (weak references: a freed weight whose address is reused cannot alias it) at their storage address and in-place
# version, so load_state_dict / .to() / optimiser steps invalidate it.  Callers pass the parameter tensors
# themselves, not views made per call.
_DERIVED: dict = {}
_DERIVED_LOCK = threading.Lock()   # the reference drives one Encoder / Decoder from several threads (core.py:54-57)
_RETIRED: list = []                # replaced values stay alive until the device has been synchronised once more
_GENERATION = [0]                  # bumped by invalidate_derived(): captured graphs made before it are stale (decoder.py)


def invalidate_derived() -> None:
    """Forget every tensor derived from weights.  load_state_dict() calls it (ParamTree); call it yourself after editing
    weights through `.data` (which does not bump the version counter the cache keys on)."""
    with _DERIVED_LOCK:
        _RETIRED.extend(v[2] for v in _DERIVED.values())
        _DERIVED.clear()
        _GENERATION[0] += 1


def derived_generation() -> int:
    return _GENERATION[0]


def _derived(tag: str, sources, make):
    key = (tag,) + tuple(id(t) for t in sources)
    stamp = tuple((t.data_ptr(), t._version) for t in sources)
    dev = sources[0].device
    cur = torch.cuda.current_stream(dev)
    if torch.cuda.is_current_stream_capturing():
        # Inside a capture the cache is read-only: a tensor MADE here would live in the graph's private pool, hold no data
        # until the first replay and be published to eager callers with a captured event; and a hit must not make the
        # capture wait on an event recorded outside it -- it has to be complete already (Decoder captures a shape only after
        # eager calls of the same shape, which made every derived tensor of the path long before).
        with _DERIVED_LOCK:
            hit = _DERIVED.get(key)
            if hit is not None and hit[1] == stamp and all(r() is t for r, t in zip(hit[0], sources)) and hit[3].query():
                return hit[2]
        raise RuntimeError(f"ops._derived({tag!r}) under stream capture: make weight-derived tensors before capturing")
    with _DERIVED_LOCK:
        hit = _DERIVED.get(key)
        if hit is not None and hit[1] == stamp and all(r() is t for r, t in zip(hit[0], sources)):
            cur.wait_event(hit[3])       # made on another stream, possibly moments ago
            for v in (hit[2] if isinstance(hit[2], (tuple, list)) else (hit[2],)):
                v.record_stream(cur)     # ... and read on this one: the allocator must not recycle it under the reader
            return hit[2]
        if len(_RETIRED) > 64:           # rare: bounded by a device sync, after which nothing can still read them
            torch.cuda.synchronize(dev)
            _RETIRED.clear()
        if hit is not None:
            _RETIRED.append(hit[2])
        if len(_DERIVED) >= 512:
            # entries of weights that no longer exist go first (models re-created, ad-hoc weights); nothing can still read them
            # through a captured graph, whose owner holds its weights.  If live entries have to go as well, captured graphs
            # that replay kernels reading them are stale: the generation they were stamped with ends here (decoder.py).
            dead = [k for k, v in _DERIVED.items() if any(r() is None for r in v[0])]
            for k in dead:
                _RETIRED.append(_DERIVED.pop(k)[2])
            if len(_DERIVED) >= 512:
                _RETIRED.extend(v[2] for v in _DERIVED.values())
                _DERIVED.clear()
                _GENERATION[0] += 1
        value = make()
        _DERIVED[key] = (tuple(weakref.ref(t) for t in sources), stamp, value, cur.record_event())
        return value


def _centre_rows(M: torch.Tensor) -> torch.Tensor:
    """(Cout, n) -> the same with every column's mean over the Cout rows removed (fp64 arithmetic, fp32 result, contiguous)"""
    Md = M.double()
    return (Md - Md.mean(0, keepdim=True)).float().contiguous()


def _gamma_sign(gamma: torch.Tensor) -> torch.Tensor:
    """(Cout, 1): +1 where gamma >= 0, -1 where gamma < 0"""
    return torch.where(gamma < 0, -torch.ones_like(gamma), torch.ones_like(gamma)).reshape(-1, 1)


def _centred_layer(W2: torch.Tensor, bias: torch.Tensor, gamma: torch.Tensor, Cin: int):
    """diag(sign gamma) (I - 11^T / Cout) applied to a grouping layer (csrc/group_mlp.hip, CENTRED):
    -> (W_f (Cout,Cin), W_r (Cout,3), bias (Cout)): zero mean over Cout, then channel c times sign(gamma_c)"""
    sg = _gamma_sign(gamma)
    Wc = _centre_rows(W2) * sg
    return Wc[:, :Cin].contiguous(), Wc[:, Cin:].contiguous(), (_centre_rows(bias.reshape(-1, 1)) * sg).reshape(-1).contiguous()


def group_mlp_max(xyz, fea, centers, idx, W, bias, gamma, beta, radius: float, generic: bool = False,
                  fused: bool = False) -> torch.Tensor:
    """xyz (B,N,3), fea (B,N,Cin), centers (B,S,3), idx (B,S,K), W (Cout,Cin+3[,1,1]) -> (B,S,Cout).
    Default: project before gather (P = fea W_f^T + b once per point with the MFMA GEMM, then gather + relative
    coordinates + LayerNorm + max).  fused=True: the one-kernel gather-GEMM path; generic=True: the plain-VALU
    kernel (cross-check paths, and the fallback for layer widths the projected path does not cover)."""
    for n, t in (("xyz", xyz), ("fea", fea), ("centers", centers), ("W", W), ("bias", bias),
                 ("gamma", gamma), ("beta", beta)):
        _chk(t, torch.float32, n)
    _chk(idx, torch.int32, "idx")
    B, N, Cin = fea.shape
    S, K = idx.shape[1], idx.shape[2]
    Cout = W.shape[0]
    if W.shape[1] != Cin + 3:
        raise ValueError(f"W must be (Cout, Cin+3) = ({Cout}, {Cin + 3}), got {tuple(W.shape)}")
    out = torch.empty(B, S, Cout, device=fea.device, dtype=torch.float32)
    lib = _lib.load()
    if not generic and not fused and Cout in PROJECTED_COUT:
        W2 = W.reshape(Cout, Cin + 3)
        # a packed copy of the feature columns (rows of the Conv2d weight are Cin+3 floats: not 16-byte aligned)
        Wf = _derived("feature-columns", (W,), lambda: W2[:, :Cin].contiguous())
        if knobs.FOLD_GATHER and knobs.GEMM_BF16X3 and Cin % 32 == 0 and Cin <= knobs.BF16X3_MAX_K and radius >= knobs.FOLD_MIN_RADIUS:
            # folded form (csrc/group_mlp.hip, FOLD): the projection's epilogue adds the POINT half of the relative-coordinate
            # term, the gather subtracts the centre half and reads no coordinates.  A property of the layer (its widths and the
            # tensors' layout class), never of the row count.
            if knobs.CENTRED_GATHER:
                # LayerNorm's mean removal moved into the layer: (I - 11^T / Cout) applied to the weight and the bias (fp64, once per
                # weight version), every projected row and centre term then has zero mean over its channels by construction
                Wfc, Wrc, bc = _derived("centred-layer", (W, bias, gamma), lambda: _centred_layer(W2, bias, gamma, Cin))
                P = linear_bf16x3(fea.reshape(B * N, Cin), Wfc, bc, rank3=(xyz.reshape(B * N, 3), Wrc.data_ptr(), 3, 1.0 / float(radius)))
                if P is not None:
                    _lib.check(lib.dpm_group_gather_ln_max_centred(_ptr(P), _ptr(centers), _ptr(idx), _ptr(Wrc), 3, _ptr(gamma), _ptr(beta),
                                                                   B, N, S, K, Cout, float(radius), _ptr(out), _stream(fea)),
                               "dpm_group_gather_ln_max_centred")
                    return out
            P = linear_bf16x3(fea.reshape(B * N, Cin), Wf, bias,
                              rank3=(xyz.reshape(B * N, 3), W2.data_ptr() + 4 * Cin, Cin + 3, 1.0 / float(radius)))
            if P is not None:
                _lib.check(lib.dpm_group_gather_ln_max_folded(_ptr(P), _ptr(centers), _ptr(idx), W2.data_ptr() + 4 * Cin, Cin + 3,
                                                              _ptr(gamma), _ptr(beta), B, N, S, K, Cout, float(radius), _ptr(out),
                                                              _stream(fea)), "dpm_group_gather_ln_max_folded")
                return out
        P = linear(fea.reshape(B * N, Cin), Wf, bias)
        _lib.check(lib.dpm_group_gather_ln_max(_ptr(P), _ptr(xyz), _ptr(centers), _ptr(idx), W2.data_ptr() + 4 * Cin,
                                               Cin + 3, _ptr(gamma), _ptr(beta), B, N, S, K, Cout, float(radius),
                                               _ptr(out), _stream(fea)), "dpm_group_gather_ln_max")
        return out
    fn = lib.dpm_group_mlp_max_generic if generic else lib.dpm_group_mlp_max
    _lib.check(fn(_ptr(xyz), _ptr(fea), _ptr(centers), _ptr(idx), _ptr(W), _ptr(bias), _ptr(gamma), _ptr(beta),
                  B, N, S, K, Cin, Cout, float(radius), _ptr(out), _stream(fea)), "dpm_group_mlp_max")
    return out


def group_mlp_max_from_xyz(xyz, W0, b0, centers, idx, W, bias, gamma, beta, radius: float,
                           fused: bool = False) -> torch.Tensor:
    """First-stage SetAbstraction with the per-point input MLP (W0 (Cin,3[,1]), b0 (Cin)) folded into the gather:
    xyz (B,N,3), centers (B,S,3), idx (B,S,K), W (Cout,Cin+3[,1,1]) -> (B,S,Cout).  Raises ValueError for
    shapes the kernels do not cover (callers fall back to linear + group_mlp_max).
    Default: the projected point feature is affine in the point, P = (W_f W0) xyz + (W_f b0 + b); the two small
    weight products are made with the GEMM and the kernel evaluates P on the fly.  fused=True: the gather-GEMM kernel
    that evaluates the 16 input features per neighbour."""
    for n, t in (("xyz", xyz), ("W0", W0), ("b0", b0), ("centers", centers), ("W", W), ("bias", bias),
                 ("gamma", gamma), ("beta", beta)):
        _chk(t, torch.float32, n)
    _chk(idx, torch.int32, "idx")
    B, N, _ = xyz.shape
    S, K = idx.shape[1], idx.shape[2]
    Cin, Cout = W0.shape[0], W.shape[0]
    if W0.shape[1] != 3 or W.shape[1] != Cin + 3:
        raise ValueError("W0 must be (Cin,3) and W (Cout,Cin+3)")
    out = torch.empty(B, S, Cout, device=xyz.device, dtype=torch.float32)
    if not fused and Cout in (32, 64, 128):
        W2 = W.reshape(Cout, Cin + 3)
        A, cvec = _derived("affine-stage0", (W, W0, b0, bias), lambda: (
            linear(W2[:, :Cin], W0.reshape(Cin, 3).t().contiguous(), exact=True),                     # (Cout,3) = W_f W0
            linear(W2[:, :Cin], b0.reshape(1, Cin), residual=bias.reshape(Cout, 1), exact=True)))     # (Cout,1) = W_f b0 + b
        if knobs.CENTRED_GATHER and knobs.FOLD_GATHER:
            Ac, cc, Wrc = _derived("affine-stage0-centred", (W, W0, b0, bias, gamma), lambda: (
                (_centre_rows(A) * _gamma_sign(gamma)).contiguous(),
                (_centre_rows(cvec.reshape(Cout, 1)) * _gamma_sign(gamma)).reshape(Cout).contiguous(),
                (_centre_rows(W2[:, Cin:]) * _gamma_sign(gamma)).contiguous()))
            _lib.check(_lib.load().dpm_group_affine_ln_max_centred(_ptr(Ac), _ptr(cc), _ptr(xyz), _ptr(centers), _ptr(idx), _ptr(Wrc), 3,
                                                                   _ptr(gamma), _ptr(beta), B, N, S, K, Cout, float(radius),
                                                                   _ptr(out), _stream(xyz)), "dpm_group_affine_ln_max_centred")
            return out
        _lib.check(_lib.load().dpm_group_affine_ln_max(_ptr(A), _ptr(cvec), _ptr(xyz), _ptr(centers), _ptr(idx),
                                                       W2.data_ptr() + 4 * Cin, Cin + 3, _ptr(gamma), _ptr(beta), B, N, S,
                                                       K, Cout, float(radius), _ptr(out), _stream(xyz)),
                   "dpm_group_affine_ln_max")
        return out
    _lib.check(_lib.load().dpm_group_mlp_max_from_xyz(_ptr(xyz), _ptr(W0), _ptr(b0), _ptr(centers), _ptr(idx), _ptr(W),
                                                      _ptr(bias), _ptr(gamma), _ptr(beta), B, N, S, K, Cin, Cout,
                                                      float(radius), _ptr(out), _stream(xyz)),
               "dpm_group_mlp_max_from_xyz")
    return out




def linear(x: torch.Tensor, W: torch.Tensor, bias: Optional[torch.Tensor] = None, act: int = ACT_NONE,
           residual: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None, exact: bool = False) -> torch.Tensor:
    """x (..., Cin) (last dim contiguous rows), W (Cout, Cin[,1[,1]]) -> (..., Cout).

    `out` may be a column slice of a wider row-major buffer (its row stride is honoured).
    Which of the two GEMM kernels runs is a property of the LAYER (its Cin, Cout and the `exact` request), never of the row
    count: a frame's result does not depend on the batch it travels in.  exact=True: the fp32-MFMA kernel (callers whose
    result must equal another kernel's bit for bit: linear_layernorm's two-kernel form against its fused form)."""
    if W.dtype != torch.float32 or not W.is_cuda:
        raise ValueError("W must be an fp32 GPU tensor")
    Cout, Cin = W.shape[0], W.shape[1]
    if knobs.GEMM_BF16X3 and not exact and Cin % 32 == 0 and Cin <= knobs.BF16X3_MAX_K and Cout % 4 == 0 and W.numel() == Cout * Cin:
        done = linear_bf16x3(x, W, bias, act, residual, out)
        if done is not None:
            return done
    if W.dim() == 2 and W.stride(1) == 1 and W.stride(0) >= Cin:
        ldw = W.stride(0)      # a column range of a wider weight matrix (e.g. the feature columns of a Conv2d weight)
    else:
        _chk(W, torch.float32, "W")
        ldw = Cin
    if x.dtype != torch.float32 or not x.is_cuda or x.stride(-1) != 1:
        raise ValueError("x must be an fp32 GPU tensor with unit stride in the last dimension")
    x2 = x.reshape(-1, x.shape[-1]) if x.is_contiguous() else x
    if x2.dim() != 2:
        raise ValueError("non-contiguous x must be 2-D")
    R = x2.shape[0]
    if out is None:
        out = torch.empty(*x.shape[:-1], Cout, device=x.device, dtype=torch.float32)
    o2 = out.reshape(-1, Cout) if out.is_contiguous() else out
    if o2.dim() != 2 or o2.stride(1) != 1:
        raise ValueError("out must be 2-D with unit column stride")
    r2 = None
    if residual is not None:
        r2 = residual.reshape(-1, Cout)
        _chk(r2, torch.float32, "residual")
    _lib.check(_lib.load().dpm_linear(_ptr(x2), x2.stride(0), _ptr(W), ldw, _ptr(bias), _ptr(r2),
                                      Cout if r2 is not None else 0, _ptr(o2), o2.stride(0), R, Cin, Cout, act,
                                      _stream(x)), "dpm_linear")
    return out


def _weight_planes(W: torch.Tensor):
    """The three bf16 planes (hi | mid | lo, csrc/gemm_b3.hip) of the PARAMETER a weight (view) belongs to, made once per
    weight version, and where W's first row sits in them: -> (planes (3, n) int16, element offset, plane stride n), or None
    when W is not a block of whole rows of a contiguous fp32 tensor."""
    base = W._base if W._base is not None else W
    Cin = W.shape[1]
    W2 = W if W.dim() == 2 else W.reshape(W.shape[0], Cin)
    if (base.dtype != torch.float32 or not base.is_cuda or not base.is_contiguous() or W2.stride(1) != 1 or
            W2.stride(0) != Cin or base.numel() % 8 != 0):
        return None
    off = W2.storage_offset() - base.storage_offset()
    if off < 0 or off + W2.numel() > base.numel():
        return None

    def make():
        planes = torch.empty(3, base.numel(), device=base.device, dtype=torch.int16)
        _lib.check(_lib.load().dpm_split_bf16x3(_ptr(base), base.numel(), _ptr(planes), _stream(base)), "dpm_split_bf16x3")
        return planes
    return _derived("bf16x3-planes", (base,), make), off, base.numel()


def linear_bf16x3(x: torch.Tensor, W: torch.Tensor, bias: Optional[torch.Tensor] = None, act: int = ACT_NONE,
                  residual: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None, rank3=None) -> Optional[torch.Tensor]:
    """linear() on the bf16 matrix pipe: every fp32 operand split exactly into three bf16 terms, six term products
    accumulated in fp32 (csrc/gemm_b3.hip; fp32-accumulation accuracy, not the fp32 kernel's bits).  Returns None when the
    shape / layout is not covered (the caller runs linear())."""
    Cout, Cin = W.shape[0], W.shape[1]
    if Cin % 32 != 0 or Cout % 4 != 0 or x.dtype != torch.float32 or not x.is_cuda or x.stride(-1) != 1:
        return None
    if bias is not None and bias.data_ptr() % 16:
        return None
    wp = _weight_planes(W)
    if wp is None:
        return None
    planes, off, n = wp
    x2 = x.reshape(-1, x.shape[-1]) if x.is_contiguous() else x
    if x2.dim() != 2:
        return None
    if out is None:
        out = torch.empty(*x.shape[:-1], Cout, device=x.device, dtype=torch.float32)
    o2 = out.reshape(-1, Cout) if out.is_contiguous() else out
    r2 = None
    if residual is not None:
        r2 = residual.reshape(-1, Cout)
        _chk(r2, torch.float32, "residual")
    if rank3 is not None:
        # rank3 = (x3 (R,3) contiguous fp32, address of w3[0, 0], its row stride in floats, scale): out += scale * x3 w3^T in the
        # epilogue (the point half of a grouping layer's relative-coordinate term: group_mlp_max)
        x3, w3_ptr, ldw3, scale = rank3
        _chk(x3, torch.float32, "x3")
        if tuple(x3.shape) != (x2.shape[0], 3):
            raise ValueError("rank3 rows must be (R, 3)")
        st = _lib.load().dpm_linear_bf16x3_rank3(_ptr(x2), x2.stride(0), planes.data_ptr() + 2 * off, Cin, n, _ptr(bias), _ptr(r2),
                                                 Cout if r2 is not None else 0, _ptr(o2), o2.stride(0), x2.shape[0], Cin, Cout, act,
                                                 _ptr(x3), ctypes.c_void_p(w3_ptr), int(ldw3), float(scale), _stream(x))
    else:
        st = _lib.load().dpm_linear_bf16x3(_ptr(x2), x2.stride(0), planes.data_ptr() + 2 * off, Cin, n, _ptr(bias), _ptr(r2),
                                           Cout if r2 is not None else 0, _ptr(o2), o2.stride(0), x2.shape[0], Cin, Cout, act,
                                           _stream(x))
    if st == -2:
        return None
    _lib.check(st, "dpm_linear_bf16x3")
    return out


def similarity_batched(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """a (B,M,C), b (B,N,C) contiguous -> S (B,M,N) with S[p] = a[p] @ b[p]^T (fp32 MFMA)."""
    _chk(a, torch.float32, "a"), _chk(b, torch.float32, "b")
    B, M, C = a.shape
    N = b.shape[1]
    out = torch.empty(B, M, N, device=a.device, dtype=torch.float32)
    _lib.check(_lib.load().dpm_linear_batched(_ptr(a), C, M * C, _ptr(b), C, N * C, None, None, 0, 0, _ptr(out), N,
                                              M * N, B, M, C, N, ACT_NONE, _stream(a)), "dpm_linear_batched")
    return out


def layernorm(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, act: int = ACT_NONE,
              pre: Optional[torch.Tensor] = None, post: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out = act(LN(x + pre) * gamma + beta + post) over the last dimension."""
    _chk(x, torch.float32, "x")
    C = x.shape[-1]
    x2 = x.reshape(-1, C)
    out = torch.empty_like(x)
    for n, t in (("pre", pre), ("post", post)):
        if t is not None:
            _chk(t, torch.float32, n)
            if t.numel() != x.numel():
                raise ValueError(f"{n} must have the shape of x")
    _lib.check(_lib.load().dpm_layernorm(_ptr(x2), C, _ptr(pre), _ptr(gamma), _ptr(beta), _ptr(post), _ptr(out), C,
                                         x2.shape[0], C, act, _stream(x)), "dpm_layernorm")
    return out


FUSED_LN_WIDTHS = (32, 64, 128, 256)  # dpm_linear_layernorm: the output row must fit one workgroup's tile
FUSED_LN_MIN_ROWS = 16384             # ... and there must be a workgroup (64 rows) for every compute unit


def linear_layernorm(x: torch.Tensor, W: torch.Tensor, bias: Optional[torch.Tensor], gamma: torch.Tensor, beta: torch.Tensor,
                     act: int = ACT_NONE, pre: Optional[torch.Tensor] = None, post: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out = act(LN(x W^T + bias + pre) * gamma + beta + post): Conv1d(k=1)/Linear + LayerNorm1d in one kernel when the
    output width is one of FUSED_LN_WIDTHS, otherwise the GEMM kernel followed by the LayerNorm kernel (same result up
    to the summation order of the row statistics)."""
    Cout, Cin = W.shape[0], W.shape[1]
    x2 = x.reshape(-1, x.shape[-1])
    # Layers the bf16x3 kernel covers (a property of the layer: K <= 512 in whole K-tiles, whole weight rows) take it in BOTH forms
    # -- fused from FUSED_LN_MIN_ROWS rows on, GEMM + LayerNorm below -- with identical rows either way
    # (from K = 128 on: with shorter reductions the kernels are bound by their epilogues and the fp32 form's smaller row tiles win)
    if (knobs.GEMM_BF16X3 and knobs.GEMM_LN_BF16X3 and Cin % 32 == 0 and knobs.BF16X3_LN_MIN_K <= Cin <= knobs.BF16X3_MAX_K and Cout % 4 == 0 and W.numel() == Cout * Cin
            and x.dtype == torch.float32):
        wp = _weight_planes(W)
        if wp is not None and (bias is None or bias.data_ptr() % 16 == 0):
            if (Cout in FUSED_LN_WIDTHS and (x2.shape[0] >= FUSED_LN_MIN_ROWS or x2.shape[0] <= knobs.FUSED_LN_SMALL_ROWS)
                    and x2.is_contiguous() and knobs.FUSED_LN):
                planes, off, n = wp
                out = torch.empty(*x.shape[:-1], Cout, device=x.device, dtype=torch.float32)
                for nm, t in (("pre", pre), ("post", post)):
                    if t is not None:
                        _chk(t, torch.float32, nm)
                        if t.numel() != out.numel():
                            raise ValueError(f"{nm} must have the shape of the output")
                st = _lib.load().dpm_linear_layernorm_bf16x3(_ptr(x2), x2.stride(0), planes.data_ptr() + 2 * off, Cin, n, _ptr(bias),
                                                             _ptr(pre), _ptr(gamma), _ptr(beta), _ptr(post), _ptr(out), Cout,
                                                             x2.shape[0], Cin, Cout, act, _stream(x))
                if st == 0:
                    return out
                if st != -2:
                    _lib.check(st, "dpm_linear_layernorm_bf16x3")
            y = linear_bf16x3(x, W, bias, residual=pre)
            if y is not None:
                return layernorm(y, gamma, beta, act=act, post=post)
    # the fused kernel owns whole output rows (64 rows per workgroup): below FUSED_LN_MIN_ROWS it leaves most of the 256
    # compute units idle and the two-kernel form is 1.5-2.8x faster (scripts/gemm_ln_shapes.py: 4096 x 1024 -> 256 takes
    # 86 us fused, 31 us as GEMM + LayerNorm)
    if (Cout in FUSED_LN_WIDTHS and x2.shape[0] >= FUSED_LN_MIN_ROWS and W.is_contiguous() and x2.is_contiguous()
            and x.dtype == torch.float32 and Cin % 4 == 0 and knobs.FUSED_LN):
        _chk(W, torch.float32, "W")
        out = torch.empty(*x.shape[:-1], Cout, device=x.device, dtype=torch.float32)
        for n, t in (("pre", pre), ("post", post)):
            if t is not None:
                _chk(t, torch.float32, n)
                if t.numel() != out.numel():
                    raise ValueError(f"{n} must have the shape of the output")
        st = _lib.load().dpm_linear_layernorm(_ptr(x2), x2.stride(0), _ptr(W), Cin, _ptr(bias), _ptr(pre), _ptr(gamma),
                                              _ptr(beta), _ptr(post), _ptr(out), Cout, x2.shape[0], Cin, Cout, act, _stream(x))
        if st == 0:
            return out
        if st != -2:  # anything but "unsupported shape"
            _lib.check(st, "dpm_linear_layernorm")
    y = linear(x, W, bias, residual=pre, exact=True)   # the fused kernel's arithmetic: same bits in either form
    return layernorm(y, gamma, beta, act=act, post=post)


def _pwconv_kperm() -> torch.Tensor:
    """stored column -> original column of W2 for dpm_pwconv_pair_bf16x3 (include/dpm_hip.h): 32 s + 8 g + e <- 16 (2 s + (e >> 2)) + 4 g + (e & 3)"""
    return torch.tensor([16 * (2 * s + (e >> 2)) + 4 * g + (e & 3) for s in range(4) for g in range(4) for e in range(8)], dtype=torch.long)


def pwconv_pair(x: torch.Tensor, W1, b1, g1, be1, W2, b2, g2, be2, post: Optional[torch.Tensor]) -> Optional[torch.Tensor]:
    """relu(LN2(relu(LN1(x W1^T + b1)) W2^T + b2) + post) in one kernel (InvResMLP's pw_conv pair, C = 32 only: csrc/gemm_b3.hip,
    pwconv_pair_b3_kernel).  None when the layer / layout is not covered: the caller runs two linear_layernorm calls -- for EVERY
    call of that layer (the decision depends on the layer's shape and the tensors' layout class, never on the row count)."""
    C, H = W1.shape[1], W1.shape[0]
    if not (knobs.FUSED_PWCONV and knobs.GEMM_BF16X3 and C == 32 and H == 128 and tuple(W2.shape[:2]) == (C, H) and x.is_cuda
            and x.dtype == torch.float32 and x.is_contiguous() and W1.numel() == C * H and W2.numel() == C * H):
        return None
    wp1 = _weight_planes(W1)
    if wp1 is None or (post is not None and (not post.is_contiguous() or post.numel() != x.numel())):
        return None
    for n, t_ in (("gamma1", g1), ("beta1", be1), ("gamma2", g2), ("beta2", be2)):
        _chk(t_, torch.float32, n)

    def make():
        Wp = W2.reshape(C, H)[:, _pwconv_kperm().to(W2.device)].contiguous()
        planes = torch.empty(3, C * H, device=W2.device, dtype=torch.int16)
        _lib.check(_lib.load().dpm_split_bf16x3(_ptr(Wp), C * H, _ptr(planes), _stream(W2)), "dpm_split_bf16x3")
        planes._dpm_keep = Wp   # (the split kernel reads it asynchronously)
        return planes
    planes2 = _derived("bf16x3-planes-kperm", (W2,), make)
    planes1, off1, n1 = wp1
    x2 = x.reshape(-1, C)
    out = torch.empty_like(x)
    st = _lib.load().dpm_pwconv_pair_bf16x3(_ptr(x2), C, planes1.data_ptr() + 2 * off1, n1, _ptr(b1), _ptr(g1), _ptr(be1),
                                            planes2.data_ptr(), C * H, _ptr(b2), _ptr(g2), _ptr(be2), _ptr(post), _ptr(out),
                                            x2.shape[0], C, H, _stream(x))
    if st == -2:
        return None
    _lib.check(st, "dpm_pwconv_pair_bf16x3")
    return out


def decoder_tail(a: torch.Tensor, z1: torch.Tensor, Wo, bo, g2, be2, W0, b0, W2, b2, g3, be3,
                 post: Optional[torch.Tensor]) -> Optional[torch.Tensor]:
    """LN3(relu(z2 W0^T + b0) W2^T + b2 + z2) [+ post] with z2 = LN2(a Wo^T + bo + z1): the tail of a decoder block in one kernel
    (csrc/gemm_b3.hip, decoder_tail_b3_kernel; C = 256).  None when the layers / layouts are not covered or the knobs route the
    three layers elsewhere: the caller runs linear_layernorm, linear (ReLU), linear_layernorm -- the same rows bit for bit.  The
    conditions are linear_layernorm's for its fused bf16x3 kernel (the row window included), so the tail replaces exactly the
    launches that kernel would have made."""
    C = a.shape[-1]
    if not (knobs.DECODER_TAIL_FUSED and knobs.GEMM_BF16X3 and knobs.GEMM_LN_BF16X3 and knobs.FUSED_LN and C == 256
            and knobs.BF16X3_LN_MIN_K <= C <= knobs.BF16X3_MAX_K and a.is_cuda and a.dtype == torch.float32 and a.dim() == 2
            and a.is_contiguous()):
        return None
    R = a.shape[0]
    if not (R >= FUSED_LN_MIN_ROWS or 1 <= R <= knobs.FUSED_LN_SMALL_ROWS):
        return None
    for t_ in (z1, post):
        if t_ is not None and not (t_.dtype == torch.float32 and t_.is_cuda and t_.is_contiguous() and tuple(t_.shape) == (R, C)):
            return None
    planes = []
    for W, b in ((Wo, bo), (W0, b0), (W2, b2)):
        if tuple(W.shape[:2]) != (C, C) or W.numel() != C * C or (b is not None and b.data_ptr() % 16):
            return None
        wp = _weight_planes(W)
        if wp is None:
            return None
        planes.append(wp)
    for n, t_ in (("gamma2", g2), ("beta2", be2), ("gamma3", g3), ("beta3", be3)):
        _chk(t_, torch.float32, n)
    out = torch.empty(R, C, device=a.device, dtype=torch.float32)
    (po, oo, no), (p0, o0, n0), (p2, o2, n2) = planes
    st = _lib.load().dpm_decoder_tail_bf16x3(_ptr(a), _ptr(z1), _ptr(post), _ptr(out), R, C, po.data_ptr() + 2 * oo, no, _ptr(bo),
                                             _ptr(g2), _ptr(be2), p0.data_ptr() + 2 * o0, n0, _ptr(b0), p2.data_ptr() + 2 * o2, n2,
                                             _ptr(b2), _ptr(g3), _ptr(be3), _stream(a))
    if st == -2:
        return None
    _lib.check(st, "dpm_decoder_tail_bf16x3")
    return out


def three_interp_cat(xyz1, xyz2, lengths2, fea1, fea2) -> torch.Tensor:
    """fine xyz1 (B,N,3)/fea1 (B,N,D1), coarse xyz2 (B,S,3)/fea2 (B,S,D2) -> (B,N,D1+D2)."""
    for n, t in (("xyz1", xyz1), ("xyz2", xyz2), ("fea1", fea1), ("fea2", fea2)):
        _chk(t, torch.float32, n)
    _chk(lengths2, torch.int32, "lengths2")
    B, N, D1 = fea1.shape
    S, D2 = fea2.shape[1], fea2.shape[2]
    out = torch.empty(B, N, D1 + D2, device=fea1.device, dtype=torch.float32)
    _lib.check(_lib.load().dpm_three_interp_cat(_ptr(xyz1), _ptr(xyz2), _ptr(lengths2), _ptr(fea1), _ptr(fea2),
                                                B, N, S, D1, D2, _ptr(out), _stream(fea1)), "dpm_three_interp_cat")
    return out


# ---------------------------------------------------------------------------------------- decoder
def _rows2d(t: torch.Tensor, name: str) -> torch.Tensor:
    """2-D fp32 GPU view with unit column stride (row stride free)."""
    if t.dtype != torch.float32 or not t.is_cuda or t.dim() != 2 or t.stride(1) != 1:
        raise ValueError(f"{name}: expected a 2-D fp32 GPU tensor with unit column stride")
    return t


def posemb(xyz_rows: torch.Tensor, dim_t: torch.Tensor, emb_dim: int) -> torch.Tensor:
    """xyz_rows (R,3) view (row stride free) -> (R, emb_dim)."""
    _rows2d(xyz_rows, "xyz")
    _chk(dim_t, torch.float32, "dim_t")
    R = xyz_rows.shape[0]
    out = torch.empty(R, emb_dim, device=xyz_rows.device, dtype=torch.float32)
    _lib.check(_lib.load().dpm_posemb(_ptr(xyz_rows), xyz_rows.stride(0), _ptr(dim_t), dim_t.numel(), emb_dim, R,
                                      _ptr(out), _stream(out)), "dpm_posemb")
    return out


ATTENTION_SPLIT_MIN_KEYS = 1024   # key-split attention: from this many keys on ...
ATTENTION_SPLIT_BLOCKS = 256      # ... while ONE sequence's plain launch would leave the chip's CUs without a workgroup each


def attention_key_splits(B: int, M: int, N: int, heads: int, head_dim: int) -> int:
    """Number of key ranges for dpm_attention_split (1 = plain kernel): few queries against many keys -- a scan's tokens
    attending a map tile -- give a handful of workgroups that each walk the whole key sequence.  Depends on the shape of
    ONE sequence only, never on the batch size, so a pair's result does not depend on the batch it travels in."""
    if head_dim != 32 or N < ATTENTION_SPLIT_MIN_KEYS:
        return 1
    blocks = -(-M // 64) * heads   # per sequence: B stays out of the rule (see above)
    if blocks >= ATTENTION_SPLIT_BLOCKS:
        return 1
    ns = max(1, min(ATTENTION_SPLIT_BLOCKS // blocks, N // 256, 64))
    chunk = -(-N // (64 * ns)) * 64   # keys per range (whole tiles); drop ranges that would start beyond the last key
    return -(-N // chunk)


def attention(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, B: int, M: int, N: int, heads: int = 8,
              out: Optional[torch.Tensor] = None, kv_shift: int = 0, key_mask: Optional[torch.Tensor] = None,
              seq_index: Optional[torch.Tensor] = None):
    """q (B*M,E) / k,v (B*N,E) row views (column slices of wider buffers allowed) -> (B*M,E)
    (written into `out`, a contiguous (B*M,E) tensor or row range of one, when given).
    kv_shift: sequence b attends the keys / values of sequence (b + kv_shift) mod B.
    key_mask (B,N) uint8, non-zero = padding key (nn.MultiheadAttention's key_padding_mask), indexed like the keys.
    seq_index (B,) int32: q / k / v hold U stored sequences ((U*M,E) / (U*N,E)) and batch element b is stored sequence
    seq_index[b] (its keys / values: stored sequence seq_index[(b + kv_shift) mod B]); the output stays (B*M,E)."""
    for n, t in (("q", q), ("k", k), ("v", v)):
        _rows2d(t, n)
    E = q.shape[1]
    if out is None:
        out = torch.empty(B * M, E, device=q.device, dtype=torch.float32)
    elif tuple(out.shape) != (B * M, E) or not out.is_contiguous() or out.dtype != torch.float32:
        raise ValueError("out must be a contiguous fp32 (B*M, E) tensor")
    if key_mask is not None:
        _chk(key_mask, torch.uint8, "key_mask")
        if tuple(key_mask.shape) != (B, N):
            raise ValueError(f"key_mask must be ({B}, {N}), got {tuple(key_mask.shape)}")
    if seq_index is not None:
        _chk(seq_index, torch.int32, "seq_index")
        if seq_index.numel() != B or key_mask is not None:
            raise ValueError("seq_index must hold B entries and excludes key_mask")
        _lib.check(_lib.load().dpm_attention_indexed(_ptr(q), q.stride(0), M * q.stride(0), _ptr(k), k.stride(0),
                                                     N * k.stride(0), _ptr(v), v.stride(0), N * v.stride(0), _ptr(out), E,
                                                     M * E, B, M, N, heads, E // heads, int(kv_shift), _ptr(seq_index),
                                                     _stream(q)), "dpm_attention_indexed")
        return out
    nsplit = attention_key_splits(B, M, N, heads, E // heads) if key_mask is None else 1
    if nsplit > 1:
        lib = _lib.load()
        ws = torch.empty(lib.dpm_attention_split_workspace_bytes(B, M, heads, E // heads, nsplit), device=q.device, dtype=torch.uint8)
        _lib.check(lib.dpm_attention_split(_ptr(q), q.stride(0), M * q.stride(0), _ptr(k), k.stride(0), N * k.stride(0),
                                           _ptr(v), v.stride(0), N * v.stride(0), _ptr(out), E, M * E, B, M, N, heads,
                                           E // heads, int(kv_shift), nsplit, _ptr(ws), _stream(q)), "dpm_attention_split")
        return out
    _lib.check(_lib.load().dpm_attention_masked(_ptr(q), q.stride(0), M * q.stride(0), _ptr(k), k.stride(0),
                                                N * k.stride(0), _ptr(v), v.stride(0), N * v.stride(0), _ptr(out), E,
                                                M * E, B, M, N, heads, E // heads, int(kv_shift), _ptr(key_mask), _stream(q)),
               "dpm_attention")
    return out


# fewer rows than this: linear() + attention() (identical results; one pair's 512 rows are pure latency, and there the planes'
# epilogue costs more than the split it saves: replayed graph 0.46 -> 0.48 ms)
KV_PLANES_MIN_ROWS = 2048


def linear_kvplanes(x: torch.Tensor, W: torch.Tensor, bias: torch.Tensor, M: int, heads: int = 8):
    """The q | k | v projection half of qkv_attention: x (U*M, E) -> (q (U*M, E) fp32 rows, kv planes (uint8, one 24 KB image per
    (sequence, head, 64-key tile))), or None when the shape is not covered (dpm_linear_bf16x3_kvplanes)."""
    E = x.shape[-1]
    if (not knobs.KV_PLANES or not knobs.GEMM_BF16X3 or E != heads * 32 or M % 64 != 0 or tuple(W.shape) != (3 * E, E) or
            E > knobs.BF16X3_MAX_K or x.dim() != 2 or x.shape[0] % M != 0 or x.dtype != torch.float32 or not x.is_cuda or
            x.stride(1) != 1 or bias is None or bias.data_ptr() % 16 or x.shape[0] < KV_PLANES_MIN_ROWS):
        return None
    wp = _weight_planes(W)
    if wp is None:
        return None
    planes, off, n = wp
    U = x.shape[0] // M
    lib = _lib.load()
    q = torch.empty(U * M, E, device=x.device, dtype=torch.float32)
    kv = torch.empty(lib.dpm_attention_planes_bytes(U, M, heads), device=x.device, dtype=torch.uint8)
    st = lib.dpm_linear_bf16x3_kvplanes(_ptr(x), x.stride(0), planes.data_ptr() + 2 * off, E, n, _ptr(bias), _ptr(q), E, U * M, E, 3 * E, E,
                                        M, heads, _ptr(kv), _stream(x))
    if st == -2:
        return None
    _lib.check(st, "dpm_linear_bf16x3_kvplanes")
    return q, kv


def attention_planes(q: torch.Tensor, kv: torch.Tensor, B: int, M: int, heads: int = 8, kv_shift: int = 0,
                     seq_index: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The attention half of qkv_attention: q (U*M, E) rows and the planes linear_kvplanes made of K / V -> (B*M, E)."""
    E = q.shape[1]
    out = torch.empty(B * M, E, device=q.device, dtype=torch.float32)
    _lib.check(_lib.load().dpm_attention_planes(_ptr(q), E, M * E, _ptr(kv), _ptr(out), E, M * E, B, M, M, heads, int(kv_shift),
                                                _ptr(seq_index), _stream(q)), "dpm_attention_planes")
    return out


def qkv_attention(x: torch.Tensor, W: torch.Tensor, bias: torch.Tensor, B: int, M: int, heads: int = 8, kv_shift: int = 0,
                  seq_index: Optional[torch.Tensor] = None) -> Optional[torch.Tensor]:
    """attention(q, k, v) with q | k | v = x W^T + bias in one hand-over: x (U*M, E) holds U stored sequences of M tokens, W (3E, E)
    is nn.MultiheadAttention's in_proj_weight; batch element b is stored sequence seq_index[b] (None: b, U == B) and attends the
    keys / values of element (b + kv_shift) mod B.  The projection writes Q as fp32 rows and K / V as the attention kernel's bf16
    operand planes (dpm_linear_bf16x3_kvplanes -> dpm_attention_planes): the same values split the same way as
    linear() + attention() would, once per key tile instead of once per query block -- identical results.
    Returns None when the shape is not covered (32-wide heads, M % 64 == 0, no mask, no key ranges, at least KV_PLANES_MIN_ROWS rows;
    the caller runs linear() + attention())."""
    if x.dim() != 2 or M <= 0 or x.shape[0] % M != 0 or attention_key_splits(B, M, M, heads, 32) > 1:
        return None
    if seq_index is not None:
        _chk(seq_index, torch.int32, "seq_index")
        if seq_index.numel() != B:
            raise ValueError("seq_index must hold B entries")
    elif x.shape[0] // M != B:
        raise ValueError("x must hold B sequences when seq_index is not given")
    made = linear_kvplanes(x, W, bias, M, heads)
    if made is None:
        return None
    return attention_planes(made[0], made[1], B, M, heads, kv_shift, seq_index)


def l2_normalize(x: torch.Tensor) -> torch.Tensor:
    _chk(x, torch.float32, "x")
    out = torch.empty_like(x)
    _lib.check(_lib.load().dpm_l2_normalize(_ptr(x), x.numel() // x.shape[-1], x.shape[-1], _ptr(out), _stream(x)),
               "dpm_l2_normalize")
    return out


def dual_softmax_topk(S: torch.Tensor, tau: float, k: int):
    """S (M,N) or (B,M,N) similarity (overwritten with the dual-softmax matrix) ->
    (values (k,) / (B,k), flat idx int32 of the same shape), each row sorted descending."""
    _chk(S, torch.float32, "S")
    single = S.dim() == 2
    B = 1 if single else S.shape[0]
    M, N = S.shape[-2], S.shape[-1]
    lib = _lib.load()
    val = torch.empty(B, k, device=S.device, dtype=torch.float32)
    idx = torch.empty(B, k, device=S.device, dtype=torch.int32)
    ws = torch.empty(lib.dpm_pairing_workspace_bytes(B, M, N), device=S.device, dtype=torch.uint8)
    _lib.check(lib.dpm_dual_softmax_topk(_ptr(S), B, M, N, float(tau), k, _ptr(val), _ptr(idx), _ptr(ws), _stream(S)),
               "dpm_dual_softmax_topk")
    return (val[0], idx[0]) if single else (val, idx)


MATCH_MAX_N, MATCH_MAX_K = 256, 2048   # dpm_match_topk: columns one workgroup holds, pairs its lists hold
MATCH_MAX_MERGE = 8192                 # candidates (strips x k) the last workgroup of a pair merges


def match_supported(M: int, N: int, C: int, k: int) -> bool:
    """shapes dpm_match_topk takes (a function of ONE pair's shape, never of the batch)"""
    # ... and few enough row strips that ONE workgroup merges their candidates quickly: a 4096 x 256 map tile (64 strips x 1088
    # candidates) spent 485 us in that merge against ~200 us for the whole five-kernel form
    strips = -(-M // 64)
    return (N <= MATCH_MAX_N and k <= MATCH_MAX_K and C % 32 == 0 and 1 <= k <= M * N and strips * min(k, 64 * N) <= MATCH_MAX_MERGE)


def match_topk(a: torch.Tensor, b: torch.Tensor, tau: float, k: int):
    """a (B,M,C), b (B,N,C) L2-normalised head outputs -> (values (B,k), flat idx (B,k) int32), sorted descending: similarity,
    dual softmax and top-k of decoder.py:185-191 without the (M,N) matrix in memory.  Raises ValueError for shapes outside
    match_supported()."""
    _chk(a, torch.float32, "a"), _chk(b, torch.float32, "b")
    B, M, C = a.shape
    N = b.shape[1]
    lib = _lib.load()
    val = torch.empty(B, k, device=a.device, dtype=torch.float32)
    idx = torch.empty(B, k, device=a.device, dtype=torch.int32)
    ws = torch.empty(lib.dpm_match_workspace_bytes(B, M, N, k), device=a.device, dtype=torch.uint8)
    _lib.check(lib.dpm_match_topk(_ptr(a), _ptr(b), B, M, N, C, float(tau), k, _ptr(val), _ptr(idx), _ptr(ws), _stream(a)),
               "dpm_match_topk")
    return val, idx


def gather_pairs(x: torch.Tensor, y: torch.Tensor, flat: torch.Tensor):
    """x (B,M,E), y (B,N,E), flat (B,k) -> X (B,2k,2E), src_idx (B,k), dst_idx (B,k)   (2-D inputs: B = 1, 2-D outputs)."""
    _chk(x, torch.float32, "x"), _chk(y, torch.float32, "y"), _chk(flat, torch.int32, "flat")
    single = x.dim() == 2
    B = 1 if single else x.shape[0]
    M, E, N, k = x.shape[-2], x.shape[-1], y.shape[-2], flat.shape[-1]
    X = torch.empty(B, 2 * k, 2 * E, device=x.device, dtype=torch.float32)
    si = torch.empty(B, k, device=x.device, dtype=torch.int32)
    di = torch.empty(B, k, device=x.device, dtype=torch.int32)
    _lib.check(_lib.load().dpm_gather_pairs(_ptr(x), _ptr(y), _ptr(flat), B, k, M, N, E, _ptr(X), _ptr(si), _ptr(di),
                                            _stream(x)), "dpm_gather_pairs")
    return (X[0], si[0], di[0]) if single else (X, si, di)


def mean_rows(x: torch.Tensor, out: torch.Tensor) -> None:
    """x (B,R,C) -> out (B,C) view (row stride free)."""
    _chk(x, torch.float32, "x")
    _rows2d(out, "out")
    B, R, C = x.shape
    _lib.check(_lib.load().dpm_mean_rows(_ptr(x), B, R, C, _ptr(out), out.stride(0), _stream(x)), "dpm_mean_rows")


RES_HDR = 20  # floats before the inlier-confidence list in a corr_kabsch result


def corr_kabsch(offsets, src_xyz, dst_xyz, src_idx, dst_idx, conf, eps_offset: float, num_iter: int = 3,
                std_ratio: float = 3.0, header_out: Optional[torch.Tensor] = None, batch: int = 1) -> torch.Tensor:
    """-> result (batch, 20 + 2k) fp32 (1-D when batch == 1 and conf is 1-D): R(9) T(3) rmse n_corr n_inlier iters
    conf30 (3 reserved), then the inlier confidences.  src_xyz / dst_xyz: (batch*M, 3) row views (row stride
    free) holding the batch elements back to back.  offsets None: (conf, src_xyz, dst_xyz) are ready-made
    correspondences.  header_out: optional (batch, >=20) fp32 view (unit column stride) that also receives
    result[:, :20]."""
    _chk(conf, torch.float32, "conf")
    _rows2d(src_xyz, "src_xyz"), _rows2d(dst_xyz, "dst_xyz")
    k = conf.shape[-1]
    if offsets is not None:
        _chk(offsets, torch.float32, "offsets")
        _chk(src_idx, torch.int32, "src_idx"), _chk(dst_idx, torch.int32, "dst_idx")
    lib = _lib.load()
    ws = torch.empty(lib.dpm_kabsch_workspace_bytes(batch, k), device=conf.device, dtype=torch.uint8)
    result = torch.empty(batch, RES_HDR + 2 * k, device=conf.device, dtype=torch.float32)
    hs = 0
    if header_out is not None:
        if header_out.dim() == 1:
            header_out = header_out.unsqueeze(0)
        _rows2d(header_out, "header_out")
        hs = header_out.stride(0)
    Ms, Md = src_xyz.shape[0] // batch, dst_xyz.shape[0] // batch
    _lib.check(lib.dpm_corr_kabsch(_ptr(offsets), _ptr(src_xyz), src_xyz.stride(0), Ms * src_xyz.stride(0),
                                   _ptr(dst_xyz), dst_xyz.stride(0), Md * dst_xyz.stride(0), _ptr(src_idx),
                                   _ptr(dst_idx), _ptr(conf), batch, k, float(eps_offset), num_iter, float(std_ratio),
                                   _ptr(ws), _ptr(result), _ptr(header_out), hs, _stream(conf)), "dpm_corr_kabsch")
    return result[0] if (batch == 1 and conf.dim() == 1) else result


def information_matrix(pcd1: torch.Tensor, pcd2: torch.Tensor, Rt: torch.Tensor, radius: float = 1.0,
                       out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """pcd1 (3,N1), pcd2 (3,N2) metres on the GPU, Rt (>=12,) [R row-major, T, ...] -> (6,6) fp32 on the GPU
    (written into `out`, a contiguous 36-float view, when given)."""
    _chk(pcd1, torch.float32, "pcd1"), _chk(pcd2, torch.float32, "pcd2"), _chk(Rt, torch.float32, "Rt")
    N1, N2 = pcd1.shape[1], pcd2.shape[1]
    lib = _lib.load()
    ws = torch.empty(lib.dpm_infomat_workspace_bytes(1, N1, N2), device=pcd1.device, dtype=torch.uint8)
    if out is None:
        out = torch.empty(6, 6, device=pcd1.device, dtype=torch.float32)
    else:
        _chk(out, torch.float32, "out")
    _lib.check(lib.dpm_information_matrix(_ptr(pcd1), N1, _ptr(pcd2), N2, _ptr(Rt), float(radius), _ptr(out),
                                          _ptr(ws), _stream(pcd1)), "dpm_information_matrix")
    return out


def information_matrix_batched(pcd: torch.Tensor, src_frame: torch.Tensor, dst_frame: torch.Tensor, Rt_rows: torch.Tensor,
                               out_rows: torch.Tensor, radius: float = 1.0, grids: Optional[torch.Tensor] = None) -> None:
    """pcd (F,3,N) metres; pair p = (src_frame[p], dst_frame[p]) (int32 GPU tensors); Rt_rows (P, >=12) and
    out_rows (P, >=36) are row views (unit column stride) -- typically columns of one edge table.
    grids: the workspace returned by information_matrix_grids(pcd, dst_frame, radius) -- only the search runs."""
    _chk(pcd, torch.float32, "pcd"), _chk(src_frame, torch.int32, "src_frame"), _chk(dst_frame, torch.int32, "dst_frame")
    _rows2d(Rt_rows, "Rt_rows"), _rows2d(out_rows, "out_rows")
    P_, N = src_frame.numel(), pcd.shape[2]
    lib = _lib.load()
    if grids is not None:
        if grids.numel() != lib.dpm_infomat_workspace_bytes(P_, N, N):
            raise ValueError("grids was built for a different (n_pairs, N)")
        _lib.check(lib.dpm_infomat_search_grids(_ptr(pcd), N, _ptr(src_frame), _ptr(dst_frame), P_, _ptr(Rt_rows),
                                                Rt_rows.stride(0), float(radius), _ptr(out_rows), out_rows.stride(0),
                                                _ptr(grids), _stream(pcd)), "dpm_infomat_search_grids")
        return
    ws = torch.empty(lib.dpm_infomat_workspace_bytes(P_, N, N), device=pcd.device, dtype=torch.uint8)
    _lib.check(lib.dpm_information_matrix_batched(_ptr(pcd), N, _ptr(src_frame), _ptr(dst_frame), P_, _ptr(Rt_rows),
                                                  Rt_rows.stride(0), float(radius), _ptr(out_rows), out_rows.stride(0),
                                                  _ptr(ws), _stream(pcd)), "dpm_information_matrix_batched")


def information_matrix_grids(pcd: torch.Tensor, dst_frame: torch.Tensor, radius: float = 1.0) -> torch.Tensor:
    """The pose-independent half of information_matrix_batched: sorts the target scan of every pair into its
    search grid.  Returns the workspace to pass as `grids=` (same pcd, dst_frame and radius)."""
    _chk(pcd, torch.float32, "pcd"), _chk(dst_frame, torch.int32, "dst_frame")
    P_, N = dst_frame.numel(), pcd.shape[2]
    lib = _lib.load()
    ws = torch.empty(lib.dpm_infomat_workspace_bytes(P_, N, N), device=pcd.device, dtype=torch.uint8)
    _lib.check(lib.dpm_infomat_build_grids(_ptr(pcd), N, _ptr(dst_frame), P_, float(radius), _ptr(ws), _stream(pcd)),
               "dpm_infomat_build_grids")
    return ws


# -- batched ICP (csrc/icp.hip; the table builder on top of it is refine.py) -------------------------------------------------
ICP_POINT, ICP_PLANE = 0, 1
ICP_CONVERGED, ICP_MAX_ITER, ICP_NO_MATCH, ICP_SINGULAR = 0, 1, 2, 3
ICP_NSUM = 29   # debug_system: H upper triangle (21), g (6), matches, squared residuals


def icp_target_normals(pcd: torch.Tensor, lengths: torch.Tensor, dst_frame: torch.Tensor, radius: float = 1.0, host=None,
                       out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """(F,N,3) fp32: dpm_point_normals of the valid points of every distinct frame in dst_frame, zeros elsewhere -- the
    `normals` of icp_refine(metric="plane").  Reads lengths and dst_frame on the host (one synchronisation), unless the caller
    knows them already: host = (the frames to compute, the lengths of all F frames) as python ints, and nothing is read.
    out: an (F,N,3) tensor to write those frames' rows into (the other rows keep what they hold)."""
    _chk(pcd, torch.float32, "pcd"), _chk(lengths, torch.int32, "lengths"), _chk(dst_frame, torch.int32, "dst_frame")
    F, _, N = pcd.shape
    lib = _lib.load()
    normals = torch.zeros(F, N, 3, device=pcd.device, dtype=torch.float32) if out is None else _chk(out, torch.float32, "out")
    if tuple(normals.shape) != (F, N, 3):
        raise ValueError("out: expected (F,N,3)")
    ws = torch.empty(lib.dpm_knn_self_workspace_bytes(N), device=pcd.device, dtype=torch.uint8)
    frames, counts = (dst_frame.tolist(), lengths.tolist()) if host is None else host
    for f in sorted(set(int(f) for f in frames)):
        if not 0 <= f < F:
            raise ValueError(f"dst_frame: frame {f} outside [0, {F})")
        n = min(max(int(counts[f]), 0), N)
        if n == 0:
            continue
        xyz = pcd[f, :, :n].t().contiguous()
        rows = torch.empty(n, 3, device=pcd.device, dtype=torch.float32)
        _lib.check(lib.dpm_point_normals(_ptr(xyz), n, float(radius), _ptr(rows), _ptr(ws), _stream(pcd)), "dpm_point_normals")
        normals[f, :n] = rows
    return normals


def _schedule_arrays(schedule):
    """schedule = [(max_dist, max_iter), ...] -> (ctypes double array of the distances, int32 array of the limits, their number)"""
    stages = [(float(d), int(n)) for d, n in schedule]
    if not stages:
        raise ValueError("schedule: at least one (max_dist, max_iter) stage")
    dist, iters = zip(*stages)
    return (ctypes.c_double * len(stages))(*dist), (ctypes.c_int32 * len(stages))(*iters), len(stages)


def _registration_results(n: int, dev):
    """the results of n registration problems: pose (n,4,4) fp64, fitness, rmse (n,) fp32, iterations, status (n,) int32"""
    new = lambda dtype, *shape: torch.empty(n, *shape, device=dev, dtype=dtype)
    return new(torch.float64, 4, 4), new(torch.float32), new(torch.float32), new(torch.int32), new(torch.int32)


def icp_refine(pcd: torch.Tensor, lengths: torch.Tensor, src_frame: torch.Tensor, dst_frame: torch.Tensor, init: torch.Tensor,
               schedule, metric: int = ICP_PLANE, tol_rot: float = 1e-7, tol_trans: float = 1e-6,
               normals: Optional[torch.Tensor] = None, debug: bool = False):
    """pcd (F,3,N) fp32 metres, lengths (F,) int32, pair p = (src_frame[p], dst_frame[p]) int32, init (P,4,4) fp64: the pose
    of the source in the target; schedule = [(max_dist, max_iter), ...]; normals (F,N,3) for ICP_PLANE (icp_target_normals).
    -> pose (P,4,4) fp64, fitness (P,) fp32, rmse (P,) fp32, iterations (P,) int32, status (P,) int32[, match (P,N) int32,
    system (P,29) fp64 with debug].  All on the GPU; no host synchronisation, capturable in a graph."""
    _chk(pcd, torch.float32, "pcd"), _chk(lengths, torch.int32, "lengths"), _chk(init, torch.float64, "init")
    _chk(src_frame, torch.int32, "src_frame"), _chk(dst_frame, torch.int32, "dst_frame")
    F, three, N = pcd.shape
    P_ = src_frame.numel()
    if three != 3 or lengths.numel() != F or dst_frame.numel() != P_ or tuple(init.shape) != (P_, 4, 4):
        raise ValueError("icp_refine: pcd (F,3,N), lengths (F,), src_frame / dst_frame (P,), init (P,4,4)")
    if metric == ICP_PLANE:
        if normals is None:
            raise ValueError("icp_refine: the plane metric needs normals (icp_target_normals)")
        _chk(normals, torch.float32, "normals")
        if tuple(normals.shape) != (F, N, 3):
            raise ValueError("normals: expected (F,N,3)")
    else:
        normals = None
    dist, iters, n_stages = _schedule_arrays(schedule)
    dev = pcd.device
    lib = _lib.load()
    pose, fitness, rmse, iterations, status = _registration_results(P_, dev)
    match = torch.full((P_, N), -1, device=dev, dtype=torch.int32) if debug else None
    system = torch.zeros(P_, ICP_NSUM, device=dev, dtype=torch.float64) if debug else None
    ws = torch.empty(lib.dpm_icp_workspace_bytes(P_, N), device=dev, dtype=torch.uint8)
    _lib.check(lib.dpm_icp_refine_batched(_ptr(pcd), F, N, _ptr(lengths), _ptr(normals), _ptr(src_frame), _ptr(dst_frame), P_,
                                          _ptr(init), int(metric), ctypes.addressof(dist), ctypes.addressof(iters), n_stages,
                                          float(tol_rot), float(tol_trans), _ptr(pose), _ptr(fitness), _ptr(rmse),
                                          _ptr(iterations), _ptr(status), _ptr(match), _ptr(system), _ptr(ws), _stream(pcd)),
               "dpm_icp_refine_batched")
    out = (pose, fitness, rmse, iterations, status)
    return out + (match, system) if debug else out


# -- the global map (csrc/voxel_map.hip; orchestration in globalmap.py) ------------------------------------------------------
VOXEL_MAP_HDR_BYTES = 256   # the workspace header globalmap.py reads back between the calls (include/dpm_hip.h)


def voxel_map_workspace_bytes(n_points: int) -> int:
    return int(_lib.load().dpm_voxel_map_workspace_bytes(int(n_points)))


def voxel_map_init(ws: torch.Tensor, n_points: int) -> None:
    _chk(ws, torch.uint8, "workspace")
    _lib.check(_lib.load().dpm_voxel_map_init(int(n_points), _ptr(ws), _stream(ws)), "dpm_voxel_map_init")


def voxel_map_bounds(ws: torch.Tensor, clouds: int, offsets: int, poses: int, n_scans: int, n_batch: int) -> None:
    """clouds / offsets / poses: device addresses of the batch's pointer, offset (int64) and pose (12 fp32 per scan) arrays"""
    _chk(ws, torch.uint8, "workspace")
    _lib.check(_lib.load().dpm_voxel_map_bounds(clouds, offsets, poses, int(n_scans), int(n_batch), _ptr(ws), _stream(ws)),
               "dpm_voxel_map_bounds")


def voxel_map_insert(ws: torch.Tensor, clouds: int, offsets: int, poses: int, n_scans: int, n_batch: int, base: int,
                     n_points: int, min_b, voxel_size: float) -> None:
    _chk(ws, torch.uint8, "workspace")
    _lib.check(_lib.load().dpm_voxel_map_insert(clouds, offsets, poses, int(n_scans), int(n_batch), int(base), int(n_points),
                                                float(min_b[0]), float(min_b[1]), float(min_b[2]), float(voxel_size),
                                                _ptr(ws), _stream(ws)), "dpm_voxel_map_insert")


def voxel_map_finish(ws: torch.Tensor, n_points: int) -> None:
    _chk(ws, torch.uint8, "workspace")
    _lib.check(_lib.load().dpm_voxel_map_finish(int(n_points), _ptr(ws), _stream(ws)), "dpm_voxel_map_finish")


def voxel_map_emit(ws: torch.Tensor, n_points: int, min_b, voxel_size: float, M: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """-> centroids (3,M) fp32, counts (M,) int32 on the workspace's device"""
    _chk(ws, torch.uint8, "workspace")
    out = torch.empty(3, M, device=ws.device, dtype=torch.float32)
    cnt = torch.empty(M, device=ws.device, dtype=torch.int32)
    _lib.check(_lib.load().dpm_voxel_map_emit(_ptr(ws), int(n_points), float(min_b[0]), float(min_b[1]), float(min_b[2]),
                                              float(voxel_size), _ptr(out), _ptr(cnt), int(M), _stream(ws)),
               "dpm_voxel_map_emit")
    return out, cnt


# ---- RegistrationLoss (training): csrc/reg_loss.hip ----------------------------------------------------------------------

def _shape(t: torch.Tensor, want, name: str):
    """the kernels index these tensors together: refuse any that disagrees with the shape the others define"""
    if tuple(t.shape) != tuple(want):
        raise ValueError(f"{name}: expected shape {tuple(want)}, got {tuple(t.shape)}")
    return t


def reg_loss_pairs(xyz_a: torch.Tensor, xyz_b: torch.Tensor, eps: float, neutral_counts: bool = False):
    """xyz_a (B,3,M), xyz_b (B,3,N) fp32 -> nn_a (B,M), nn_b (B,N) int32 (make_pairs of both directions: the first nearest
    neighbour where its squared distance is <= eps^2, else -1) [, neutral_a (B,M), neutral_b (B,N) int32: per row the entries
    within eps other than the neighbour]."""
    _chk(xyz_a, torch.float32, "xyz_a"), _chk(xyz_b, torch.float32, "xyz_b")
    if xyz_a.dim() != 3 or xyz_b.dim() != 3:
        raise ValueError(f"coordinates must be (B,3,M) / (B,3,N), got {tuple(xyz_a.shape)} / {tuple(xyz_b.shape)}")
    B, _, M = xyz_a.shape
    N = xyz_b.shape[2]
    _shape(xyz_a, (B, 3, M), "xyz_a"), _shape(xyz_b, (B, 3, N), "xyz_b")
    nn_a = torch.empty(B, M, device=xyz_a.device, dtype=torch.int32)
    nn_b = torch.empty(B, N, device=xyz_a.device, dtype=torch.int32)
    ne_a = torch.empty_like(nn_a) if neutral_counts else None
    ne_b = torch.empty_like(nn_b) if neutral_counts else None
    _lib.check(_lib.load().dpm_reg_loss_pairs(_ptr(xyz_a), _ptr(xyz_b), B, M, N, float(eps), _ptr(nn_a), _ptr(nn_b), _ptr(ne_a),
                                              _ptr(ne_b), _stream(xyz_a)), "dpm_reg_loss_pairs")
    return (nn_a, nn_b, ne_a, ne_b) if neutral_counts else (nn_a, nn_b)


def reg_loss_forward(fea_a, fea_b, xyz_a, xyz_b, pad_a, pad_b, nn_a, nn_b, tau: float, eps: float, neutral: bool,
                     argmax: bool = False):
    """One feature pair (B,C,M) / (B,C,N) fp32 through both InfoNCE directions -> (loss 0-d, stats (8,), workspace[, argmax_a,
    argmax_b]); the workspace is what reg_loss_backward reads.  pad_*: bool, True on padding.  Raises ValueError for C outside
    {64, 128, 192, 256}."""
    for t, n in ((fea_a, "fea_a"), (fea_b, "fea_b")):
        _chk(t, torch.float32, n)
    _chk(pad_a, torch.bool, "pad_a"), _chk(pad_b, torch.bool, "pad_b")
    _chk(nn_a, torch.int32, "nn_a"), _chk(nn_b, torch.int32, "nn_b")
    if neutral:
        _chk(xyz_a, torch.float32, "xyz_a"), _chk(xyz_b, torch.float32, "xyz_b")
    if fea_a.dim() != 3 or fea_b.dim() != 3:
        raise ValueError(f"features must be (B,C,M) / (B,C,N), got {tuple(fea_a.shape)} / {tuple(fea_b.shape)}")
    B, C, M = fea_a.shape
    N = fea_b.shape[2]
    _shape(fea_b, (B, C, N), "fea_b")
    _shape(pad_a, (B, M), "pad_a"), _shape(pad_b, (B, N), "pad_b")
    _shape(nn_a, (B, M), "nn_a"), _shape(nn_b, (B, N), "nn_b")
    if neutral:
        _shape(xyz_a, (B, 3, M), "xyz_a"), _shape(xyz_b, (B, 3, N), "xyz_b")
    lib = _lib.load()
    dev = fea_a.device
    ws = torch.empty(lib.dpm_reg_loss_workspace_bytes(B, M, N, C), device=dev, dtype=torch.uint8)
    loss = torch.empty((), device=dev, dtype=torch.float32)
    stats = torch.empty(8, device=dev, dtype=torch.float32)
    am_a = torch.empty(B, M, device=dev, dtype=torch.int32) if argmax else None
    am_b = torch.empty(B, N, device=dev, dtype=torch.int32) if argmax else None
    _lib.check(lib.dpm_reg_loss_forward(_ptr(fea_a), _ptr(fea_b), _ptr(xyz_a) if neutral else None,
                                        _ptr(xyz_b) if neutral else None, _ptr(pad_a), _ptr(pad_b), _ptr(nn_a), _ptr(nn_b), B, M,
                                        N, C, float(tau), float(eps), int(neutral), _ptr(am_a), _ptr(am_b), _ptr(loss),
                                        _ptr(stats), _ptr(ws), _stream(fea_a)), "dpm_reg_loss_forward")
    return (loss, stats, ws, am_a, am_b) if argmax else (loss, stats, ws)


def reg_loss_backward(xyz_a, xyz_b, nn_a, nn_b, shape, tau: float, eps: float, neutral: bool, grad_loss: torch.Tensor,
                      stats: torch.Tensor, ws: torch.Tensor):
    """Gradients (B,C,M), (B,C,N) of grad_loss (0-d fp32 on the device) x the loss reg_loss_forward returned with stats / ws."""
    B, C, M, N = shape
    _chk(grad_loss, torch.float32, "grad_loss"), _shape(grad_loss, (), "grad_loss")
    _chk(nn_a, torch.int32, "nn_a"), _chk(nn_b, torch.int32, "nn_b")
    _shape(nn_a, (B, M), "nn_a"), _shape(nn_b, (B, N), "nn_b")
    if neutral:
        _shape(xyz_a, (B, 3, M), "xyz_a"), _shape(xyz_b, (B, 3, N), "xyz_b")
    _shape(stats, (8,), "stats")
    if ws.numel() < _lib.load().dpm_reg_loss_workspace_bytes(B, M, N, C):
        raise ValueError("reg_loss_backward: the workspace is smaller than this shape's forward needs")
    ga = torch.empty(B, C, M, device=ws.device, dtype=torch.float32)
    gb = torch.empty(B, C, N, device=ws.device, dtype=torch.float32)
    _lib.check(_lib.load().dpm_reg_loss_backward(_ptr(xyz_a) if neutral else None, _ptr(xyz_b) if neutral else None, _ptr(nn_a),
                                                 _ptr(nn_b), B, M, N, C, float(tau), float(eps), int(neutral), _ptr(grad_loss),
                                                 _ptr(stats), _ptr(ws), _ptr(ga), _ptr(gb), _stream(ws)),
               "dpm_reg_loss_backward")
    return ga, gb


# ---- attention for training: csrc/attention_train.hip ----------------------------------------------------------------------

ATTENTION_TRAIN_HEAD_DIM = 32   # the one head width dpm_attention_train_* implements (model_channel 256, 8 heads)


def _attention_train_args(q, k, v, B: int, M: int, N: int, heads: int, key_mask):
    for n, t, rows in (("q", q, B * M), ("k", k, B * N), ("v", v, B * N)):
        _rows2d(t, n)
        if t.shape[0] != rows:
            raise ValueError(f"{n}: expected {rows} rows, got {t.shape[0]}")
    E = q.shape[1]
    if k.shape[1] != E or v.shape[1] != E or heads < 1 or E % heads:
        raise ValueError(f"q / k / v must share a width divisible by heads = {heads}, got {q.shape[1]}, {k.shape[1]}, {v.shape[1]}")
    if E // heads != ATTENTION_TRAIN_HEAD_DIM:
        raise ValueError(f"attention_train: head width {E // heads} is not supported, only {ATTENTION_TRAIN_HEAD_DIM} "
                         f"(model_channel {ATTENTION_TRAIN_HEAD_DIM * heads} at {heads} heads)")
    if key_mask is not None:
        _chk(key_mask, torch.uint8, "key_mask")
        if tuple(key_mask.shape) != (B, N):
            raise ValueError(f"key_mask must be ({B}, {N}), got {tuple(key_mask.shape)}")
    return E


def attention_train_forward(q, k, v, B: int, M: int, N: int, heads: int = 8, key_mask: Optional[torch.Tensor] = None):
    """q (B*M,E) / k, v (B*N,E) row views -> (out (B*M,E), lse (B,heads,M)): the attention core and the log-sum-exp of every
    score row over its unmasked keys, which is all the backward needs besides the operands."""
    E = _attention_train_args(q, k, v, B, M, N, heads, key_mask)
    out = torch.empty(B * M, E, device=q.device, dtype=torch.float32)
    lse = torch.empty(B, heads, M, device=q.device, dtype=torch.float32)
    _lib.check(_lib.load().dpm_attention_train_forward(_ptr(q), q.stride(0), M * q.stride(0), _ptr(k), k.stride(0), N * k.stride(0),
                                                       _ptr(v), v.stride(0), N * v.stride(0), _ptr(out), E, M * E, _ptr(lse), B, M,
                                                       N, heads, E // heads, _ptr(key_mask), _stream(q)),
               "dpm_attention_train_forward")
    return out, lse


def attention_train_backward(q, k, v, out, lse, dout, B: int, M: int, N: int, heads: int = 8,
                             key_mask: Optional[torch.Tensor] = None):
    """-> (dq (B*M,E), dk (B*N,E), dv (B*N,E)) from the operands, the forward's out / lse and dout (B*M,E).  Deterministic."""
    E = _attention_train_args(q, k, v, B, M, N, heads, key_mask)
    _rows2d(out, "out"), _rows2d(dout, "dout")
    _chk(lse, torch.float32, "lse")
    _shape(out, (B * M, E), "out"), _shape(dout, (B * M, E), "dout"), _shape(lse, (B, heads, M), "lse")
    lib = _lib.load()
    dev = q.device
    ws = torch.empty(lib.dpm_attention_train_workspace_bytes(B, M, N, heads), device=dev, dtype=torch.uint8)
    dq = torch.empty(B * M, E, device=dev, dtype=torch.float32)
    dk = torch.empty(B * N, E, device=dev, dtype=torch.float32)
    dv = torch.empty(B * N, E, device=dev, dtype=torch.float32)
    _lib.check(lib.dpm_attention_train_backward(_ptr(q), q.stride(0), M * q.stride(0), _ptr(k), k.stride(0), N * k.stride(0),
                                                _ptr(v), v.stride(0), N * v.stride(0), _ptr(out), out.stride(0), M * out.stride(0),
                                                _ptr(lse), _ptr(dout), dout.stride(0), M * dout.stride(0), _ptr(key_mask), _ptr(dq),
                                                _ptr(dk), _ptr(dv), B, M, N, heads, E // heads, _ptr(ws), _stream(q)),
               "dpm_attention_train_backward")
    return dq, dk, dv


class _AttentionTrain(torch.autograd.Function):
    """Saved for the backward: the operands, out and lse -- no probability tensor."""

    @staticmethod
    def forward(ctx, q, k, v, B, M, N, heads, key_mask):
        out, lse = attention_train_forward(q, k, v, B, M, N, heads, key_mask)
        ctx.save_for_backward(q, k, v, out, lse)
        ctx.mask, ctx.cfg = key_mask, (B, M, N, heads)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dout):
        q, k, v, out, lse = ctx.saved_tensors
        if dout.stride(1) != 1 or dout.stride(0) % 4 or dout.data_ptr() % 16:
            dout = dout.contiguous()
        dq, dk, dv = attention_train_backward(q, k, v, out, lse, dout, *ctx.cfg, key_mask=ctx.mask)
        return dq, dk, dv, None, None, None, None, None


def attention_train(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, B: int, M: int, N: int, heads: int = 8,
                    key_mask: Optional[torch.Tensor] = None) -> torch.Tensor:
    """ops.attention for training: q (B*M,E) / k, v (B*N,E) fp32 row views (column slices of wider buffers allowed, rows 16-byte
    aligned) -> (B*M,E), differentiable with respect to q, k and v.  key_mask (B,N) uint8, non-zero = padding key
    (nn.MultiheadAttention's key_padding_mask); masked keys get exactly zero gradients.  Forward and backward run in
    csrc/attention_train.hip in strips of the score matrix: no (B,heads,M,N) tensor exists, what is saved for the backward is
    the output and one log-sum-exp per score row, and two runs give identical bytes.  Head width 32 only (ValueError
    otherwise).  A sequence whose keys are all padding is a precondition violation: it yields NaN, as the reference does."""
    return _AttentionTrain.apply(q, k, v, B, M, N, heads, key_mask)


# ---- offset pairs of the training forward: csrc/offset_pairs.hip -----------------------------------------------------------

def _offset_pairs_offsets(xa, xb, pa, pb, eps: float):
    B, _, M = xa.shape
    N = xb.shape[2]
    counts = torch.empty(B * M, device=xa.device, dtype=torch.int32)
    offsets = torch.empty(B * M + 1, device=xa.device, dtype=torch.int32)
    _lib.check(_lib.load().dpm_offset_pairs_count(_ptr(xa), _ptr(xb), _ptr(pa), _ptr(pb), B, M, N, float(eps), _ptr(counts),
                                                  _ptr(offsets), _stream(xa)), "dpm_offset_pairs_count")
    return offsets


def offset_pairs(xyz_a: torch.Tensor, xyz_b: torch.Tensor, pad_a: torch.Tensor, pad_b: torch.Tensor, eps: float):
    """xyz_a (B,3,M), xyz_b (B,3,N) fp32, pad_* (B,M) / (B,N) bool (True = padding) -> (triples (K,3) int32, offsets_a (B*M+1),
    offsets_b (B*N+1), perm_b (K,) int32): every (batch, a, b) with squared distance <= eps^2 between unpadded tokens in
    torch.nonzero's order; offsets_a[r] .. offsets_a[r+1] are the pairs of a row r; perm_b lists the pairs stably sorted by b
    row, offsets_b their ranges -- what offset_pair_rows' backward sums over.  One host synchronisation (K sizes the list)."""
    _chk(xyz_a, torch.float32, "xyz_a"), _chk(xyz_b, torch.float32, "xyz_b")
    _chk(pad_a, torch.bool, "pad_a"), _chk(pad_b, torch.bool, "pad_b")
    if xyz_a.dim() != 3 or xyz_b.dim() != 3:
        raise ValueError(f"coordinates must be (B,3,M) / (B,3,N), got {tuple(xyz_a.shape)} / {tuple(xyz_b.shape)}")
    B, _, M = xyz_a.shape
    N = xyz_b.shape[2]
    _shape(xyz_a, (B, 3, M), "xyz_a"), _shape(xyz_b, (B, 3, N), "xyz_b")
    _shape(pad_a, (B, M), "pad_a"), _shape(pad_b, (B, N), "pad_b")
    off_a = _offset_pairs_offsets(xyz_a, xyz_b, pad_a, pad_b, eps)
    off_b = _offset_pairs_offsets(xyz_b, xyz_a, pad_b, pad_a, eps)   # the distance is symmetric bit for bit: the same pairs
    K = int(off_a[-1])
    if K < 0:
        raise ValueError("offset_pairs: more than 2^31 - 1 pairs")
    triples = torch.empty(K, 3, device=xyz_a.device, dtype=torch.int32)
    if K:
        _lib.check(_lib.load().dpm_offset_pairs_fill(_ptr(xyz_a), _ptr(xyz_b), _ptr(pad_a), _ptr(pad_b), B, M, N, float(eps),
                                                     _ptr(off_a), _ptr(triples), _stream(xyz_a)), "dpm_offset_pairs_fill")
    key = triples[:, 0].long() * N + triples[:, 2].long()
    perm_b = torch.sort(key, stable=True)[1].to(torch.int32)
    return triples, off_a, off_b, perm_b


def _segment_sum(g: torch.Tensor, offsets: torch.Tensor, perm: Optional[torch.Tensor], R: int) -> torch.Tensor:
    E = g.shape[1]
    out = torch.empty(R, E, device=g.device, dtype=torch.float32)
    _lib.check(_lib.load().dpm_offset_pairs_segment_sum(_ptr(g) if g.numel() else None, max(g.stride(0), E), _ptr(offsets),
                                                        _ptr(perm) if perm is not None and perm.numel() else None, R, E, _ptr(out),
                                                        _stream(out)), "dpm_offset_pairs_segment_sum")
    return out


class _OffsetPairRows(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, y, triples, off_a, off_b, perm_b, M, N):
        K, E = triples.shape[0], x.shape[1]
        lib = _lib.load()
        outs = []
        for side, (t, rows) in enumerate(((x, M), (y, N))):
            o = torch.empty(K, E, device=x.device, dtype=torch.float32)
            _lib.check(lib.dpm_offset_pairs_gather(_ptr(t), t.stride(0), _ptr(triples), side, rows, K, E, _ptr(o), _stream(t)),
                       "dpm_offset_pairs_gather")
            outs.append(o)
        ctx.save_for_backward(off_a, off_b, perm_b)
        ctx.rows = (x.shape[0], y.shape[0])
        return outs[0], outs[1]

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, ga, gb):
        off_a, off_b, perm_b = ctx.saved_tensors
        gx = _segment_sum(ga.contiguous(), off_a, None, ctx.rows[0])
        gy = _segment_sum(gb.contiguous(), off_b, perm_b, ctx.rows[1])
        return gx, gy, None, None, None, None, None, None


def offset_pair_rows(x: torch.Tensor, y: torch.Tensor, pairs, M: int, N: int):
    """x (B*M,E), y (B*N,E) fp32 rows, pairs = offset_pairs(...) -> (x rows of the pairs' a tokens (K,E), y rows of their b tokens
    (K,E)), differentiable: the backward adds the K gradient rows back per token in a fixed order (no atomics)."""
    _rows2d(x, "x"), _rows2d(y, "y")
    triples, off_a, off_b, perm_b = pairs
    if x.shape[1] != y.shape[1] or x.shape[1] % 4 or x.stride(0) % 4 or y.stride(0) % 4:
        raise ValueError("offset_pair_rows: x and y must share a width that is a multiple of 4, rows 16-byte aligned")
    if x.shape[0] + 1 != off_a.numel() or y.shape[0] + 1 != off_b.numel():
        raise ValueError("offset_pair_rows: the pair list was made for other row counts")
    return _OffsetPairRows.apply(x, y, triples, off_a, off_b, perm_b, M, N)


# ---- the encoder's grouping layer for training: csrc/group_train.hip -------------------------------------------------------

GROUP_TRAIN_COUT = (32, 64, 128, 256, 512)   # the widths and neighbour counts dpm_group_train_* implements: every shipped layer
GROUP_TRAIN_K = (16, 32)
GROUP_TRAIN_NO_WINNER = 255                  # slot value where no neighbour exceeds the ReLU floor


def _group_train_args(P, xyz, centers, idx, W_rel, gamma, layer: str):
    for n, t in (("P", P), ("xyz", xyz), ("centers", centers), ("W_rel", W_rel), ("gamma", gamma)):
        _chk(t, torch.float32, n)
    _chk(idx, torch.int32, "idx")
    if P.dim() != 3 or idx.dim() != 3:
        raise ValueError("group_train: P must be (B,N,Cout) and idx (B,S,K)")
    B, N, Cout = P.shape
    S, K = idx.shape[1], idx.shape[2]
    if Cout not in GROUP_TRAIN_COUT or K not in GROUP_TRAIN_K:
        raise ValueError(f"group_train: layer {layer or '<unnamed>'} has width {Cout} and {K} neighbours; the training kernels cover "
                         f"widths {GROUP_TRAIN_COUT} and neighbour counts {GROUP_TRAIN_K}")
    _shape(xyz, (B, N, 3), "xyz"), _shape(centers, (B, S, 3), "centers"), _shape(W_rel, (Cout, 3), "W_rel")
    _shape(gamma, (Cout,), "gamma")
    if idx.shape[0] != B:
        raise ValueError(f"idx must be ({B}, S, K), got {tuple(idx.shape)}")
    return B, N, S, K, Cout


def group_train_forward(P, xyz, centers, idx, W_rel, gamma, beta, radius: float, layer: str = ""):
    """P (B,N,Cout) projected point rows, xyz (B,N,3), centers (B,S,3), idx (B,S,K) int32, W_rel (Cout,3) ->
    (out (B,S,Cout), slots (B,S,Cout) uint8): dpm_group_gather_ln_max's result and, per channel, the neighbour slot k that
    gave the maximum (GROUP_TRAIN_NO_WINNER where the ReLU floor did) -- all the backward needs besides the operands."""
    B, N, S, K, Cout = _group_train_args(P, xyz, centers, idx, W_rel, gamma, layer)
    _chk(beta, torch.float32, "beta"), _shape(beta, (Cout,), "beta")
    out = torch.empty(B, S, Cout, device=P.device, dtype=torch.float32)
    slots = torch.empty(B, S, Cout, device=P.device, dtype=torch.uint8)
    _lib.check(_lib.load().dpm_group_train_forward(_ptr(P), _ptr(xyz), _ptr(centers), _ptr(idx), _ptr(W_rel), 3, _ptr(gamma),
                                                   _ptr(beta), B, N, S, K, Cout, float(radius), _ptr(out), _ptr(slots),
                                                   _stream(P)), "dpm_group_train_forward")
    return out, slots


def group_train_backward(P, xyz, centers, idx, W_rel, gamma, radius: float, dout, slots, layer: str = ""):
    """-> (dP (B,N,Cout), dW_rel (Cout,3), dgamma (Cout), dbeta (Cout)) from the operands, the forward's slots and dout
    (B,S,Cout).  Deterministic; rows of dP that no winning neighbour names are exact zeros."""
    B, N, S, K, Cout = _group_train_args(P, xyz, centers, idx, W_rel, gamma, layer)
    _chk(dout, torch.float32, "dout"), _chk(slots, torch.uint8, "slots")
    _shape(dout, (B, S, Cout), "dout"), _shape(slots, (B, S, Cout), "slots")
    lib, dev = _lib.load(), P.device
    ws = torch.empty(lib.dpm_group_train_workspace_bytes(B, N, S, K, Cout), device=dev, dtype=torch.uint8)
    dP = torch.empty(B, N, Cout, device=dev, dtype=torch.float32)
    dW = torch.empty(Cout, 3, device=dev, dtype=torch.float32)
    dgamma = torch.empty(Cout, device=dev, dtype=torch.float32)
    dbeta = torch.empty(Cout, device=dev, dtype=torch.float32)
    _lib.check(lib.dpm_group_train_backward(_ptr(P), _ptr(xyz), _ptr(centers), _ptr(idx), _ptr(W_rel), 3, _ptr(gamma), B, N, S, K,
                                            Cout, float(radius), _ptr(dout), _ptr(slots), _ptr(dP), _ptr(dW), _ptr(dgamma),
                                            _ptr(dbeta), _ptr(ws), _stream(P)), "dpm_group_train_backward")
    return dP, dW, dgamma, dbeta


class _GroupTrain(torch.autograd.Function):
    """Saved for the backward: P, the (small) geometry and layer tensors and one byte per output element -- no (B,S,K,Cout) tensor."""

    @staticmethod
    def forward(ctx, P, W_rel, gamma, beta, xyz, centers, idx, radius, layer, keep):
        out, slots = group_train_forward(P, xyz, centers, idx, W_rel, gamma, beta, radius, layer)
        ctx.save_for_backward(P, W_rel, gamma, xyz, centers, idx, slots)
        ctx.cfg = (float(radius), layer)
        if keep is not None:
            keep.append(slots)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dout):
        P, W_rel, gamma, xyz, centers, idx, slots = ctx.saved_tensors
        radius, layer = ctx.cfg
        dP, dW, dgamma, dbeta = group_train_backward(P, xyz, centers, idx, W_rel, gamma, radius, dout.contiguous(), slots, layer)
        return dP, dW, dgamma, dbeta, None, None, None, None, None, None


def group_train(P: torch.Tensor, xyz: torch.Tensor, centers: torch.Tensor, idx: torch.Tensor, W_rel: torch.Tensor,
                gamma: torch.Tensor, beta: torch.Tensor, radius: float, layer: str = "", keep_slots: Optional[list] = None):
    """The grouping layer for training: out[b,s,c] = max_k relu(LN_c(P[b, idx[b,s,k]] + W_rel (xyz[idx] - centre) / radius)),
    differentiable with respect to P, W_rel (Cout,3), gamma and beta (LayerNorm eps 1e-5, biased variance); the geometry gets
    no gradient.  P = fea W_f^T + b is the caller's, under autograd.  Forward and backward run in csrc/group_train.hip; what is
    saved is P and a byte per output element, and two runs give identical bytes.  idx entries outside [0, N) are read as
    clamped to it, as the inference kernels do.  Rows of P and xyz that idx never names are not read into any result and may
    hold anything; their dP rows are exact zeros.  ValueError (naming `layer`) for a width
    outside GROUP_TRAIN_COUT or a neighbour count outside GROUP_TRAIN_K.  keep_slots: a list that receives the winning slots
    (group_train_winners turns them into point indices)."""
    return _GroupTrain.apply(P, W_rel, gamma, beta, xyz, centers, idx, radius, layer, keep_slots)


def group_train_winners(idx: torch.Tensor, slots: torch.Tensor) -> torch.Tensor:
    """idx (B,S,K) int32, slots (B,S,Cout) uint8 -> (B,S,Cout) int64: the POINT idx[b,s,slot] that wins channel c of centre s,
    -1 where none does (the ReLU floor)."""
    live = slots != GROUP_TRAIN_NO_WINNER
    pts = torch.gather(idx.long(), 2, slots.long().clamp(max=idx.shape[2] - 1))
    return torch.where(live, pts, torch.full_like(pts, -1))


# ---- the loop head for training: csrc/loop_head_train.hip ------------------------------------------------------------------

LOOP_POOL_CHANNELS = 256   # the one width dpm_loop_pool_* implements (model_channel of every shipped config)


def _loop_pool_args(x, B: int, L: int, W1, b1):
    _rows2d(x, "x")
    E = x.shape[1]
    if E != LOOP_POOL_CHANNELS:
        raise ValueError(f"loop_pool: width {E} is not supported, only {LOOP_POOL_CHANNELS} (model_channel)")
    if B < 1 or L < 1:
        raise ValueError(f"loop_pool: needs B >= 1 sequences of L >= 1 tokens, got B = {B}, L = {L}")
    if x.shape[0] != B * L:
        raise ValueError(f"x: expected {B * L} rows (B * L), got {x.shape[0]}")
    _chk(W1, torch.float32, "W1"), _chk(b1, torch.float32, "b1")
    _shape(W1, (E, E), "W1"), _shape(b1, (E,), "b1")
    return E


def loop_pool_forward(x: torch.Tensor, B: int, L: int, W1: torch.Tensor, b1: torch.Tensor) -> torch.Tensor:
    """x (B*L, E) fp32 row view, W1 (E,E), b1 (E) -> m (B,E) = mean over the L tokens of relu(x W1^T + b1)."""
    E = _loop_pool_args(x, B, L, W1, b1)
    lib = _lib.load()
    ws = torch.empty(lib.dpm_loop_pool_workspace_bytes(B, L, E), device=x.device, dtype=torch.uint8)
    m = torch.empty(B, E, device=x.device, dtype=torch.float32)
    _lib.check(lib.dpm_loop_pool_forward(_ptr(x), x.stride(0), _ptr(W1), _ptr(b1), B, L, E, _ptr(m), _ptr(ws), _stream(x)),
               "dpm_loop_pool_forward")
    return m


def loop_pool_backward(x: torch.Tensor, B: int, L: int, W1: torch.Tensor, b1: torch.Tensor, g: torch.Tensor):
    """-> (dW1 (E,E), db1 (E)) from g = dL/dm (B,E) and the forward's operands.  Deterministic; x gets no gradient."""
    E = _loop_pool_args(x, B, L, W1, b1)
    _chk(g, torch.float32, "g"), _shape(g, (B, E), "g")
    lib = _lib.load()
    ws = torch.empty(lib.dpm_loop_pool_workspace_bytes(B, L, E), device=x.device, dtype=torch.uint8)
    dW1 = torch.empty(E, E, device=x.device, dtype=torch.float32)
    db1 = torch.empty(E, device=x.device, dtype=torch.float32)
    _lib.check(lib.dpm_loop_pool_backward(_ptr(x), x.stride(0), _ptr(W1), _ptr(b1), _ptr(g), B, L, E, _ptr(dW1), _ptr(db1),
                                          _ptr(ws), _stream(x)), "dpm_loop_pool_backward")
    return dW1, db1


class _LoopPool(torch.autograd.Function):
    """Saved for the backward: x, W1, b1 -- nothing of B * L * E elements besides the input itself."""

    @staticmethod
    def forward(ctx, x, B, L, W1, b1):
        W1c, b1c = W1.detach().contiguous(), b1.detach().contiguous()
        m = loop_pool_forward(x, B, L, W1c, b1c)
        ctx.save_for_backward(x, W1c, b1c)
        ctx.cfg = (B, L)
        return m

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        x, W1, b1 = ctx.saved_tensors
        dW1, db1 = loop_pool_backward(x, *ctx.cfg, W1, b1, g.contiguous())
        return None, None, None, dW1, db1


def loop_pool(x: torch.Tensor, B: int, L: int, W1: torch.Tensor, b1: torch.Tensor) -> torch.Tensor:
    """mean over the tokens of relu(x W1^T + b1): x (B*L, E) fp32 row view (a column slice of a wider buffer is allowed, rows
    16-byte aligned), W1 (E,E), b1 (E) -> (B,E), differentiable with respect to W1 and b1 ONLY -- x is the output of a frozen
    trunk and gets no gradient.  The mean runs over all L tokens.  Forward and backward run in csrc/loop_head_train.hip: the
    (B*L, E) pre-activation exists in neither direction, the backward recomputes it with the forward's instruction sequence
    (the same ReLU mask, bit for bit), and two runs give identical bytes.  E = 256 only (ValueError otherwise)."""
    return _LoopPool.apply(x, B, L, W1, b1)


class _LoopBce(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, target):
        p, y = pred.detach().contiguous(), target.detach().contiguous()
        dev = p.device
        loss = torch.empty((), device=dev, dtype=torch.float32)
        stats = torch.empty(8, device=dev, dtype=torch.float32)
        unit = torch.empty_like(p)
        _lib.check(_lib.load().dpm_loop_bce_forward(_ptr(p), _ptr(y), p.numel(), _ptr(loss), _ptr(stats), _ptr(unit), _stream(p)),
                   "dpm_loop_bce_forward")
        ctx.save_for_backward(unit)
        ctx.mark_non_differentiable(stats)
        return loss, stats

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_loss, _grad_stats):
        unit, = ctx.saved_tensors
        return grad_loss * unit, None


def loop_bce(pred: torch.Tensor, target: torch.Tensor):
    """F.binary_cross_entropy(pred, target) of (B,) fp32 probabilities and 0 / 1 labels (mean reduction, both logarithms clamped
    at -100) -> (loss 0-d, stats (8,)), one launch: stats = [loss, n_pos, n_neg, n_equal, true_pos, false_pos, 0, 0] with the
    prediction `pred > 0.5` (model_pipeline.py:160-173).  loss is differentiable with respect to pred, by torch's formula
    grad (p - t) / max(p (1 - p), 1e-12) / B; stats is not differentiable."""
    _chk(pred.detach(), torch.float32, "pred"), _chk(target.detach(), torch.float32, "target")
    if pred.dim() != 1 or pred.numel() < 1:
        raise ValueError(f"pred must be (B,) with B >= 1, got {tuple(pred.shape)}")
    _shape(target, pred.shape, "target")
    return _LoopBce.apply(pred, target)


# ---- the dense layers for training (csrc/dense_train.hip) ----------------------------------------------------------------------

def _dense_check(t, shape, name: str) -> None:
    """shape (None = any leading dimensions, then the given ones) and dtype -> ValueError"""
    ok = isinstance(t, torch.Tensor) and t.dim() >= len(shape) and all(
        w is None or w == g for w, g in zip(shape, t.shape[t.dim() - len(shape):])) and (shape[0] is None or t.dim() == len(shape))
    if not ok:
        want = ", ".join("..." if w is None else str(w) for w in shape)
        raise ValueError(f"{name}: expected ({want}), got {tuple(t.shape) if isinstance(t, torch.Tensor) else type(t)}")
    if t.dtype != torch.float32:
        raise ValueError(f"{name}: expected torch.float32, got {t.dtype}")


def _dense_rows(t: torch.Tensor, cols: int, name: str) -> torch.Tensor:
    """(..., cols) fp32 on the GPU -> a (rows, cols) view with last-dimension stride 1 (a copy only where no such view exists)"""
    if not t.is_cuda:
        raise _lib.DpmError(f"{name}: expected a tensor on the GPU, got {t.device} (no CPU fallback)")
    t = t.detach().reshape(-1, cols)
    if t.stride(1) != 1 or (t.shape[0] > 1 and t.stride(0) < cols):
        t = t.contiguous()
    return t


def _dense_ld(t: torch.Tensor) -> int:
    return max(t.stride(0), t.shape[1]) if t.shape[0] > 1 else t.shape[1]


def _dense_args(x, W, bias, residual, gamma, beta, post, act: int, what: str):
    if act not in (ACT_NONE, ACT_RELU):
        raise ValueError(f"{what}: act must be ACT_NONE or ACT_RELU, got {act}")
    if not isinstance(W, torch.Tensor) or W.dim() != 2 or W.shape[0] < 1 or W.shape[1] < 1:
        raise ValueError(f"{what}: W must be (Cout >= 1, Cin >= 1), got {tuple(W.shape) if isinstance(W, torch.Tensor) else type(W)}")
    Cout, Cin = W.shape
    _dense_check(W, (Cout, Cin), "W")
    _dense_check(x, (None, Cin), "x")
    lead = tuple(x.shape[:-1])
    for t, name in ((bias, "bias"), (gamma, "gamma"), (beta, "beta")):
        if t is not None:
            _dense_check(t, (Cout,), name)
    for t, name in ((residual, "residual"), (post, "post")):
        if t is not None:
            _dense_check(t, lead + (Cout,), name)
    for t, name in ((W, "W"), (bias, "bias"), (gamma, "gamma"), (beta, "beta"), (residual, "residual"), (post, "post")):
        if t is not None and t.device != x.device:
            raise ValueError(f"{what}: x on {x.device}, {name} on {t.device}")
    vec = lambda t, name: None if t is None else _dense_rows(t, Cout, name).reshape(Cout).contiguous()   # noqa: E731
    rows = lambda t, name: None if t is None else _dense_rows(t, Cout, name).contiguous()                # noqa: E731
    return (_dense_rows(x, Cin, "x"), _dense_rows(W, Cin, "W"), vec(bias, "bias"), rows(residual, "residual"), vec(gamma, "gamma"),
            vec(beta, "beta"), rows(post, "post"), lead)


def _dense_ws(lib, R: int, Cin: int, Cout: int, dev) -> torch.Tensor:
    return torch.empty(lib.dpm_dense_train_workspace_bytes(R, Cin, Cout), device=dev, dtype=torch.uint8)


def _dense_backward_gemm(dh, x, W, need_x: bool, need_W: bool, need_b: bool):
    """dh (R, Cout) contiguous -> (dx (R, Cin) | None, dW (Cout, Cin) | None, dbias (Cout) | None)"""
    R, (Cout, Cin) = x.shape[0], W.shape
    lib, dev = _lib.load(), dh.device
    dx = torch.empty(R, Cin, device=dev, dtype=torch.float32) if need_x else None
    dW = torch.empty(Cout, Cin, device=dev, dtype=torch.float32) if (need_W or need_b) else None
    db = torch.empty(Cout, device=dev, dtype=torch.float32) if need_b else None
    if dx is not None or dW is not None:
        ws = _dense_ws(lib, R, Cin, Cout, dev) if dW is not None else None
        _lib.check(lib.dpm_dense_train_backward_gemm(_ptr(dh), _ptr(x), _dense_ld(x), _ptr(W), _dense_ld(W), R, Cin, Cout, _ptr(dx),
                                                     _ptr(dW), _ptr(db), _ptr(ws), _stream(dh)), "dpm_dense_train_backward_gemm")
    return dx, (dW if need_W else None), db


def _dense_forward(x, W, bias, gamma, beta, residual, post, act: int):
    """-> (out, h, stats, (the row views of x and W and the contiguous gamma the kernels read))"""
    normed = gamma is not None
    if normed != (beta is not None) or (post is not None and not normed):
        raise ValueError("dense_train_forward: gamma and beta come together, post needs them")
    xv, Wv, bv, rv, gv, bev, pv, lead = _dense_args(x, W, bias, residual, gamma, beta, post, act, "dense_train_forward")
    R, (Cout, Cin) = xv.shape[0], Wv.shape
    dev = xv.device
    out = torch.empty(R, Cout, device=dev, dtype=torch.float32)
    h = torch.empty(R, Cout, device=dev, dtype=torch.float32) if normed else None
    stats = torch.empty(R, 2, device=dev, dtype=torch.float32) if normed else None
    _lib.check(_lib.load().dpm_dense_train_forward(_ptr(xv), _dense_ld(xv), _ptr(Wv), _dense_ld(Wv), _ptr(bv), _ptr(rv), _ptr(gv),
                                                   _ptr(bev), _ptr(pv), R, Cin, Cout, act, _ptr(out), _ptr(h), _ptr(stats),
                                                   _stream(xv)), "dpm_dense_train_forward")
    return out.view(lead + (Cout,)), h, stats, (xv, Wv, gv)


def dense_train_forward(x, W, bias=None, gamma=None, beta=None, residual=None, post=None, act: int = ACT_NONE):
    """The forward of both forms without a graph -> (out (..., Cout), h (R, Cout), stats (R, 2)); normed when gamma is given, else
    h and stats are None.  h = x W^T + bias + residual: the same bits in both forms.  stats = (mean, rstd) per row."""
    return _dense_forward(x, W, bias, gamma, beta, residual, post, act)[:3]


class _DenseLinear(torch.autograd.Function):
    """Saved for the backward: x, W and, with ReLU, the output (its sign is the mask)."""

    @staticmethod
    def forward(ctx, x, W, bias, residual, act):
        out, _, _, (xv, Wv, _) = _dense_forward(x, W, bias, None, None, residual, None, act)
        ctx.save_for_backward(xv, Wv, out.view(xv.shape[0], Wv.shape[0]) if act == ACT_RELU else None)
        ctx.cfg = (act, tuple(x.shape), tuple(W.shape), tuple(out.shape))
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy):
        xv, Wv, out = ctx.saved_tensors
        act, xshape, wshape, oshape = ctx.cfg
        need_x, need_W, need_b, need_r = ctx.needs_input_grad[:4]
        R, Cout = xv.shape[0], Wv.shape[0]
        g = dy.reshape(R, Cout).contiguous()
        if act == ACT_RELU:
            gm = torch.empty_like(g)
            _lib.check(_lib.load().dpm_dense_train_backward_rows(_ptr(g), _ptr(out), None, None, None, R, Cout, act, _ptr(gm), None, None,
                                                                 None, None, _stream(g)), "dpm_dense_train_backward_rows")
            g = gm
        dx, dW, db = _dense_backward_gemm(g, xv, Wv, need_x, need_W, need_b)
        return (None if dx is None else dx.view(xshape), None if dW is None else dW.view(wshape), db,
                g.view(oshape) if need_r else None, None)


def dense_linear_train(x: torch.Tensor, W: torch.Tensor, bias: Optional[torch.Tensor] = None, residual: Optional[torch.Tensor] = None,
                       act: int = ACT_NONE) -> torch.Tensor:
    """act(x W^T + bias + residual) with a backward, both in csrc/dense_train.hip: x (..., Cin) fp32 (a column slice of a wider
    buffer is used in place), W (Cout, Cin) (a column slice likewise: any row stride, any alignment), bias (Cout), residual
    (..., Cout), act ACT_NONE or ACT_RELU -> (..., Cout).  Differentiable with respect to x, W, bias and residual; each gradient is
    computed only when it is needed.  Exact fp32 products, every sum in one order: two runs give identical bytes.  Operands whose
    last-dimension stride is not 1 are copied.  ValueError for shape or dtype mismatches."""
    return _DenseLinear.apply(x, W, bias, residual, act)


class _DenseLinearLN(torch.autograd.Function):
    """Saved for the backward: x, W, gamma, the pre-norm rows h, (mean, rstd) per row and, with ReLU, the output."""

    @staticmethod
    def forward(ctx, x, W, bias, gamma, beta, residual, post, act):
        if gamma is None or beta is None:
            raise ValueError("dense_linear_ln_train: gamma and beta are required")
        out, h, stats, (xv, Wv, gv) = _dense_forward(x, W, bias, gamma, beta, residual, post, act)
        ctx.save_for_backward(xv, Wv, gv, h, stats, out.view(xv.shape[0], Wv.shape[0]) if act == ACT_RELU else None)
        ctx.cfg = (act, tuple(x.shape), tuple(W.shape), tuple(out.shape))
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy):
        xv, Wv, gv, h, stats, out = ctx.saved_tensors
        act, xshape, wshape, oshape = ctx.cfg
        need_x, need_W, need_b, need_g, need_be, need_r, need_p = ctx.needs_input_grad[:7]
        R, (Cout, Cin) = xv.shape[0], Wv.shape
        lib, dev = _lib.load(), xv.device
        dy = dy.reshape(R, Cout).contiguous()
        if act == ACT_NONE and need_p:
            g = None                      # d post is dy itself
        else:
            g = torch.empty_like(dy) if need_p else None
        dh = torch.empty_like(dy)
        affine = need_g or need_be
        dgamma = torch.empty(Cout, device=dev, dtype=torch.float32) if affine else None
        dbeta = torch.empty(Cout, device=dev, dtype=torch.float32) if affine else None
        ws = _dense_ws(lib, R, Cin, Cout, dev) if affine else None
        _lib.check(lib.dpm_dense_train_backward_rows(_ptr(dy), _ptr(out), _ptr(h), _ptr(stats), _ptr(gv), R, Cout, act, _ptr(g), _ptr(dh),
                                                     _ptr(dgamma), _ptr(dbeta), _ptr(ws), _stream(dy)), "dpm_dense_train_backward_rows")
        dx, dW, db = _dense_backward_gemm(dh, xv, Wv, need_x, need_W, need_b)
        dpost = None if not need_p else (dy if g is None else g).view(oshape)
        return (None if dx is None else dx.view(xshape), None if dW is None else dW.view(wshape), db,
                dgamma if need_g else None, dbeta if need_be else None, dh.view(oshape) if need_r else None, dpost, None)


def dense_linear_ln_train(x: torch.Tensor, W: torch.Tensor, bias: Optional[torch.Tensor], gamma: torch.Tensor, beta: torch.Tensor,
                          residual: Optional[torch.Tensor] = None, post: Optional[torch.Tensor] = None,
                          act: int = ACT_NONE) -> torch.Tensor:
    """act(LN(x W^T + bias + residual) * gamma + beta + post) (eps 1e-5, biased variance) with a backward, both in
    csrc/dense_train.hip; operands as for dense_linear_train, gamma, beta (Cout), post (..., Cout).  Differentiable with respect to
    x, W, bias, gamma, beta, residual and post; each gradient is computed only when it is needed.  Widths 32, 64, 128, 256 normalise
    in the product kernel's epilogue, other widths in a row kernel after it; the pre-norm rows are the bits dense_linear_train gives
    for the same operands either way.  Two runs give identical bytes.  ValueError for shape or dtype mismatches."""
    return _DenseLinearLN.apply(x, W, bias, gamma, beta, residual, post, act)


# ---- the map assembly of the registration training step (csrc/map_assemble.hip) -------------------------------------------------
def _map_split(F: int, S: int, S1: int, what: str) -> int:
    if S < 2 or not 1 <= S1 < S or F < S or F % S:
        raise ValueError(f"{what}: needs F = B * S frames with S >= 2 and 1 <= S1 < S, got F = {F}, S = {S}, S1 = {S1}")
    return F // S


def map_poses(R: torch.Tensor, T: torch.Tensor, calib: torch.Tensor, icp: torch.Tensor, has_icp: torch.Tensor, S: int, S1: int):
    """R (F,3,3), T (F,3,1), calib (F,4,4) fp32: the global poses and calibrations of F = B * S frames; icp (F+B,16) fp32,
    has_icp (F+B,) uint8: the refined poses the host found (train_pipeline.icp_table) -> rel (F,12), gt (B,12), rows [R | T]
    (3x4): frame (b,s) into its map's first frame (frame 0 for s < S1, frame S1 otherwise; those two get the exact identity)
    and map b's source-first into its target-first.  With has_icp: d_calib @ icp @ inverse(s_calib); otherwise
    rt_global_to_relative.  One launch, no host round trip.  A singular calib is not supported (Inf / NaN)."""
    for t, name in ((R, "R"), (T, "T"), (calib, "calib"), (icp, "icp")):
        _chk(t, torch.float32, name)
    _chk(has_icp, torch.uint8, "has_icp")
    F = R.shape[0]
    B = _map_split(F, S, S1, "map_poses")
    _shape(R, (F, 3, 3), "R"), _shape(T, (F, 3, 1), "T"), _shape(calib, (F, 4, 4), "calib")
    _shape(icp, (F + B, 16), "icp"), _shape(has_icp, (F + B,), "has_icp")
    rel = torch.empty(F, 12, device=R.device, dtype=torch.float32)
    gt = torch.empty(B, 12, device=R.device, dtype=torch.float32)
    _lib.check(_lib.load().dpm_map_poses(_ptr(R), _ptr(T), _ptr(calib), _ptr(icp), _ptr(has_icp), B, S, S1, _ptr(rel), _ptr(gt),
                                         _stream(R)), "dpm_map_poses")
    return rel, gt


def map_assemble_forward(coor, fea, mask, rel, gt, S: int, S1: int, coor_scale: float):
    for t, name in ((coor, "coor"), (fea, "fea"), (rel, "rel"), (gt, "gt")):
        _chk(t, torch.float32, name)
    m = _chk(mask.view(torch.uint8) if mask.dtype == torch.bool else mask, torch.uint8, "mask")   # same bytes
    F, C, N = fea.shape
    B = _map_split(F, S, S1, "map_assemble")
    _shape(coor, (F, 3, N), "coor"), _shape(m, (F, N), "mask"), _shape(rel, (F, 12), "rel"), _shape(gt, (B, 12), "gt")
    if N < 1 or C < 1:
        raise ValueError(f"map_assemble: needs N >= 1 points and C >= 1 channels, got N = {N}, C = {C}")
    dev, S2 = fea.device, S - S1
    new = lambda *shape, dtype=torch.float32: torch.empty(*shape, device=dev, dtype=dtype)   # noqa: E731
    src_desc, dst_desc = new(B, C + 3, S1 * N), new(B, C + 3, S2 * N)
    src_mask, dst_mask = new(B, S1 * N, dtype=torch.uint8), new(B, S2 * N, dtype=torch.uint8)
    src_global, dst_global = new(B, 3, S1 * N), new(B, 3, S2 * N)
    _lib.check(_lib.load().dpm_map_assemble_fwd(_ptr(coor), _ptr(fea), _ptr(m), _ptr(rel), _ptr(gt), B, S, S1, N, C,
                                                float(coor_scale), _ptr(src_desc), _ptr(dst_desc), _ptr(src_mask), _ptr(dst_mask),
                                                _ptr(src_global), _ptr(dst_global), _stream(fea)), "dpm_map_assemble_fwd")
    return src_desc, dst_desc, src_mask.view(torch.bool), dst_mask.view(torch.bool), src_global, dst_global


def map_assemble_backward(d_src_desc, d_dst_desc, F: int, C: int, N: int, S: int, S1: int) -> torch.Tensor:
    """dfea (F,C,N) from the gradients of the two descriptors (either may be None: zeros); a gather, exact and repeatable"""
    B = _map_split(F, S, S1, "map_assemble")
    ref = d_src_desc if d_src_desc is not None else d_dst_desc
    if ref is None:
        raise ValueError("map_assemble_backward: no gradient given")
    for t, name, Sx in ((d_src_desc, "d_src_desc", S1), (d_dst_desc, "d_dst_desc", S - S1)):
        if t is not None:
            _chk(t, torch.float32, name), _shape(t, (B, C + 3, Sx * N), name)
    dfea = torch.empty(F, C, N, device=ref.device, dtype=torch.float32)
    _lib.check(_lib.load().dpm_map_assemble_bwd(_ptr(d_src_desc), _ptr(d_dst_desc), B, S, S1, N, C, _ptr(dfea), _stream(ref)),
               "dpm_map_assemble_bwd")
    return dfea


class _MapAssemble(torch.autograd.Function):
    @staticmethod
    def forward(ctx, fea, coor, mask, rel, gt, S, S1, coor_scale):
        outs = map_assemble_forward(coor, fea.detach().contiguous(), mask, rel, gt, S, S1, coor_scale)
        ctx.cfg = (*fea.shape, S, S1)
        ctx.mark_non_differentiable(*outs[2:])
        return outs

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, d_src, d_dst, *_):
        F, C, N, S, S1 = ctx.cfg
        dfea = map_assemble_backward(None if d_src is None else d_src.contiguous(), None if d_dst is None else d_dst.contiguous(),
                                     F, C, N, S, S1)
        return dfea, None, None, None, None, None, None, None


def map_assemble(coor: torch.Tensor, fea: torch.Tensor, mask: torch.Tensor, rel: torch.Tensor, gt: torch.Tensor, S: int, S1: int,
                 coor_scale: float):
    """model_pipeline.py:40-104 after the poses: coor (F,3,N) unscaled, fea (F,C,N), mask (F,N) bool of F = B * S encoded frames,
    rel (F,12), gt (B,12) from map_poses -> (src_desc (B,C+3,S1*N), dst_desc (B,C+3,S2*N), src_mask (B,S1*N), dst_mask (B,S2*N),
    src_global (B,3,S1*N), dst_global (B,3,S2*N)), S2 = S - S1: what the decoder and the criterion take.  Token s*N + n of a
    map is point n of its frame s; feature rows first, then xyz = rel_R @ (coor * coor_scale) + rel_T (a map's first frame:
    coor * coor_scale and nothing else); src_global = gt_R @ src_xyz + gt_T.  One launch forward, one backward.
    Differentiable with respect to fea ONLY: the xyz rows and coor get no gradient (the decoder's rule), and the
    backward is a gather of the two descriptor gradients' feature rows -- exact, identical bytes on every run."""
    return _MapAssemble.apply(fea, coor, mask, rel, gt, S, S1, coor_scale)


# ------------------------------------------------------------------------------------------------------------
# batched frame ingest (csrc/ingest.hip)
# ------------------------------------------------------------------------------------------------------------
INGEST_CHUNK = 4096   # records per compaction block of csrc/ingest.hip (the entry point refuses any other value)


def ingest_layout(shapes):
    """shapes: per frame (rows, stride in floats).  -> (per-frame offsets in 32-bit words from the start of the staging
    block, size of the block in bytes): the header of F x 4 int64, then the frames' records back to back."""
    off, offsets = 8 * len(shapes), []
    for rows, stride in shapes:
        offsets.append(off)
        off += int(rows) * int(stride)
    return offsets, 4 * off


def ingest_stage(frames, block: Optional[torch.Tensor] = None) -> torch.Tensor:
    """frames: per frame (rows (n,stride) float32 numpy array of whole records, drop_nan) -> the staging block of
    dpm_ingest_frames, a uint8 host tensor (pinned when it is allocated here).  `block`: a staging slot to fill instead
    (it must be large enough; the filled prefix is returned)."""
    import numpy as np
    shapes = []
    for rows, _ in frames:
        if rows.dtype != np.float32 or rows.ndim != 2 or rows.shape[1] < 3:
            raise ValueError("a frame's records are a float32 array (rows, stride >= 3)")
        shapes.append(rows.shape)
    offsets, nbytes = ingest_layout(shapes)
    if block is None:
        block = torch.empty(nbytes, dtype=torch.uint8, pin_memory=torch.cuda.is_available())
    elif block.dtype != torch.uint8 or block.is_cuda or not block.is_contiguous() or block.numel() < nbytes:
        raise ValueError(f"the staging slot must be a contiguous uint8 host tensor of at least {nbytes} bytes")
    block = block[:nbytes]
    view = block.numpy()
    header = view[:32 * len(frames)].view(np.int64).reshape(len(frames), 4)
    words = view.view(np.float32)
    for f, ((rows, drop_nan), off) in enumerate(zip(frames, offsets)):
        header[f] = (off, rows.shape[0], rows.shape[1], int(bool(drop_nan)))
        words[off:off + rows.size].reshape(rows.shape)[...] = rows   # a plain copy: the bytes of every float survive
    return block


def ingest_frames(block: torch.Tensor, F: int, capacity: int, device=None, staging_dev: Optional[torch.Tensor] = None):
    """One asynchronous copy of the staging block (ingest_stage) and three launches on the current stream, no host
    synchronisation: -> xyz (F,capacity,3) fp32 = the kept records' first three floats as bits, in input order, zero at and
    past the count; idx (F,capacity) int32 = 0..capacity-1; count (F,) int32.  Frame f equals
    PointCloud(reader's filtered array, capacity=capacity) byte for byte (augment.PointCloud.from_buffers wraps it).
    A row count above `capacity` raises ValueError before anything is queued.  The caller leaves `block` untouched until
    the stream has passed the copy; `staging_dev`: device bytes to copy into (allocated here otherwise)."""
    import numpy as np
    F, capacity = int(F), int(capacity)
    if block.dtype != torch.uint8 or block.is_cuda or not block.is_contiguous() or block.numel() < 32 * F or F < 1:
        raise ValueError("block: a contiguous uint8 host tensor from ingest_stage holding F >= 1 frames")
    header = block.numpy()[:32 * F].view(np.int64).reshape(F, 4)
    for f in range(F):
        if header[f, 1] > capacity:
            raise ValueError(f"frame {f} has {int(header[f, 1])} records, more than the capacity {capacity}")
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    with torch.cuda.device(dev):
        if staging_dev is None:
            staging_dev = torch.empty(block.numel(), device=dev, dtype=torch.uint8)
        _chk(staging_dev, torch.uint8, "staging_dev")
        if staging_dev.numel() < block.numel():
            raise ValueError("staging_dev is smaller than the staging block")
        xyz = torch.empty(F, capacity, 3, device=dev, dtype=torch.float32)
        idx = torch.empty(F, capacity, device=dev, dtype=torch.int32)
        count = torch.empty(F, device=dev, dtype=torch.int32)
        ws = torch.empty(F * ((capacity + INGEST_CHUNK - 1) // INGEST_CHUNK), device=dev, dtype=torch.int32)
        _lib.check(_lib.load().dpm_ingest_frames(block.data_ptr(), _ptr(staging_dev), block.numel(), F, capacity, INGEST_CHUNK,
                                                 _ptr(xyz), _ptr(idx), _ptr(count), _ptr(ws), _stream(xyz)), "dpm_ingest_frames")
    return xyz, idx, count


# ------------------------------------------------------------------------------------------------------------
# LiDAR simulator (csrc/lidar_sim.hip)
# ------------------------------------------------------------------------------------------------------------
LIDAR_REC = 16        # floats of a kept record
LIDAR_PRIM = 10       # doubles of a scene primitive
LIDAR_COL = 12        # floats per column of a sweep table
LIDAR_BOX, LIDAR_CYLINDER = 0, 1
LIDAR_MAX_RAYS = 1 << 24


def _lidar_arg(t, dtype, name: str, shape_ok: bool, shape: str):
    """dtype (TypeError) and shape (ValueError) before the device: a host-side mistake is reported without a GPU"""
    if t.dtype != dtype:
        raise TypeError(f"{name}: expected {dtype}, got {t.dtype}")
    if not shape_ok:
        raise ValueError(f"{name}: expected {shape}, got {tuple(t.shape)}")
    return t


def _lidar_dev(**tensors):
    for name, t in tensors.items():
        if t is not None:
            _chk(t, t.dtype, name)


def lidar_cull(prims: torch.Tensor, kind: torch.Tensor, ground: torch.Tensor, poses: torch.Tensor, max_range: float,
               max_kept: int):
    """dpm_lidar_cull: prims (P,10) float64, kind (P,) int32, ground (2,) float64, poses (F,4,4) float64 sensor-to-world ->
    kept (F,max_kept,16) fp32 sensor-frame records in ascending primitive index, plane (F,4) fp32, status (F,2) int32 =
    (primitives in range, overflow flag).  One launch, no host synchronisation: the CALLER raises on the flag at read-back."""
    max_kept = int(max_kept)
    if max_kept < 1 or not float(max_range) > 0:
        raise ValueError("max_kept >= 1 and max_range > 0")
    _lidar_arg(prims, torch.float64, "prims", prims.dim() == 2 and prims.shape[1] == LIDAR_PRIM, f"(P,{LIDAR_PRIM})")
    _lidar_arg(kind, torch.int32, "kind", kind.shape == prims.shape[:1], "(P,)")
    _lidar_arg(ground, torch.float64, "ground", ground.shape == (2,), "(2,)")
    _lidar_arg(poses, torch.float64, "poses", poses.dim() == 3 and poses.shape[1:] == (4, 4) and poses.shape[0] >= 1, "(F,4,4), F >= 1")
    _lidar_dev(prims=prims, kind=kind, ground=ground, poses=poses)
    P, F, dev = prims.shape[0], poses.shape[0], poses.device
    with torch.cuda.device(dev):
        kept = torch.empty(F, max_kept, LIDAR_REC, device=dev, dtype=torch.float32)
        plane = torch.empty(F, 4, device=dev, dtype=torch.float32)
        status = torch.empty(F, 2, device=dev, dtype=torch.int32)
        _lib.check(_lib.load().dpm_lidar_cull(_ptr(prims), _ptr(kind), P, _ptr(ground), _ptr(poses), F, float(max_range),
                                              max_kept, _ptr(kept), _ptr(plane), _ptr(status), _stream(poses)), "dpm_lidar_cull")
    return kept, plane, status


def lidar_cast(kept: torch.Tensor, plane: torch.Tensor, status: torch.Tensor, P: int, dirs: torch.Tensor, min_range: float,
               max_range: float):
    """dpm_lidar_cast: the outputs of lidar_cull, P = the scene's primitive count (the ground's id), dirs (rays,3) fp32
    unit directions -> range (F,rays) fp32, prim (F,rays) int32 (index, P = ground, -1 = no return), cos_inc (F,rays)."""
    if not 0.0 <= float(min_range) < float(max_range) or int(P) < 0:
        raise ValueError("0 <= min_range < max_range and P >= 0")
    _lidar_arg(kept, torch.float32, "kept", kept.dim() == 3 and kept.shape[2] == LIDAR_REC and kept.shape[0] >= 1 and kept.shape[1] >= 1,
               f"(F,max_kept,{LIDAR_REC})")
    F, max_kept = kept.shape[:2]
    _lidar_arg(plane, torch.float32, "plane", plane.shape == (F, 4), "(F,4)")
    _lidar_arg(status, torch.int32, "status", status.shape == (F, 2), "(F,2)")
    _lidar_arg(dirs, torch.float32, "dirs", dirs.dim() == 2 and dirs.shape[1] == 3 and 1 <= dirs.shape[0] <= LIDAR_MAX_RAYS,
               "(rays,3), 1 <= rays <= 2^24")
    _lidar_dev(kept=kept, plane=plane, status=status, dirs=dirs)
    rays, dev = dirs.shape[0], kept.device
    with torch.cuda.device(dev):
        rng = torch.empty(F, rays, device=dev, dtype=torch.float32)
        prim = torch.empty(F, rays, device=dev, dtype=torch.int32)
        cos_inc = torch.empty(F, rays, device=dev, dtype=torch.float32)
        _lib.check(_lib.load().dpm_lidar_cast(_ptr(kept), _ptr(plane), _ptr(status), max_kept, int(P), _ptr(dirs), rays, F,
                                              float(min_range), float(max_range), _ptr(rng), _ptr(prim), _ptr(cos_inc),
                                              _stream(kept)), "dpm_lidar_cast")
    return rng, prim, cos_inc


def lidar_cull_sweep(prims: torch.Tensor, kind: torch.Tensor, ground: torch.Tensor, poses0: torch.Tensor, poses1: torch.Tensor,
                     azimuth_steps: int, max_range: float, max_kept: int):
    """dpm_lidar_cull_sweep: lidar_cull about poses0 for a sensor that moves to poses1 (F,4,4) float64 during the sweep: the
    max_range ball grows by the travel -> kept, plane, status as lidar_cull, and table (F,azimuth_steps,12) fp32 = per
    column the rotation Exp(s_c w) (9) and the origin s_c t_D (3) in the frame of poses0."""
    max_kept, A = int(max_kept), int(azimuth_steps)
    if max_kept < 1 or not float(max_range) > 0 or not 1 <= A <= LIDAR_MAX_RAYS:
        raise ValueError("max_kept >= 1, max_range > 0 and 1 <= azimuth_steps <= 2^24")
    _lidar_arg(prims, torch.float64, "prims", prims.dim() == 2 and prims.shape[1] == LIDAR_PRIM, f"(P,{LIDAR_PRIM})")
    _lidar_arg(kind, torch.int32, "kind", kind.shape == prims.shape[:1], "(P,)")
    _lidar_arg(ground, torch.float64, "ground", ground.shape == (2,), "(2,)")
    _lidar_arg(poses0, torch.float64, "poses0", poses0.dim() == 3 and poses0.shape[1:] == (4, 4) and poses0.shape[0] >= 1, "(F,4,4), F >= 1")
    _lidar_arg(poses1, torch.float64, "poses1", poses1.shape == poses0.shape, "(F,4,4)")
    _lidar_dev(prims=prims, kind=kind, ground=ground, poses0=poses0, poses1=poses1)
    P, F, dev = prims.shape[0], poses0.shape[0], poses0.device
    with torch.cuda.device(dev):
        kept = torch.empty(F, max_kept, LIDAR_REC, device=dev, dtype=torch.float32)
        plane = torch.empty(F, 4, device=dev, dtype=torch.float32)
        status = torch.empty(F, 2, device=dev, dtype=torch.int32)
        table = torch.empty(F, A, LIDAR_COL, device=dev, dtype=torch.float32)
        _lib.check(_lib.load().dpm_lidar_cull_sweep(_ptr(prims), _ptr(kind), P, _ptr(ground), _ptr(poses0), _ptr(poses1), F, A,
                                                    float(max_range), max_kept, _ptr(kept), _ptr(plane), _ptr(status),
                                                    _ptr(table), _stream(poses0)), "dpm_lidar_cull_sweep")
    return kept, plane, status, table


def lidar_cast_sweep(kept: torch.Tensor, plane: torch.Tensor, status: torch.Tensor, table: torch.Tensor, P: int,
                     dirs: torch.Tensor, min_range: float, max_range: float):
    """dpm_lidar_cast_sweep: lidar_cast over the outputs of lidar_cull_sweep; ray r fires from column r % azimuth_steps of the
    table (rays a multiple of azimuth_steps); range is measured from the sensor's origin at the ray's own time."""
    if not 0.0 <= float(min_range) < float(max_range) or int(P) < 0:
        raise ValueError("0 <= min_range < max_range and P >= 0")
    _lidar_arg(kept, torch.float32, "kept", kept.dim() == 3 and kept.shape[2] == LIDAR_REC and kept.shape[0] >= 1 and kept.shape[1] >= 1,
               f"(F,max_kept,{LIDAR_REC})")
    F, max_kept = kept.shape[:2]
    _lidar_arg(plane, torch.float32, "plane", plane.shape == (F, 4), "(F,4)")
    _lidar_arg(status, torch.int32, "status", status.shape == (F, 2), "(F,2)")
    _lidar_arg(dirs, torch.float32, "dirs", dirs.dim() == 2 and dirs.shape[1] == 3 and 1 <= dirs.shape[0] <= LIDAR_MAX_RAYS,
               "(rays,3), 1 <= rays <= 2^24")
    rays = dirs.shape[0]
    _lidar_arg(table, torch.float32, "table", table.dim() == 3 and table.shape[0] == F and table.shape[2] == LIDAR_COL
               and table.shape[1] >= 1 and rays % table.shape[1] == 0, f"(F,azimuth_steps,{LIDAR_COL}), azimuth_steps dividing rays")
    _lidar_dev(kept=kept, plane=plane, status=status, table=table, dirs=dirs)
    dev = kept.device
    with torch.cuda.device(dev):
        rng = torch.empty(F, rays, device=dev, dtype=torch.float32)
        prim = torch.empty(F, rays, device=dev, dtype=torch.int32)
        cos_inc = torch.empty(F, rays, device=dev, dtype=torch.float32)
        _lib.check(_lib.load().dpm_lidar_cast_sweep(_ptr(kept), _ptr(plane), _ptr(status), max_kept, int(P), _ptr(dirs), rays, F,
                                                    _ptr(table), table.shape[1], float(min_range), float(max_range), _ptr(rng),
                                                    _ptr(prim), _ptr(cos_inc), _stream(kept)), "dpm_lidar_cast_sweep")
    return rng, prim, cos_inc


def lidar_emit(rng: torch.Tensor, prim: torch.Tensor, cos_inc: torch.Tensor, dirs: torch.Tensor, albedo: torch.Tensor,
               class_id: torch.Tensor, noise: Optional[torch.Tensor] = None, u: Optional[torch.Tensor] = None,
               drop_prob: float = 0.0):
    """dpm_lidar_emit: the outputs of lidar_cast, albedo (P+1,) fp32 and class_id (P+1,) int32 with the ground last, optional
    noise / u (F,rays) fp32 -> xyz (F,rays,3), idx (F,rays) ray indices, count (F,), intensity (F,rays), label (F,rays)."""
    if not 0.0 <= float(drop_prob) <= 1.0:
        raise ValueError("drop_prob in [0, 1]")
    _lidar_arg(rng, torch.float32, "range", rng.dim() == 2 and rng.shape[0] >= 1 and 1 <= rng.shape[1] <= LIDAR_MAX_RAYS,
               "(F,rays), F >= 1, 1 <= rays <= 2^24")
    F, rays = rng.shape
    _lidar_arg(prim, torch.int32, "prim", prim.shape == rng.shape, "(F,rays)")
    _lidar_arg(cos_inc, torch.float32, "cos_inc", cos_inc.shape == rng.shape, "(F,rays)")
    _lidar_arg(dirs, torch.float32, "dirs", dirs.shape == (rays, 3), "(rays,3)")
    _lidar_arg(albedo, torch.float32, "albedo", albedo.dim() == 1 and albedo.shape[0] >= 1, "(P+1,)")
    _lidar_arg(class_id, torch.int32, "class_id", class_id.shape == albedo.shape, "(P+1,)")
    for name, t in (("noise", noise), ("u", u)):
        if t is not None:
            _lidar_arg(t, torch.float32, name, t.shape == rng.shape, "(F,rays)")
    _lidar_dev(range=rng, prim=prim, cos_inc=cos_inc, dirs=dirs, albedo=albedo, class_id=class_id, noise=noise, u=u)
    dev = rng.device
    with torch.cuda.device(dev):
        xyz = torch.empty(F, rays, 3, device=dev, dtype=torch.float32)
        idx = torch.empty(F, rays, device=dev, dtype=torch.int32)
        count = torch.empty(F, device=dev, dtype=torch.int32)
        intensity = torch.empty(F, rays, device=dev, dtype=torch.float32)
        label = torch.empty(F, rays, device=dev, dtype=torch.int32)
        _lib.check(_lib.load().dpm_lidar_emit(_ptr(rng), _ptr(prim), _ptr(cos_inc), _ptr(dirs), rays, F, _ptr(noise), _ptr(u),
                                              float(drop_prob), _ptr(albedo), _ptr(class_id), albedo.shape[0] - 1, _ptr(xyz),
                                              _ptr(idx), _ptr(count), _ptr(intensity), _ptr(label), _stream(rng)),
                   "dpm_lidar_emit")
    return xyz, idx, count, intensity, label


# ------------------------------------------------------------------------------------------------------------
# deskew (csrc/deskew.hip)
# ------------------------------------------------------------------------------------------------------------
DESKEW_COLUMN, DESKEW_AZIMUTH, DESKEW_TIMES = 0, 1, 2


def points_deskew(xyz: torch.Tensor, idx: torch.Tensor, count: torch.Tensor, motion, time_mode: int, azimuth_steps: int = 0,
                  times: Optional[torch.Tensor] = None, s_ref: float = 0.0):
    """dpm_points_deskew, in place: xyz (cap,3) fp32, idx (cap,) int32, count (1,) int32 on the GPU; motion (4,4) float64 on
    the HOST = D, the sensor's pose at the end of the sweep in its frame at the start; time_mode DESKEW_COLUMN (idx %
    azimuth_steps), DESKEW_AZIMUTH (the point's own azimuth, rounded to a column when azimuth_steps > 0) or DESKEW_TIMES
    (times[idx], fp32 on the GPU); every row p measured at fraction s becomes D(s_ref)^-1 D(s) p."""
    import numpy as np
    _lidar_arg(xyz, torch.float32, "xyz", xyz.dim() == 2 and xyz.shape[1] == 3 and xyz.shape[0] >= 1, "(cap,3), cap >= 1")
    _lidar_arg(idx, torch.int32, "idx", idx.shape == xyz.shape[:1], "(cap,)")
    _lidar_arg(count, torch.int32, "count", count.numel() == 1, "(1,)")
    if times is not None:
        _lidar_arg(times, torch.float32, "times", times.dim() == 1 and times.shape[0] >= 1, "(n,), n >= 1")
    _lidar_dev(xyz=xyz, idx=idx, count=count, times=times)
    D = np.ascontiguousarray(np.asarray(motion, dtype=np.float64))
    if D.shape != (4, 4) or not np.isfinite(D).all():
        raise ValueError("motion: a finite (4,4) matrix")
    m = (ctypes.c_double * 16)(*D.reshape(-1).tolist())
    with torch.cuda.device(xyz.device):
        _lib.check(_lib.load().dpm_points_deskew(_ptr(xyz), _ptr(idx), _ptr(count), xyz.shape[0], int(time_mode), _ptr(times),
                                                 0 if times is None else times.shape[0], int(azimuth_steps),
                                                 ctypes.cast(m, ctypes.c_void_p), float(s_ref), _stream(xyz)),
                   "dpm_points_deskew")
    return xyz


# ------------------------------------------------------------------------------------------------------------
# map evaluation (csrc/map_eval.hip)
# ------------------------------------------------------------------------------------------------------------
MAP_EVAL_REC = 12            # floats of a scene record
STATS_COLS = 5               # columns of the statistics table before the thresholds
STATS_MAX_THRESHOLDS = 8
STATS_MAX_CLASSES = 256


def _origin3(origin):
    o = [float(v) for v in origin]
    if len(o) != 3:
        raise ValueError("origin: three numbers")
    return o


def scene_distance(points: torch.Tensor, records: torch.Tensor, ground: Optional[float], origin):
    """dpm_scene_distance: points (3,M) fp32, records (P,12) fp32 (evaluate.scene_records), ground = z0 - origin_z or None,
    origin three floats -> dist (M,) fp32, surf (M,) int32 (0..P-1, P = ground, -1 = none).  One launch, no synchronisation."""
    _lidar_arg(points, torch.float32, "points", points.dim() == 2 and points.shape[0] == 3, "(3,M)")
    _lidar_arg(records, torch.float32, "records", records.dim() == 2 and records.shape[1] == MAP_EVAL_REC, f"(P,{MAP_EVAL_REC})")
    o = _origin3(origin)
    _lidar_dev(points=points, records=records)
    M, P, dev = points.shape[1], records.shape[0], points.device
    with torch.cuda.device(dev):
        dist = torch.empty(M, device=dev, dtype=torch.float32)
        surf = torch.empty(M, device=dev, dtype=torch.int32)
        _lib.check(_lib.load().dpm_scene_distance(_ptr(points), M, _ptr(records) if P else None, P,
                                                  0.0 if ground is None else float(ground), int(ground is not None), *o,
                                                  _ptr(dist), _ptr(surf), _stream(points)), "dpm_scene_distance")
    return dist, surf


def cloud_nn(query: torch.Tensor, target: torch.Tensor, max_dist: float, origin):
    """dpm_cloud_nn: query (3,Nq), target (3,Nt) fp32 -> dist (Nq,) fp32 (+inf without a neighbour within max_dist),
    idx (Nq,) int32 (-1).  Five launches, no synchronisation."""
    if not 0.0 < float(max_dist) < 1e18:
        raise ValueError("0 < max_dist < 1e18")
    _lidar_arg(query, torch.float32, "query", query.dim() == 2 and query.shape[0] == 3, "(3,Nq)")
    _lidar_arg(target, torch.float32, "target", target.dim() == 2 and target.shape[0] == 3, "(3,Nt)")
    o = _origin3(origin)
    _lidar_dev(query=query, target=target)
    Nq, Nt, dev = query.shape[1], target.shape[1], query.device
    lib = _lib.load()
    with torch.cuda.device(dev):
        dist = torch.empty(Nq, device=dev, dtype=torch.float32)
        idx = torch.empty(Nq, device=dev, dtype=torch.int32)
        ws = torch.empty(lib.dpm_cloud_nn_workspace_bytes(Nq, Nt), device=dev, dtype=torch.uint8)
        _lib.check(lib.dpm_cloud_nn(_ptr(query) if Nq else None, Nq, _ptr(target) if Nt else None, Nt, float(max_dist), *o,
                                    _ptr(dist), _ptr(idx), _ptr(ws), _stream(query)), "dpm_cloud_nn")
    return dist, idx


def distance_stats(dist: torch.Tensor, thresholds, max_dist: float, surf: Optional[torch.Tensor] = None,
                   class_id: Optional[torch.Tensor] = None, n_classes: int = 0) -> torch.Tensor:
    """dpm_distance_stats: dist (M,) fp32, thresholds a sequence of at most 8 numbers (rounded to fp32), optional surf (M,)
    int32 with class_id (P+1,) int32 and n_classes -> (n_classes + 1, 5 + T) float64 on the device: per class, then in total,
    matched count, unmatched count, sum d, sum d^2, max d, count with d <= thresholds[t].  Two launches, no synchronisation."""
    thr = (ctypes.c_float * max(len(thresholds), 1))(*[float(t) for t in thresholds])
    T, C = len(thresholds), int(n_classes)
    if T > STATS_MAX_THRESHOLDS:
        raise ValueError(f"at most {STATS_MAX_THRESHOLDS} thresholds")
    if not 0 <= C <= STATS_MAX_CLASSES or not float(max_dist) > 0:
        raise ValueError(f"0 <= n_classes <= {STATS_MAX_CLASSES} and max_dist > 0")
    _lidar_arg(dist, torch.float32, "dist", dist.dim() == 1, "(M,)")
    if C:
        if surf is None or class_id is None:
            raise ValueError("n_classes > 0 needs surf and class_id")
        _lidar_arg(surf, torch.int32, "surf", surf.shape == dist.shape, "(M,)")
        _lidar_arg(class_id, torch.int32, "class_id", class_id.dim() == 1 and class_id.shape[0] >= 1, "(P+1,)")
    else:
        surf = class_id = None
    _lidar_dev(dist=dist, surf=surf, class_id=class_id)
    M, dev = dist.shape[0], dist.device
    lib = _lib.load()
    with torch.cuda.device(dev):
        out = torch.empty(C + 1, STATS_COLS + T, device=dev, dtype=torch.float64)
        ws = torch.empty(lib.dpm_distance_stats_workspace_bytes(M, C, T), device=dev, dtype=torch.uint8)
        _lib.check(lib.dpm_distance_stats(_ptr(dist) if M else None, M, _ptr(surf), _ptr(class_id),
                                          0 if class_id is None else class_id.shape[0], C, ctypes.addressof(thr) if T else None,
                                          T, float(max_dist), _ptr(out), _ptr(ws), _stream(dist)), "dpm_distance_stats")
    return out


# -- the rolling local map and the registration against it (csrc/local_map.hip; orchestration in odometry.py) ----------------
LOCAL_MAP_HDR_WORDS = 64    # the map buffer's header as int32 words: [0] points that found no slot, [1] points outside the keys


def _local_map_args(table: torch.Tensor, cap_vox: int, subdiv: int, origin=None):
    _chk(table, torch.uint8, "table")
    if table.numel() != _lib.load().dpm_local_map_bytes(int(cap_vox), int(subdiv)) or table.numel() == 0:
        raise ValueError("table: dpm_local_map_bytes(cap_vox, subdiv) bytes, cap_vox a power of two in [2, 2^24], subdiv in 1..3")
    return None if origin is None else (ctypes.c_double * 3)(*_origin3(origin))


# what the local map and the TSDF map (below) take alike: a frame, a list of stored frames, one registration problem
def _frame_args(what, xyz, count, pose, idx=None):
    _chk(xyz, torch.float32, "xyz"), idx is None or _chk(idx, torch.int32, "idx"), _chk(count, torch.int32, "count")
    _chk(pose, torch.float64, "pose")
    if xyz.dim() != 2 or xyz.shape[1] != 3 or (idx is not None and idx.shape != xyz.shape[:1]) or count.numel() != 1 \
            or pose.numel() != 16:
        raise ValueError(f"{what}: xyz (cap,3), {'' if idx is None else 'idx (cap,), '}count (1,), pose (4,4)")


def _frame_list_args(what, store, lengths, frames, poses) -> int:
    _chk(store, torch.float32, "store"), _chk(lengths, torch.int32, "lengths"), _chk(frames, torch.int32, "frames")
    _chk(poses, torch.float64, "poses")
    F = frames.numel()
    if store.dim() != 3 or store.shape[1] != 3 or store.shape[0] < 1 or store.shape[2] < 1 or lengths.shape != store.shape[:1] \
            or frames.dim() != 1 or poses.numel() != 16 * F or F > 65535:
        raise ValueError(f"{what}: store (capacity,3,P), lengths (capacity,), frames (F,) with F <= 65535, poses (F,4,4)")
    return F


# The two sources of rows (csrc/scan_source.h) as the C entry points take them: the first pointer, then the rest; an operation's
# per-row side arrays (normals, idx) sit between the two, and a list's F follows its per-entry arrays, in the operation's tail.
def _one_frame(what, xyz, count, pose, idx=None):
    _frame_args(what, xyz, count, pose, idx)
    return _ptr(xyz), (_ptr(count), xyz.shape[0], _ptr(pose))


def _stored_frames(what, store, lengths, frames, poses):
    F = _frame_list_args(what, store, lengths, frames, poses)
    return (_ptr(store), (_ptr(lengths), store.shape[0], store.shape[2], _ptr(frames), _ptr(poses))), F


def _source_call(entry, table, head, o, source, side, tail):
    """lib.<entry>(table, *head, origin, the source with its side arrays in their place, *tail, stream)"""
    first, rest = source
    with torch.cuda.device(table.device):
        _lib.check(getattr(_lib.load(), entry)(_ptr(table), *head, ctypes.addressof(o), first, *side, *rest, *tail, _stream(table)),
                   entry)


def _register_one(what, entry, head, table, xyz, count, init, schedule, kernel_scale, tol_rot, tol_trans, debug, row_dtypes,
                  ws_bytes):
    """one scan against a map: entry(*head, the frame, init, the schedule, the results, the debug rows, system, workspace,
    stream); `what` names it in an error.  row_dtypes: the per-row debug outputs, (cap,) each, -1 where nothing is written
    -> (pose (4,4), fitness, rmse, iterations, status[, *rows, system (29,) fp64 with debug])"""
    dist, iters, n_stages = _schedule_arrays(schedule)
    dev, cap = table.device, xyz.shape[0]
    with torch.cuda.device(dev):
        pose, fitness, rmse, iterations, status = _registration_results(1, dev)
        pose = pose[0]
        rows = [torch.full((cap,), -1, device=dev, dtype=t) if debug else None for t in row_dtypes]
        system = torch.zeros(ICP_NSUM, device=dev, dtype=torch.float64) if debug else None
        ws = torch.empty(ws_bytes, device=dev, dtype=torch.uint8)
        _lib.check(entry(*head, _ptr(xyz), _ptr(count), cap, _ptr(init), ctypes.addressof(dist), ctypes.addressof(iters), n_stages,
                         float(kernel_scale), float(tol_rot), float(tol_trans), _ptr(pose), _ptr(fitness), _ptr(rmse),
                         _ptr(iterations), _ptr(status), *[_ptr(r) for r in rows], _ptr(system), _ptr(ws), _stream(table)), what)
    out = (pose, fitness, rmse, iterations, status)
    return (*out, *rows, system) if debug else out


def local_map_new(cap_vox: int, subdiv: int, device) -> torch.Tensor:
    """an empty map: the uint8 buffer every other local_map_* call takes"""
    n = _lib.load().dpm_local_map_bytes(int(cap_vox), int(subdiv))
    if n == 0:
        raise ValueError("cap_vox: a power of two in [2, 2^24]; subdiv: 1, 2 or 3")
    with torch.cuda.device(device):
        table = torch.empty(n, device=device, dtype=torch.uint8)
    return local_map_clear(table, cap_vox, subdiv)


def local_map_clear(table, cap_vox, subdiv) -> torch.Tensor:
    """dpm_local_map_init: the header zeroed, both halves empty"""
    _local_map_args(table, cap_vox, subdiv)
    with torch.cuda.device(table.device):
        _lib.check(_lib.load().dpm_local_map_init(_ptr(table), int(cap_vox), int(subdiv), _stream(table)), "dpm_local_map_init")
    return table


def local_map_insert(table, cap_vox, subdiv, half, voxel, origin, xyz, idx, count, pose, stamp, min_range, max_range):
    """dpm_local_map_insert: xyz (cap,3) fp32, idx (cap,) int32, count (1,) int32, pose (4,4) fp64, all on the GPU"""
    o = _local_map_args(table, cap_vox, subdiv, origin)
    _source_call("dpm_local_map_insert", table, (int(cap_vox), int(subdiv), int(half), float(voxel)), o,
                 _one_frame("local_map_insert", xyz, count, pose, idx), (_ptr(idx),), (int(stamp), float(min_range), float(max_range)))


def local_map_prune(table, cap_vox, subdiv, half, voxel, origin, pose, radius):
    """dpm_local_map_prune: half `half` -> the other half; the caller works on 1 - half afterwards"""
    o = _local_map_args(table, cap_vox, subdiv, origin)
    _chk(pose, torch.float64, "pose")
    if pose.numel() != 16:
        raise ValueError("local_map_prune: pose (4,4)")
    with torch.cuda.device(table.device):
        _lib.check(_lib.load().dpm_local_map_prune(_ptr(table), int(cap_vox), int(subdiv), int(half), float(voxel), ctypes.addressof(o),
                                                   _ptr(pose), float(radius), _stream(table)), "dpm_local_map_prune")


def local_map_insert_frames(table, cap_vox, subdiv, half, voxel, origin, store, lengths, frames, poses, stamps, centre, radius,
                            min_range, max_range):
    """dpm_local_map_insert_frames: store (capacity,3,P) fp32 channel-major, lengths (capacity,) int32, frames (F,) int32 rows
    of the store, poses (F,4,4) fp64, stamps (F,) int32 holding the uint32 stamps' bits, centre (4,4) fp64 or None (then
    radius is ignored), all on the GPU.  Two launches for any F, no host synchronisation, capturable in a graph."""
    o = _local_map_args(table, cap_vox, subdiv, origin)
    source, F = _stored_frames("local_map_insert_frames", store, lengths, frames, poses)
    if _chk(stamps, torch.int32, "stamps").shape != frames.shape:
        raise ValueError("local_map_insert_frames: stamps (F,), one per frame")
    if centre is not None:
        _chk(centre, torch.float64, "centre")
        if centre.numel() != 16:
            raise ValueError("local_map_insert_frames: centre (4,4)")
    _source_call("dpm_local_map_insert_frames", table, (int(cap_vox), int(subdiv), int(half), float(voxel)), o, source, (),
                 (_ptr(stamps), F, _ptr(centre), 0.0 if centre is None else float(radius), float(min_range), float(max_range)))


def local_map_planes(table, cap_vox, subdiv, half, voxel, origin, plane_radius, planes=None, counts=None):
    """dpm_local_map_planes -> (planes (cap_vox,4) fp32 (normal, w), counts (cap_vox,) int32) per SLOT of half `half`, written
    into the given buffers or new ones.  One launch, no host synchronisation, capturable in a graph."""
    o = _local_map_args(table, cap_vox, subdiv, origin)
    dev = table.device
    with torch.cuda.device(dev):
        planes = torch.empty(int(cap_vox), 4, device=dev, dtype=torch.float32) if planes is None else planes
        counts = torch.empty(int(cap_vox), device=dev, dtype=torch.int32) if counts is None else counts
        _chk(planes, torch.float32, "planes"), _chk(counts, torch.int32, "counts")
        if tuple(planes.shape) != (int(cap_vox), 4) or tuple(counts.shape) != (int(cap_vox),):
            raise ValueError("local_map_planes: planes (cap_vox,4), counts (cap_vox,)")
        _lib.check(_lib.load().dpm_local_map_planes(_ptr(table), int(cap_vox), int(subdiv), int(half), float(voxel),
                                                    ctypes.addressof(o), float(plane_radius), _ptr(planes), _ptr(counts),
                                                    _stream(table)), "dpm_local_map_planes")
    return planes, counts


def local_map_register_planes(table, cap_vox, subdiv, half, voxel, origin, planes, counts, min_points, max_ratio, xyz, count,
                              init, schedule, kernel_scale=0.0, tol_rot=1e-7, tol_trans=1e-6, debug=False):
    """dpm_local_map_register_planes: local_map_register with point-to-plane rows on the planes / counts local_map_planes
    wrote for this map and half; key and sub of debug are -1 where the match gave no row"""
    _chk(planes, torch.float32, "planes"), _chk(counts, torch.int32, "counts")
    if tuple(planes.shape) != (int(cap_vox), 4) or tuple(counts.shape) != (int(cap_vox),):
        raise ValueError("local_map_register_planes: planes (cap_vox,4), counts (cap_vox,)")
    return local_map_register(table, cap_vox, subdiv, half, voxel, origin, xyz, count, init, schedule, kernel_scale, tol_rot,
                              tol_trans, debug, _plane=(planes, counts, int(min_points), float(max_ratio)))


def local_map_register(table, cap_vox, subdiv, half, voxel, origin, xyz, count, init, schedule, kernel_scale=0.0,
                       tol_rot=1e-7, tol_trans=1e-6, debug=False, _plane=None):
    """dpm_local_map_register: xyz (cap,3) fp32, count (1,) int32, init (4,4) fp64 on the GPU; schedule = [(max_dist, max_iter),
    ...] with every max_dist <= voxel -> pose (4,4) fp64, fitness, rmse (1,) fp32, iterations, status (1,) int32[, key (cap,)
    int64, sub (cap,) int32, system (29,) fp64 with debug].  No host synchronisation, capturable in a graph."""
    o = _local_map_args(table, cap_vox, subdiv, origin)
    _chk(xyz, torch.float32, "xyz"), _chk(count, torch.int32, "count"), _chk(init, torch.float64, "init")
    if xyz.dim() != 2 or xyz.shape[1] != 3 or xyz.shape[0] < 1 or count.numel() != 1 or tuple(init.shape) != (4, 4):
        raise ValueError("local_map_register: xyz (cap,3) with cap >= 1, count (1,), init (4,4)")
    lib, head = _lib.load(), (_ptr(table), int(cap_vox), int(subdiv), int(half), float(voxel), ctypes.addressof(o))
    what, entry = "dpm_local_map_register", lib.dpm_local_map_register
    if _plane is not None:
        planes, counts, min_points, max_ratio = _plane
        what, entry = "dpm_local_map_register_planes", lib.dpm_local_map_register_planes
        head = (*head, _ptr(planes), _ptr(counts), min_points, max_ratio)
    return _register_one(what, entry, head, table, xyz, count, init, schedule, kernel_scale, tol_rot, tol_trans, debug,
                         (torch.int64, torch.int32), 512 + 256 * ((xyz.shape[0] + 255) // 256))


def local_map_export(table, cap_vox, subdiv, half, max_out=None):
    """dpm_local_map_export -> (keys (n,) int64 holding the uint64 keys' bits, sub (n,) int32, owner (n,) int64, xyz (n,3) fp32),
    in no defined order; max_out None: counted first (a host synchronisation), then exported whole (a second one).
    max_out = 0 -> the count alone, as an int."""
    _local_map_args(table, cap_vox, subdiv)
    dev = table.device
    lib = _lib.load()

    def call(n):
        with torch.cuda.device(dev):
            count = torch.zeros(1, device=dev, dtype=torch.int32)
            keys = torch.empty(n, device=dev, dtype=torch.int64)
            sub = torch.empty(n, device=dev, dtype=torch.int32)
            owner = torch.empty(n, device=dev, dtype=torch.int64)
            xyz = torch.empty(n, 3, device=dev, dtype=torch.float32)
            _lib.check(lib.dpm_local_map_export(_ptr(table), int(cap_vox), int(subdiv), int(half), _ptr(keys) if n else None,
                                                _ptr(sub) if n else None, _ptr(owner) if n else None, _ptr(xyz) if n else None,
                                                _ptr(count), n, _stream(table)), "dpm_local_map_export")
        return count, keys, sub, owner, xyz

    if max_out is None or int(max_out) == 0:
        n = int(call(0)[0].item())
        if max_out is not None:
            return n
        max_out = n
    count, keys, sub, owner, xyz = call(int(max_out))
    n = min(int(count.item()), int(max_out))
    return keys[:n], sub[:n], owner[:n], xyz[:n]


# -- the TSDF surface map (csrc/tsdf_map.hip; orchestration in tsdf.py) --------------------------------------------------------
TSDF_MAX_TRUNCATION = 64.0  # metres: tau 2^24 2^32 < 2^63
TSDF_MAX_STEPS = 4096       # ceil(truncation / step) at most
TSDF_MAX_CARVE_WEIGHT = 65535   # count units a carve may add per crossed voxel
TSDF_MAX_CARVE_STEPS = 65536    # max_range / step at most for a carve


def tsdf_rays(truncation: float, step: float, min_range: float, max_range: float):
    """the ray parameters every integrate call takes, checked as the entry points check them -> four floats"""
    tau, h, lo, hi = float(truncation), float(step), float(min_range), float(max_range)
    if not (0.0 < tau <= TSDF_MAX_TRUNCATION and h > 0.0 and tau / h <= TSDF_MAX_STEPS):
        raise ValueError(f"0 < truncation <= {TSDF_MAX_TRUNCATION}, step > 0 and ceil(truncation / step) <= {TSDF_MAX_STEPS}")
    if not 0.0 <= lo <= hi < 1e18:
        raise ValueError("0 <= min_range <= max_range")
    return lo, hi, tau, h


def _tsdf_args(table: torch.Tensor, cap_vox: int, origin=None):
    _chk(table, torch.uint8, "table")
    if table.numel() != _lib.load().dpm_tsdf_bytes(int(cap_vox)) or table.numel() == 0:
        raise ValueError("table: dpm_tsdf_bytes(cap_vox) bytes, cap_vox a power of two in [2, 2^24]")
    return None if origin is None else (ctypes.c_double * 3)(*_origin3(origin))


def tsdf_new(cap_vox: int, device) -> torch.Tensor:
    """an empty map: the uint8 buffer every other tsdf_* call takes"""
    n = _lib.load().dpm_tsdf_bytes(int(cap_vox))
    if n == 0:
        raise ValueError("cap_vox: a power of two in [2, 2^24]")
    with torch.cuda.device(device):
        table = torch.empty(n, device=device, dtype=torch.uint8)
    return tsdf_clear(table, cap_vox)


def tsdf_clear(table, cap_vox) -> torch.Tensor:
    """dpm_tsdf_init: the header zeroed, the table empty"""
    _tsdf_args(table, cap_vox)
    with torch.cuda.device(table.device):
        _lib.check(_lib.load().dpm_tsdf_init(_ptr(table), int(cap_vox), _stream(table)), "dpm_tsdf_init")
    return table


def tsdf_integrate(table, cap_vox, voxel, origin, xyz, count, pose, min_range, max_range, truncation, step):
    """dpm_tsdf_integrate: xyz (cap,3) fp32, count (1,) int32, pose (4,4) fp64, all on the GPU.  One launch, no host
    synchronisation, capturable in a graph."""
    rays = tsdf_rays(truncation, step, min_range, max_range)
    o = _tsdf_args(table, cap_vox, origin)
    _source_call("dpm_tsdf_integrate", table, (int(cap_vox), float(voxel)), o, _one_frame("tsdf_integrate", xyz, count, pose), (), rays)


def tsdf_integrate_frames(table, cap_vox, voxel, origin, store, lengths, frames, poses, min_range, max_range, truncation, step):
    """dpm_tsdf_integrate_frames: store (capacity,3,P) fp32 channel-major, lengths (capacity,) int32, frames (F,) int32 rows of
    the store, poses (F,4,4) fp64, all on the GPU.  One launch for any F, no host synchronisation, capturable in a graph."""
    rays = tsdf_rays(truncation, step, min_range, max_range)
    o = _tsdf_args(table, cap_vox, origin)
    source, F = _stored_frames("tsdf_integrate_frames", store, lengths, frames, poses)
    _source_call("dpm_tsdf_integrate_frames", table, (int(cap_vox), float(voxel)), o, source, (), (F, *rays))


def _tsdf_cos(cos_min) -> float:
    if not 0.0 <= float(cos_min) <= 1.0:
        raise ValueError("0 <= cos_min <= 1")
    return float(cos_min)


def tsdf_carve_args(weight, margin, step: float, max_range: float):
    """the carve's own arguments, checked as the entry points check them -> (int weight, float margin)"""
    w, g = int(weight), float(margin)
    if not (1 <= w <= TSDF_MAX_CARVE_WEIGHT and 0.0 <= g < 1e18):
        raise ValueError(f"carve: weight in [1, {TSDF_MAX_CARVE_WEIGHT}] count units, margin >= 0")
    if not float(max_range) / float(step) <= TSDF_MAX_CARVE_STEPS:
        raise ValueError(f"carve: max_range / step <= {TSDF_MAX_CARVE_STEPS}")
    return w, g


def tsdf_integrate_planes(table, cap_vox, voxel, origin, xyz, normals, count, pose, min_range, max_range, truncation, step,
                          cos_min=0.0):
    """dpm_tsdf_integrate_planes: tsdf_integrate's arguments and normals (cap,3) fp32 in the sensor frame.  One launch, no host
    synchronisation, capturable in a graph."""
    rays = tsdf_rays(truncation, step, min_range, max_range)
    o = _tsdf_args(table, cap_vox, origin)
    source = _one_frame("tsdf_integrate_planes", xyz, count, pose)
    if _chk(normals, torch.float32, "normals").shape != xyz.shape:
        raise ValueError("tsdf_integrate_planes: normals (cap,3), one per row of xyz")
    _source_call("dpm_tsdf_integrate_planes", table, (int(cap_vox), float(voxel)), o, source, (_ptr(normals),),
                 (*rays, _tsdf_cos(cos_min)))


def tsdf_integrate_planes_frames(table, cap_vox, voxel, origin, store, normals, lengths, frames, poses, min_range, max_range,
                                 truncation, step, cos_min=0.0):
    """dpm_tsdf_integrate_planes_frames: tsdf_integrate_frames' arguments and a normals store (capacity,P,3) fp32"""
    rays = tsdf_rays(truncation, step, min_range, max_range)
    o = _tsdf_args(table, cap_vox, origin)
    source, F = _stored_frames("tsdf_integrate_planes_frames", store, lengths, frames, poses)
    if tuple(_chk(normals, torch.float32, "normals").shape) != (store.shape[0], store.shape[2], 3):
        raise ValueError("tsdf_integrate_planes_frames: normals (capacity,P,3)")
    _source_call("dpm_tsdf_integrate_planes_frames", table, (int(cap_vox), float(voxel)), o, source, (_ptr(normals),),
                 (F, *rays, _tsdf_cos(cos_min)))


def tsdf_carve(table, cap_vox, voxel, origin, xyz, count, pose, min_range, max_range, truncation, step, weight, margin):
    """dpm_tsdf_carve: tsdf_integrate's arguments, weight (count units) and margin (metres).  Lookups only; one launch, no
    host synchronisation, capturable in a graph."""
    rays = tsdf_rays(truncation, step, min_range, max_range)
    carve = tsdf_carve_args(weight, margin, step, max_range)
    o = _tsdf_args(table, cap_vox, origin)
    _source_call("dpm_tsdf_carve", table, (int(cap_vox), float(voxel)), o, _one_frame("tsdf_carve", xyz, count, pose), (),
                 (*rays, *carve))


def tsdf_carve_frames(table, cap_vox, voxel, origin, store, lengths, frames, poses, min_range, max_range, truncation, step, weight,
                      margin):
    """dpm_tsdf_carve_frames: tsdf_integrate_frames' arguments, weight and margin"""
    rays = tsdf_rays(truncation, step, min_range, max_range)
    carve = tsdf_carve_args(weight, margin, step, max_range)
    o = _tsdf_args(table, cap_vox, origin)
    source, F = _stored_frames("tsdf_carve_frames", store, lengths, frames, poses)
    _source_call("dpm_tsdf_carve_frames", table, (int(cap_vox), float(voxel)), o, source, (), (F, *rays, *carve))


def _counted(call, max_out):
    """the `count may exceed max_out` contract of the export-style entry points: call(n) -> (count (1,) int32, *outputs of n
    rows).  max_out None: counted first, then written whole (the map has not changed in between, so the count is not read
    again); max_out = 0 -> the count alone, as an int; otherwise -> (count as an int, *outputs cut to min(count, max_out)
    rows).  One read of the count, a host synchronisation, in every case."""
    if max_out is None or int(max_out) == 0:
        n = int(call(0)[0].item())
        return n if max_out is not None else (n, *call(n)[1:])
    count, *out = call(int(max_out))
    total = int(count.item())
    return (total, *[t[:min(total, int(max_out))] for t in out])


def tsdf_export(table, cap_vox, max_out=None):
    """dpm_tsdf_export -> (count, keys (n,) int64 holding the uint64 keys' bits, sums (n,) int64, counts (n,) int32 holding
    the uint32 counts' bits) in no defined order; max_out as in _counted"""
    _tsdf_args(table, cap_vox)
    dev, lib = table.device, _lib.load()

    def call(n):
        with torch.cuda.device(dev):
            count = torch.zeros(1, device=dev, dtype=torch.int32)
            keys = torch.empty(n, device=dev, dtype=torch.int64)
            sums = torch.empty(n, device=dev, dtype=torch.int64)
            counts = torch.empty(n, device=dev, dtype=torch.int32)
            _lib.check(lib.dpm_tsdf_export(_ptr(table), int(cap_vox), _ptr(keys) if n else None, _ptr(sums) if n else None,
                                           _ptr(counts) if n else None, _ptr(count), n, _stream(table)), "dpm_tsdf_export")
        return count, keys, sums, counts
    return _counted(call, max_out)


TSDF_TILE_BITS = (3, 10)    # a tile has 2^b voxels per axis, b in this range


def tsdf_evict(src, dst, cap_vox, voxel, origin, pose, radius, tile_bits, keys, sums, counts, count):
    """dpm_tsdf_evict: src -> dst (a second table of the same cap_vox, not src), pose (4,4) fp64 on the GPU.  keys, sums (n,)
    int64 and counts (n,) int32 on the GPU are the list (max_out = n; n = 0: nothing leaves), count (1,) int32 receives the
    number of voxels that wanted out -- it is zeroed by the call and NOT read here.  Two launches, no host synchronisation,
    capturable in a graph."""
    o = _tsdf_args(src, cap_vox, origin)
    _tsdf_args(dst, cap_vox)
    if o is None or dst.device != src.device or dst.data_ptr() == src.data_ptr():
        raise ValueError("tsdf_evict: an origin, and dst a second table on src's device")
    _chk(pose, torch.float64, "pose")
    if pose.numel() != 16:
        raise ValueError("tsdf_evict: pose (4,4)")
    if not (0.0 <= float(radius) < 1e18 and TSDF_TILE_BITS[0] <= int(tile_bits) <= TSDF_TILE_BITS[1]):
        raise ValueError(f"tsdf_evict: radius >= 0, tile_bits in [{TSDF_TILE_BITS[0]}, {TSDF_TILE_BITS[1]}]")
    n = _chk(keys, torch.int64, "keys").numel()
    if _chk(sums, torch.int64, "sums").numel() != n or _chk(counts, torch.int32, "counts").numel() != n:
        raise ValueError("tsdf_evict: keys, sums, counts of one length")
    if _chk(count, torch.int32, "count").numel() != 1:
        raise ValueError("tsdf_evict: count (1,)")
    with torch.cuda.device(src.device):
        _lib.check(_lib.load().dpm_tsdf_evict(_ptr(src), _ptr(dst), int(cap_vox), float(voxel), ctypes.addressof(o), _ptr(pose),
                                              float(radius), int(tile_bits), _ptr(keys) if n else None, _ptr(sums) if n else None,
                                              _ptr(counts) if n else None, _ptr(count), n, _stream(src)), "dpm_tsdf_evict")


def tsdf_absorb(table, cap_vox, keys, sums, counts):
    """dpm_tsdf_absorb: keys, sums (n,) int64 and counts (n,) int32 (the uint32 counts' bits) on the GPU are added to the
    table.  One launch, no host synchronisation, capturable in a graph; n = 0 launches nothing."""
    _tsdf_args(table, cap_vox)
    n = _chk(keys, torch.int64, "keys").numel()
    if _chk(sums, torch.int64, "sums").numel() != n or _chk(counts, torch.int32, "counts").numel() != n:
        raise ValueError("tsdf_absorb: keys, sums, counts of one length")
    if n == 0:
        return
    with torch.cuda.device(table.device):
        _lib.check(_lib.load().dpm_tsdf_absorb(_ptr(table), int(cap_vox), _ptr(keys), _ptr(sums), _ptr(counts), n, _stream(table)),
                   "dpm_tsdf_absorb")


def _tsdf_surface(entry, table, cap_vox, voxel, min_count, owners, max_out):
    """both surface entry points: the four outputs allocated, `entry` called with `owners` (its arguments between min_count and
    the outputs) -> (count, keys, axes, xyz, normals); max_out as in _counted"""
    _tsdf_args(table, cap_vox)
    if int(min_count) < 1:
        raise ValueError("min_count >= 1")
    dev, fn = table.device, getattr(_lib.load(), entry)

    def call(n):
        with torch.cuda.device(dev):
            count = torch.zeros(1, device=dev, dtype=torch.int32)
            keys = torch.empty(n, device=dev, dtype=torch.int64)
            axes = torch.empty(n, device=dev, dtype=torch.int32)
            xyz = torch.empty(n, 3, device=dev, dtype=torch.float32)
            normals = torch.empty(n, 3, device=dev, dtype=torch.float32)
            _lib.check(fn(_ptr(table), int(cap_vox), float(voxel), int(min_count), *owners, _ptr(keys) if n else None,
                          _ptr(axes) if n else None, _ptr(xyz) if n else None, _ptr(normals) if n else None, _ptr(count), n,
                          _stream(table)), entry)
        return count, keys, axes, xyz, normals
    return _counted(call, max_out)


def tsdf_surface(table, cap_vox, voxel, min_count=1, max_out=None):
    """dpm_tsdf_surface -> (count, keys (n,) int64, axes (n,) int32, xyz (n,3) fp32 map-frame, normals (n,3) fp32) in no
    defined order; max_out as in _counted"""
    return _tsdf_surface("dpm_tsdf_surface", table, cap_vox, voxel, min_count, (), max_out)


def tsdf_mesh(table, cap_vox, voxel, min_count=1, max_out=None):
    """dpm_tsdf_mesh -> (count, vertex_keys (n,3) int64, vertex_dirs (n,3) int32, xyz (n,3,3) fp32 map-frame): one triangle a
    row, in no defined order; max_out as in _counted"""
    _tsdf_args(table, cap_vox)
    if int(min_count) < 1:
        raise ValueError("min_count >= 1")
    dev, lib = table.device, _lib.load()

    def call(n):
        with torch.cuda.device(dev):
            count = torch.zeros(1, device=dev, dtype=torch.int32)
            vkeys = torch.empty(n, 3, device=dev, dtype=torch.int64)
            vdirs = torch.empty(n, 3, device=dev, dtype=torch.int32)
            xyz = torch.empty(n, 3, 3, device=dev, dtype=torch.float32)
            _lib.check(lib.dpm_tsdf_mesh(_ptr(table), int(cap_vox), float(voxel), int(min_count), _ptr(vkeys) if n else None,
                                         _ptr(vdirs) if n else None, _ptr(xyz) if n else None, _ptr(count), n, _stream(table)),
                       "dpm_tsdf_mesh")
        return count, vkeys, vdirs, xyz
    return _counted(call, max_out)


def _tsdf_owners(what, tiles, tile_bits, dev):
    """the owner list of a tile-owned extraction -> (pointer or None, n, tile_bits): tiles (n,) int64 on the device, SORTED and
    unique (the caller's word: nothing is read here); None or empty: everything is owned"""
    if tiles is None or tiles.numel() == 0:
        return None, 0, int(tile_bits)
    if _chk(tiles, torch.int64, "tiles").dim() != 1 or tiles.device != dev:
        raise ValueError(f"{what}: tiles (n,) int64 on the table's device")
    if not TSDF_TILE_BITS[0] <= int(tile_bits) <= TSDF_TILE_BITS[1]:
        raise ValueError(f"{what}: tile_bits in [{TSDF_TILE_BITS[0]}, {TSDF_TILE_BITS[1]}]")
    return _ptr(tiles), tiles.numel(), int(tile_bits)


def tsdf_surface_tiles(table, cap_vox, voxel, min_count=1, tiles=None, tile_bits=5, max_out=None):
    """dpm_tsdf_surface_tiles -> tsdf_surface's outputs for the records whose voxel k0 lies in one of `tiles` ((n,) int64 tile
    keys on the device, sorted ascending and unique; None or empty: every record); max_out as in _counted"""
    _tsdf_args(table, cap_vox)
    own, n_own, b = _tsdf_owners("tsdf_surface_tiles", tiles, tile_bits, table.device)
    return _tsdf_surface("dpm_tsdf_surface_tiles", table, cap_vox, voxel, min_count, (b, own, n_own), max_out)


def tsdf_mesh_indexed(table, cap_vox, voxel, min_count=1, tiles=None, tile_bits=5, max_out=None):
    """dpm_tsdf_mesh_indexed -> ((V, F), vertex_keys (v,) int64, vertex_dirs (v,) int32, xyz (v,3) fp32 map-frame, normals (v,3)
    fp32, faces (f,3) int32) in the table's slot order; tiles as in tsdf_surface_tiles.  max_out in _counted's manner with a
    pair: None: counted first, then written whole; (0, 0): the counts alone, as (V, F); (max_v, max_f): outputs cut to min(V,
    max_v) and min(F, max_f) rows, V and F as counted, nothing written beyond either maximum (a face may then name a vertex at
    or past max_v).  One read of the two counts, a host synchronisation, in every case."""
    _tsdf_args(table, cap_vox)
    if int(min_count) < 1:
        raise ValueError("min_count >= 1")
    dev, lib = table.device, _lib.load()
    own, n_own, b = _tsdf_owners("tsdf_mesh_indexed", tiles, tile_bits, dev)

    def call(nv, nf):
        with torch.cuda.device(dev):
            counts = torch.empty(2, device=dev, dtype=torch.int32)
            work = torch.empty(lib.dpm_tsdf_mesh_indexed_bytes(int(cap_vox)), device=dev, dtype=torch.uint8)
            vkeys = torch.empty(nv, device=dev, dtype=torch.int64)
            vdirs = torch.empty(nv, device=dev, dtype=torch.int32)
            xyz = torch.empty(nv, 3, device=dev, dtype=torch.float32)
            normals = torch.empty(nv, 3, device=dev, dtype=torch.float32)
            faces = torch.empty(nf, 3, device=dev, dtype=torch.int32)
            _lib.check(lib.dpm_tsdf_mesh_indexed(_ptr(table), int(cap_vox), float(voxel), int(min_count), b, own, n_own,
                                                 _ptr(vkeys) if nv else None, _ptr(vdirs) if nv else None, _ptr(xyz) if nv else None,
                                                 _ptr(normals) if nv else None, _ptr(faces) if nf else None, _ptr(counts), nv, nf,
                                                 _ptr(work), _stream(table)), "dpm_tsdf_mesh_indexed")
        return counts, vkeys, vdirs, xyz, normals, faces
    if max_out is None or tuple(int(n) for n in max_out) == (0, 0):
        V, F = (int(n) for n in call(0, 0)[0].tolist())
        return (V, F) if max_out is not None else ((V, F), *call(V, F)[1:])
    nv, nf = (int(n) for n in max_out)
    counts, *out = call(nv, nf)
    V, F = (int(n) for n in counts.tolist())
    return ((V, F), *[t[:min(V, nv)] for t in out[:4]], out[4][:min(F, nf)])


def tsdf_sample(table, cap_vox, voxel, origin, xyz, count, pose, min_count=1):
    """dpm_tsdf_sample: xyz (cap,3) fp32, count (1,) int32, pose (4,4) fp64 on the GPU -> (d (cap,) fp32, grad (cap,3) fp32 in
    the map frame's axes, flag (cap,) int32: 1 a value, 0 none, -1 past the count).  Lookups only; one launch, no host
    synchronisation, capturable in a graph."""
    o = _tsdf_args(table, cap_vox, origin)
    _frame_args("tsdf_sample", xyz, count, pose)
    if int(min_count) < 1:
        raise ValueError("min_count >= 1")
    dev, cap = table.device, xyz.shape[0]
    with torch.cuda.device(dev):
        d = torch.empty(cap, device=dev, dtype=torch.float32)
        grad = torch.empty(cap, 3, device=dev, dtype=torch.float32)
        flag = torch.empty(cap, device=dev, dtype=torch.int32)
        _lib.check(_lib.load().dpm_tsdf_sample(_ptr(table), int(cap_vox), float(voxel), ctypes.addressof(o), _ptr(xyz), _ptr(count),
                                               cap, _ptr(pose), int(min_count), _ptr(d) if cap else None, _ptr(grad) if cap else None,
                                               _ptr(flag) if cap else None, _stream(table)), "dpm_tsdf_sample")
    return d, grad, flag


def tsdf_register(table, cap_vox, voxel, origin, truncation, xyz, count, init, schedule, kernel_scale=0.0, tol_rot=1e-7,
                  tol_trans=1e-6, min_count=1, grad_min=0.5, debug=False):
    """dpm_tsdf_register: xyz (cap,3) fp32 with cap >= 1, count (1,) int32, init (4,4) fp64 on the GPU; schedule = [(max_dist,
    max_iter), ...] with every max_dist in (0, truncation] -> pose (4,4) fp64, fitness, rmse (1,) fp32, iterations, status (1,)
    int32[, flag (cap,) int32, system (29,) fp64 with debug].  Lookups only; no host synchronisation, capturable in a graph."""
    o = _tsdf_args(table, cap_vox, origin)
    _frame_args("tsdf_register", xyz, count, init)
    if xyz.shape[0] < 1 or tuple(init.shape) != (4, 4):
        raise ValueError("tsdf_register: xyz (cap,3) with cap >= 1, init (4,4)")
    if int(min_count) < 1 or not 0.0 <= float(grad_min) < 1e18:
        raise ValueError("tsdf_register: min_count >= 1, grad_min >= 0")
    stages = [(float(d), int(n)) for d, n in schedule]
    if any(not 0.0 < d <= float(truncation) for d, _ in stages):
        raise ValueError("tsdf_register: every max_dist of the schedule must lie in (0, truncation] (beyond the clamp the field is flat)")
    lib = _lib.load()
    head = (_ptr(table), int(cap_vox), float(voxel), ctypes.addressof(o), float(truncation), int(min_count), float(grad_min))
    return _register_one("dpm_tsdf_register", lib.dpm_tsdf_register, head, table, xyz, count, init, stages, kernel_scale, tol_rot,
                         tol_trans, debug, (torch.int32,), lib.dpm_tsdf_register_scratch_bytes(xyz.shape[0]))


TSDF_MAX_CAST_SAMPLES = 65536   # floor((max_range - min_range) / step) + 1 at most for a ray-cast
TSDF_MISS, TSDF_HIT, TSDF_BACK = 0, 1, 2


def tsdf_cast_args(min_range, max_range, step):
    """the marcher's own arguments, checked as the entry point checks them -> three floats"""
    lo, hi, h = float(min_range), float(max_range), float(step)
    if not (h > 0.0 and 0.0 <= lo <= hi < 1e18):
        raise ValueError("raycast: step > 0 and 0 <= min_range <= max_range")
    if not (hi - lo) / h < TSDF_MAX_CAST_SAMPLES:      # floor(q) + 1 <= N  <=>  q < N
        raise ValueError(f"raycast: floor((max_range - min_range) / step) + 1 <= {TSDF_MAX_CAST_SAMPLES}")
    return lo, hi, h


def _tsdf_blocks_args(blocks, cap_blocks):
    _chk(blocks, torch.uint8, "blocks")
    if blocks.numel() != _lib.load().dpm_tsdf_blocks_bytes(int(cap_blocks)) or blocks.numel() == 0:
        raise ValueError("blocks: dpm_tsdf_blocks_bytes(cap_blocks) bytes, cap_blocks a power of two in [2, 2^24]")


def tsdf_blocks(table, cap_vox, min_count, cap_blocks, out=None) -> torch.Tensor:
    """dpm_tsdf_blocks: the occupied-block set of the table as it is now, for voxels qualified at min_count -> the uint8 buffer
    tsdf_raycast takes (out: a buffer to build into).  Word 0 counts the claims that found no room.  Two launches, no host
    synchronisation, capturable in a graph."""
    _tsdf_args(table, cap_vox)
    if int(min_count) < 1:
        raise ValueError("min_count >= 1")
    n = _lib.load().dpm_tsdf_blocks_bytes(int(cap_blocks))
    if n == 0:
        raise ValueError("cap_blocks: a power of two in [2, 2^24]")
    with torch.cuda.device(table.device):
        blocks = torch.empty(n, device=table.device, dtype=torch.uint8) if out is None else out
        _tsdf_blocks_args(blocks, cap_blocks)
        _lib.check(_lib.load().dpm_tsdf_blocks(_ptr(table), int(cap_vox), int(min_count), _ptr(blocks), int(cap_blocks),
                                               _stream(table)), "dpm_tsdf_blocks")
    return blocks


def tsdf_raycast(table, cap_vox, voxel, origin, blocks, cap_blocks, poses, dirs, min_range, max_range, step, min_count=1, out=None):
    """dpm_tsdf_raycast: poses (F,4,4) fp64 and dirs (R,3) fp32 (sensor frame, unit) on the GPU; blocks: None (the plain form)
    or tsdf_blocks' buffer of this table and min_count -> (range (F,R) fp32, normals (F,R,3) fp32 in the sensor frame, flag (F,R)
    int32: TSDF_MISS / TSDF_HIT / TSDF_BACK); out: those three to write into.  Lookups only; one launch, no host
    synchronisation, capturable in a graph."""
    lo, hi, h = tsdf_cast_args(min_range, max_range, step)
    o = _tsdf_args(table, cap_vox, origin)
    _chk(poses, torch.float64, "poses"), _chk(dirs, torch.float32, "dirs")
    if poses.dim() != 3 or tuple(poses.shape[1:]) != (4, 4) or poses.shape[0] > 65535:
        raise ValueError("tsdf_raycast: poses (F,4,4), F <= 65535")
    if dirs.dim() != 2 or dirs.shape[1] != 3:
        raise ValueError("tsdf_raycast: dirs (R,3)")
    if int(min_count) < 1:
        raise ValueError("min_count >= 1")
    if blocks is not None:
        _tsdf_blocks_args(blocks, cap_blocks)
    dev, F, R = table.device, poses.shape[0], dirs.shape[0]
    with torch.cuda.device(dev):
        if out is None:
            out = (torch.empty(F, R, device=dev, dtype=torch.float32), torch.empty(F, R, 3, device=dev, dtype=torch.float32),
                   torch.empty(F, R, device=dev, dtype=torch.int32))
        rng, nrm, flag = out
        _chk(rng, torch.float32, "range"), _chk(nrm, torch.float32, "normals"), _chk(flag, torch.int32, "flag")
        if rng.numel() != F * R or nrm.numel() != 3 * F * R or flag.numel() != F * R:
            raise ValueError("tsdf_raycast: range (F,R), normals (F,R,3), flag (F,R)")
        n = F * R
        _lib.check(_lib.load().dpm_tsdf_raycast(
            _ptr(table), int(cap_vox), float(voxel), ctypes.addressof(o), None if blocks is None else _ptr(blocks),
            0 if blocks is None else int(cap_blocks), _ptr(poses) if F else None, F, _ptr(dirs) if R else None, R, lo, hi, h,
            int(min_count), _ptr(rng) if n else None, _ptr(nrm) if n else None, _ptr(flag) if n else None, _stream(table)),
            "dpm_tsdf_raycast")
    return rng, nrm, flag


# ------------------------------------------------------------------------------------------------------------
# Scan Context descriptors and their exhaustive search (csrc/scan_context.hip; loop_closure.py is the caller)
# ------------------------------------------------------------------------------------------------------------
SC_MAX_RINGS, SC_MAX_SECTORS, SC_MAX_K = 32, 64, 8


def scan_context_tables(rings: int, sectors: int, max_range: float):
    """the host tables of dpm_scan_context_build, formed in float64 and rounded once: ring_e2 (rings,) float32 = the squared
    ring edges e_1 .. e_rings, sector_cs (sectors/2 - 1, 2) float32 = (cos, sin) of 2 pi m / sectors, m = 1 .. sectors/2 - 1"""
    import numpy as np
    rings, sectors = int(rings), int(sectors)
    if not (1 <= rings <= SC_MAX_RINGS and 4 <= sectors <= SC_MAX_SECTORS and sectors % 2 == 0):
        raise ValueError(f"rings in 1..{SC_MAX_RINGS}, sectors even in 4..{SC_MAX_SECTORS}")
    m = np.arange(1, rings + 1, dtype=np.float64)
    ring_e2 = ((m * float(max_range) / rings) ** 2).astype(np.float32)
    a = 2.0 * np.pi * np.arange(1, sectors // 2, dtype=np.float64) / sectors
    sector_cs = np.stack([np.cos(a), np.sin(a)], axis=1).astype(np.float32)
    return np.ascontiguousarray(ring_e2), np.ascontiguousarray(sector_cs)


def _sc_outputs(out, F: int, rings: int, sectors: int, dev):
    if out is None:
        return (torch.empty(F, rings, sectors, device=dev, dtype=torch.float32),
                torch.empty(F, rings, sectors, device=dev, dtype=torch.float32), torch.empty(F, device=dev, dtype=torch.int64))
    raw, norm, mask = out
    _chk(raw, torch.float32, "raw"), _chk(norm, torch.float32, "norm"), _chk(mask, torch.int64, "mask")
    if raw.numel() != F * rings * sectors or norm.numel() != F * rings * sectors or mask.numel() != F:
        raise ValueError("scan context outputs: raw / norm (F,rings,sectors) fp32 and mask (F,) int64 (the mask's bits)")
    return raw, norm, mask


def scan_context_build(xyz: torch.Tensor, count: torch.Tensor, rings: int, sectors: int, max_range: float, min_range: float,
                       z_offset: float, tables=None, out=None):
    """dpm_scan_context_build: xyz (cap,3) fp32, count (1,) int32 on the GPU -> (raw (1,rings,sectors), norm (1,rings,sectors)
    fp32, mask (1,) int64 holding the 64 mask bits); `out` = (raw, norm, mask) views of one database row to write into.
    Three launches, no host synchronisation."""
    _lidar_arg(xyz, torch.float32, "xyz", xyz.dim() == 2 and xyz.shape[1] == 3, "(cap,3)")
    _lidar_arg(count, torch.int32, "count", count.numel() == 1, "(1,)")
    _lidar_dev(xyz=xyz, count=count)
    ring_e2, sector_cs = scan_context_tables(rings, sectors, max_range) if tables is None else tables
    dev = xyz.device
    with torch.cuda.device(dev):
        raw, norm, mask = _sc_outputs(out, 1, int(rings), int(sectors), dev)
        _lib.check(_lib.load().dpm_scan_context_build(_ptr(xyz) if xyz.shape[0] else None, _ptr(count), xyz.shape[0], int(rings),
                                                      int(sectors), float(max_range), float(min_range), float(z_offset),
                                                      ring_e2.ctypes.data, sector_cs.ctypes.data, _ptr(raw), _ptr(norm), _ptr(mask),
                                                      _stream(xyz)), "dpm_scan_context_build")
    return raw, norm, mask


def scan_context_build_batched(pcd: torch.Tensor, lengths: torch.Tensor, rings: int, sectors: int, max_range: float,
                               min_range: float, z_offset: float, tables=None, out=None):
    """dpm_scan_context_build_batched: pcd (F,3,N) fp32, lengths (F,) int32 -> (raw, norm (F,rings,sectors), mask (F,) int64)"""
    _lidar_arg(pcd, torch.float32, "pcd", pcd.dim() == 3 and pcd.shape[1] == 3 and pcd.shape[0] >= 1, "(F,3,N), F >= 1")
    _lidar_arg(lengths, torch.int32, "lengths", lengths.dim() == 1 and lengths.shape[0] == pcd.shape[0], "(F,)")
    _lidar_dev(pcd=pcd, lengths=lengths)
    ring_e2, sector_cs = scan_context_tables(rings, sectors, max_range) if tables is None else tables
    dev, (F, _, N) = pcd.device, pcd.shape
    with torch.cuda.device(dev):
        raw, norm, mask = _sc_outputs(out, F, int(rings), int(sectors), dev)
        _lib.check(_lib.load().dpm_scan_context_build_batched(_ptr(pcd) if N else None, _ptr(lengths), F, N, int(rings), int(sectors),
                                                              float(max_range), float(min_range), float(z_offset),
                                                              ring_e2.ctypes.data, sector_cs.ctypes.data, _ptr(raw), _ptr(norm),
                                                              _ptr(mask), _stream(pcd)), "dpm_scan_context_build_batched")
    return raw, norm, mask


def scan_context_search(q_norm: torch.Tensor, q_mask: torch.Tensor, db_norm: torch.Tensor, db_mask: torch.Tensor,
                        limit: torch.Tensor, k: int, rows: Optional[int] = None):
    """dpm_scan_context_search: queries (Q,rings,sectors) fp32 / (Q,) int64 against rows 0 .. limit[q]-1 of the first `rows`
    (default all) database rows (D,rings,sectors) / (D,) -> dist (Q,k) fp32, row (Q,k) int32, shift (Q,k) int32, ascending,
    padded with (inf, -1, -1).  Two launches, no host synchronisation."""
    _chk(q_norm, torch.float32, "q_norm"), _chk(q_mask, torch.int64, "q_mask"), _chk(limit, torch.int32, "limit")
    _chk(db_norm, torch.float32, "db_norm"), _chk(db_mask, torch.int64, "db_mask")
    if q_norm.dim() != 3 or db_norm.dim() != 3 or q_norm.shape[1:] != db_norm.shape[1:]:
        raise ValueError("scan_context_search: q_norm (Q,rings,sectors) and db_norm (D,rings,sectors)")
    Q, rings, sectors = q_norm.shape
    D = db_norm.shape[0] if rows is None else int(rows)
    if not 1 <= D <= db_norm.shape[0] or Q < 1 or q_mask.numel() != Q or limit.numel() != Q or db_mask.numel() != db_norm.shape[0]:
        raise ValueError("scan_context_search: Q >= 1, 1 <= rows <= D, q_mask / limit (Q,), db_mask (D,)")
    if not 1 <= int(k) <= SC_MAX_K:
        raise ValueError(f"k in 1..{SC_MAX_K}")
    dev = q_norm.device
    lib = _lib.load()
    with torch.cuda.device(dev):
        dist = torch.empty(Q, int(k), device=dev, dtype=torch.float32)
        row = torch.empty(Q, int(k), device=dev, dtype=torch.int32)
        shift = torch.empty(Q, int(k), device=dev, dtype=torch.int32)
        ws = torch.empty(lib.dpm_scan_context_search_workspace_bytes(Q, D, int(k)), device=dev, dtype=torch.uint8)
        _lib.check(lib.dpm_scan_context_search(_ptr(q_norm), _ptr(q_mask), Q, _ptr(db_norm), _ptr(db_mask), D, _ptr(limit), rings,
                                               sectors, int(k), _ptr(dist), _ptr(row), _ptr(shift), _ptr(ws), _stream(q_norm)),
                   "dpm_scan_context_search")
    return dist, row, shift
