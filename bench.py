#!/usr/bin/env python3
"""Headline benchmark: LiDAR frames/s for encode + match + register at 65 536 points per frame.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--dump-outputs DIR] [--full]

One "step" = one pass of the hot path over one batch of 64 synthetic scans per GPU
(deeppointmap_amd/synthetic.py, BASELINE.json config 2): Encoder.forward on the batch, then for
every frame one registration_forward against its predecessor (256 x 256 descriptors) and one
information matrix on the two full 65 536-point scans -- the per-frame work of
SlamSystem.step's extract + odometry stages (reference system/core.py:369-393).  Inputs are
resident in HBM before the timed region.  With N > 1 (launched by torch.distributed.run, one
process per GPU) every rank runs its own batch (weak scaling) and ships its descriptors and
edge table to rank 0 with one RCCL gather per step.

Prints ONE JSON line on rank 0.  A plain run sets up, warms up, times the K steps and prints the headline figure
(`value`, `ms_per_step`); nothing else runs.  --full adds everything else the benchmark measures or checks:
`roofline` for the dominant kernel (HIP-event timed inside the timed region) and `roofline_mfma`, `parity_gate` (the
last timed step against the reference's results; a failed gate voids `value` and exits 1), the extra measurements
(`sustained`, the kernels alone, PCIe-inclusive rate, latency mode, rank-0 consumer; --no-extras skips them) and
`cpu_baseline` (the oracle timed on the host cores over a bounded sample; N == 1 only; --cpu-frames 0 skips it).
--dump-outputs DIR writes what the last timed step returned on rank 0 (descriptors, edge table) as float32 .npy files.
"""
from __future__ import annotations

import argparse
import json
import os
import signal
import sys
import time

METRIC = "LiDAR frames/s (encode+match+register), 65 536 pts/frame"


def _sigterm_before_start(*_):
    """A launcher that lost another rank during start-up sends SIGTERM while this process is still importing torch (1-2 s, minutes on
    a fresh box): rank 0 leaves its ONE error line even then.  Replaced by Guard's handler as soon as the benchmark starts."""
    if os.environ.get("RANK", "0") == "0":
        os.write(1, (json.dumps({"metric": METRIC, "value": None, "unit": "frames/s", "n_gpus": int(os.environ.get("WORLD_SIZE", "1")),
                                 "higher_is_better": True, "phase": "start",
                                 "error": "SIGTERM from the launcher before the benchmark had started (another rank failed during start-up)"}) + "\n").encode())
    os._exit(143)


if __name__ == "__main__":
    signal.signal(signal.SIGTERM, _sigterm_before_start)

import torch  # noqa: E402

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

B_ALG_FRAME = 66_497_536  # algorithmic bytes per frame of the whole encoder
HBM_PEAK = 8.0e12         # B/s, MI355X spec (MI355X_MICROARCH.md)


def fps0_algorithmic_bytes(n_points: int, k: int) -> int:
    """Algorithmic bytes of ONE frame of the first-stage FPS launch: read xyz once, write idx + new_xyz."""
    return n_points * 12 + k * 4 + k * 12


def pmc_traffic_bytes(frames_per_launch: int):
    """HBM-side bytes per launch of the roofline kernel pair, from the committed rocprofv3 PMC passes
    (profiles/pmc_traffic.json; collected with separate --pmc FETCH_SIZE / WRITE_SIZE runs and corrected as
    MI355X_MICROARCH.md prescribes).  None if the file is missing or was taken at another batch size."""
    try:
        with open(os.path.join(ROOT, "profiles", "pmc_traffic.json")) as f:
            j = json.load(f)
        if j.get("frames_per_launch") != frames_per_launch:
            return None
        tot = 0
        for k in ("fps_bucket_kernel", "fps_str_sort_kernels"):
            tot += (2 * j[k]["FETCH_SIZE_KB"] + j[k]["WRITE_SIZE_KB"]) * 1024
        return int(tot)
    except Exception:
        return None


def parity_gate(desc: torch.Tensor, table: torch.Tensor, n_points: int) -> dict:
    """What the timed steps computed, held against the reference's own results for this workload (a parity
    gate with every number).  `desc` (>= 6, 131, 256) / `table` (>= 6, 56) are the rows the LAST timed step gathered on rank 0;
    row f of the table is the edge (f - 1, f).  Checked against fixtures made by importing the reference
    (tests/golden/make_golden.py; reference network/decoder/decoder.py:91-127, network/encoder/encoder.py:57-67,
    network/encoder/utils.py:232-262):
      * edges 0->1 ... 4->5 vs poses_full.npz: translation < 1e-4 m, rotation < 1e-4 rad, inlier count equal, |rmse| < 1e-3;
      * frame 0's 256 key points bit-equal to the first 256 picks of the reference's farthest point sampling (fps.npz) and to the
        reference encoder's coordinates (encoder_full.npz); descriptors of frames 0, 1 within 1.5e-5 of the reference's (five times what the
        reference moves by between one and eight torch threads, four times the 3.8e-6 observed; tests/conftest.py FEATURE_TOL);
      * every information matrix of the step finite and symmetric.
    The fixtures exist for the 65 536-point synthetic sequence only; another workload reports `checked: false`."""
    import numpy as np
    gold = os.path.join(ROOT, "tests", "golden")
    if n_points != 65536 or desc is None or desc.shape[0] < 6 or table.shape[0] < 6:
        return {"checked": False, "why": "fixtures cover the 65 536-point synthetic sequence, frames 0-5"}
    poses, fps, enc = (np.load(os.path.join(gold, f)) for f in ("poses_full.npz", "fps.npz", "encoder_full.npz"))
    d, t = desc[:6].detach().cpu().float(), table.detach().cpu().double()   # copies only: no device arithmetic for the gate
    max_dt = max_dr = max_drmse = 0.0
    n_conf_equal = True
    for f in range(1, 6):
        k = f"pair{f - 1}_{f}"
        R, T = t[f, 0:9].view(3, 3), t[f, 9:12].view(3, 1)
        max_dt = max(max_dt, float((T - torch.from_numpy(poses[k + ".T"]).double()).norm()))
        M = R.T @ torch.from_numpy(poses[k + ".R"]).double()
        max_dr = max(max_dr, float(np.arctan2(float(torch.linalg.norm(M - M.T)) / (2 * 2 ** 0.5), float((torch.trace(M) - 1) / 2))))
        max_drmse = max(max_drmse, abs(float(t[f, 12]) - float(poses[k + ".rmse"])))
        n_conf_equal &= int(t[f, 14]) == int(poses[k + ".n_conf"])
    key_xyz = d[0, 128:131, :]                                                         # metres: coordinates x 60 (fp32)
    fps_prefix_equal = bool(torch.equal(key_xyz, (torch.from_numpy(fps["synthetic0_k4096.new"][:256]) * 60.0).t().contiguous()))
    coor_equal = bool(torch.equal(key_xyz, torch.from_numpy(enc["synthetic0.coor"]) * 60.0))
    desc_err = max(float((d[f, :128] - torch.from_numpy(enc[f"synthetic{f}.fea"])).abs().max()) for f in (0, 1))
    info = t[:, 20:56].view(-1, 6, 6)
    info_ok = bool(torch.isfinite(info).all()) and bool(((info - info.transpose(1, 2)).abs() <= 1e-5 * info.abs().amax(dim=(1, 2), keepdim=True) + 1e-12).all())
    ok = (max_dt < 1e-4 and max_dr < 1e-4 and max_drmse < 1e-3 and n_conf_equal and fps_prefix_equal and coor_equal
          and desc_err < 1.5e-5 and info_ok)
    return {"checked": True, "ok": bool(ok), "pairs": 5, "max_dT_m": float(f"{max_dt:.3g}"), "max_dR_rad": float(f"{max_dr:.3g}"),
            "max_drmse": float(f"{max_drmse:.3g}"), "n_conf_equal": bool(n_conf_equal), "fps_prefix_equal": fps_prefix_equal,
            "keypoints_equal_reference": coor_equal, "descriptor_max_err": float(f"{desc_err:.3g}"),
            "information_matrices": int(info.shape[0]), "information_finite_symmetric": info_ok,
            "against": "tests/golden/{poses_full,fps,encoder_full}.npz (made by importing the reference)",
            "tolerance": "1e-4 m / 1e-4 rad (north_star); rmse 1e-3; descriptors 1.5e-5; key points and inlier counts exact"}


def cpu_baseline(n_frames: int, n_points: int, threads: int):
    """The oracle (CPU restatement, oracle/dpm_oracle.py) on a bounded sample of the same workload."""
    from oracle import dpm_oracle as O
    from deeppointmap_amd import synthetic
    from deeppointmap_amd.config import default_args
    from deeppointmap_amd.params import decoder_shapes, encoder_shapes
    from deeppointmap_amd.weights import procedural_state_dict
    torch.set_num_threads(threads)
    cfg = default_args()
    sde, sdd = procedural_state_dict(encoder_shapes(cfg)), procedural_state_dict(decoder_shapes(cfg))
    pts, pad = synthetic.frames(n_frames, n_points)
    t0 = time.perf_counter()
    descs = []
    for f in range(n_frames):  # the reference's single-thread mode encodes one frame per step (core.py:370)
        coor, fea, _ = O.encoder_forward(sde, cfg, pts[f:f + 1], pad[f:f + 1], fast_fps=True)
        descs.append(torch.cat([fea[0], coor[0] * 60.0], 0))
    t1 = time.perf_counter()
    for f in range(n_frames):
        s, d = (f - 1) % n_frames, f
        R, T, conf, rmse = O.registration_forward(sdd, cfg, descs[s], descs[d], 0.5)
        O.information_matrix(pts[s] * 60.0, pts[d] * 60.0, O.se3(R, T))
    t2 = time.perf_counter()
    return n_frames / (t2 - t0), (t1 - t0) / n_frames, (t2 - t1) / n_frames


DUMP_BYTES = 64_000_000   # --dump-outputs: all files together, headers included


def dump_outputs(directory: str, desc: torch.Tensor, table: torch.Tensor) -> dict:
    """--dump-outputs: what the last timed step returned on rank 0, as a caller of HotPath.submit / flush receives it --
    `descriptors.npy` (frames, 131, S): 128 features over the key points' coordinates in metres, and `edges.npy` (frames, 56):
    row f is the edge (f - 1, f), 20-float registration header | 6x6 information matrix (pipeline.EDGE_FLOATS) -- in float32.
    The scans are the seeded synthetic sequence, so two builds run with the same arguments compare file for file.  Whole frames
    are kept in order while both files fit DUMP_BYTES (all of them at the default 64 frames: 8.6 MB)."""
    import numpy as np
    d = desc.detach().float().cpu().numpy()
    e = table.detach().float().cpu().numpy()
    keep = min(d.shape[0], e.shape[0], (DUMP_BYTES - 2 * 4096) // (d[0].nbytes + e[0].nbytes))
    os.makedirs(directory, exist_ok=True)
    np.save(os.path.join(directory, "descriptors.npy"), np.ascontiguousarray(d[:keep]))
    np.save(os.path.join(directory, "edges.npy"), np.ascontiguousarray(e[:keep]))
    return {"frames": int(keep), "of": int(d.shape[0])}


class Guard:
    """Makes a run unable to hang or to die silently (the first N > 1 run on hardware happens under the driver, unobserved):
      * every phase leaves a rank-tagged breadcrumb on stderr and has a deadline; a watchdog thread that finds the deadline passed
        makes rank 0 print ONE JSON line carrying "error" (same metric / n_gpus keys as the result line) and ends the process;
      * an exception anywhere does the same (`fail`); so does SIGTERM from the launcher (another rank died).
    The process-group timeout (init_process_group(timeout=...)) is set to the same collective budget, so RCCL's own watchdog
    raises in the rank that waits instead of blocking for its default ten minutes."""

    def __init__(self, rank: int, world: int, args):
        import signal
        import threading
        self.rank, self.world, self.args = rank, world, args
        self.t0 = time.time()
        self.phase_name, self.deadline = "start", time.time() + 300
        self._done = False
        self._lock = threading.Lock()
        threading.Thread(target=self._watch, daemon=True).start()
        try:
            signal.signal(signal.SIGTERM, lambda *_: self.fail("SIGTERM from the launcher (another rank failed or the run was cancelled)", 143))
        except ValueError:   # not the main thread
            pass

    def phase(self, name: str, budget_s: float) -> None:
        self.phase_name, self.deadline = name, time.time() + budget_s
        print(f"[bench rank {self.rank}/{self.world} +{time.time() - self.t0:6.1f}s] {name} (budget {budget_s:.0f} s)", file=sys.stderr, flush=True)

    def _watch(self) -> None:
        while not self._done:
            time.sleep(0.5)
            if not self._done and time.time() > self.deadline:
                self.fail(f"phase '{self.phase_name}' exceeded its budget: a collective or a kernel did not complete", 124)

    def fail(self, why: str, code: int = 1) -> None:
        if not self._lock.acquire(blocking=False):   # somebody is failing already (a signal handler must not wait for its own thread)
            return
        if self._done:
            self._lock.release()
            return
        self._done = True
        msg = f"{why} [rank {self.rank}/{self.world}, phase '{self.phase_name}', +{time.time() - self.t0:.1f} s]"
        # raw writes: this may run inside a signal handler that interrupted a print, or next to a thread that holds a stream's lock
        os.write(2, f"[bench rank {self.rank}/{self.world}] ERROR: {msg}\n".encode())
        if self.rank == 0:
            os.write(1, (json.dumps({"metric": METRIC, "value": None, "unit": "frames/s", "n_gpus": self.world, "steps": self.args.steps,
                                     "warmup": self.args.warmup, "higher_is_better": True, "error": msg, "phase": self.phase_name}) + "\n").encode())
        os._exit(code)    # not sys.exit: a thread blocked inside a collective would keep the process alive

    def finish(self) -> None:
        self._done = True


def self_launch_command(argv, n_gpus: int, port: int | None = None) -> list:
    """The command `python bench.py --gpus N ...` turns itself into when no launcher set WORLD_SIZE: torch.distributed.run with one
    process per GPU on this node, rendezvous on 127.0.0.1 (the container's host name may not resolve), a free port unless given."""
    if port is None:
        import socket
        with socket.socket() as sock:
            sock.bind(("127.0.0.1", 0))
            port = sock.getsockname()[1]
    return [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n_gpus}", "--master-addr", "127.0.0.1",
            "--master-port", str(port), os.path.abspath(__file__), *argv]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--frames", type=int, default=64, help="frames per GPU per step")
    ap.add_argument("--points", type=int, default=65536)
    ap.add_argument("--cpu-frames", type=int, default=64, help="--full: frames of the cpu_baseline sample (0 = skip; default: the whole batch)")
    ap.add_argument("--no-extras", action="store_true", help="--full: skip the extra measurements (PCIe-inclusive rate, latency mode, rank-0 consumer)")
    ap.add_argument("--no-pipeline", action="store_true", help="run every step start-to-finish on one stream")
    ap.add_argument("--geometry-depth", type=int, default=None, help="geometry passes kept in flight (pipeline tuning)")
    ap.add_argument("--geometry-group", type=int, default=None, help="batches per first-level sampling launch (pipeline tuning)")
    ap.add_argument("--geometry-knn", type=int, default=None, help="1: neighbour queries run in the geometry stage, 0: in the feature stage")
    ap.add_argument("--feature-streams", type=int, default=None, help="feature-stage streams (pipeline tuning)")
    ap.add_argument("--geometry-knn-from", type=int, default=None, help="first downsampling level whose neighbour queries run in the geometry stage (pipeline tuning; -1 = none)")
    ap.add_argument("--feature-split", type=int, default=None, help="downsampling level at which the feature stage moves to its second stream (pipeline tuning; 0 = one stage)")
    ap.add_argument("--wait-for-caller-stream", type=int, default=1, choices=(0, 1),
                    help="HotPath.inputs_on_caller_stream: 1 (the library's default) = the geometry stage of a batch waits for the caller's "
                         "stream; 0 = the inputs are complete at submit() (true of this benchmark's resident scans) and it does not")
    ap.add_argument("--stages", action="store_true", help="also print a per-stage time breakdown to stderr")
    ap.add_argument("--backend", default="nccl", choices=("nccl", "gloo"),
                    help="process-group backend for --gpus > 1; gloo (ranks folded onto the visible GPUs) exists only to dry-run "
                         "the N>1 code path on a single-GPU box and is recorded in config.parallelism")
    ap.add_argument("--allow-knobs", action="store_true",
                    help="run although DPM_* variables are set / an experimental library is loaded (A/B measurements); they are "
                         "recorded under config.knobs and the line is not a headline number")
    ap.add_argument("--collective-timeout", type=float, default=120.0,
                    help="seconds a collective (and the process-group rendezvous) may take before the run ends with an error line")
    ap.add_argument("--force-collectives", action="store_true",
                    help="--gpus 1 only: create a one-rank process group and issue the step's gather anyway (executes the RCCL call "
                         "path on a single-GPU box; recorded in config.parallelism)")
    ap.add_argument("--inject-failure", default="none", choices=("none", "hang-in-gather", "raise-in-step"),
                    help="test hook for the guard: the named failure happens in the first timed step")
    ap.add_argument("--full", action="store_true",
                    help="also measure and check everything beyond the headline figure: roofline figures, the parity gate against "
                         "the reference's results, the extra measurements and the cpu_baseline (a plain run times the steps only)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last one returned on rank 0 as DIR/<name>.npy (float32): "
                         "descriptors (frames, 131, 256) and edges (frames, 56); at most 64 MB, whole frames kept in order")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # started as `python bench.py --gpus N` (the N = 1 command form): become the launcher -- one process per GPU, rendezvous on
        # the loopback address.  exec, not spawn: signals and the exit code are the launcher's, stdout carries rank 0's one line.
        cmd = self_launch_command(sys.argv[1:], args.gpus)
        print("[bench] no launcher in the environment: " + " ".join(cmd), file=sys.stderr, flush=True)
        os.execv(cmd[0], cmd)
    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    guard = Guard(rank, world, args)
    try:
        run(args, guard, rank, world)
    except SystemExit as e:
        if e.code not in (0, None):
            guard.fail(str(e.code) if not isinstance(e.code, int) else f"exit code {e.code}", e.code if isinstance(e.code, int) else 1)
        raise
    except BaseException as e:  # noqa: BLE001 -- whatever it is, rank 0 says so in the record
        import traceback
        traceback.print_exc()
        guard.fail(f"{type(e).__name__}: {e}")
    guard.finish()


def run(args, guard, rank, world):
    # Tamper evidence: the headline number comes from the shipped library and the shipped host settings or not at all.
    # DPM_LIB swaps the library, the other DPM_* names are what an experimental build (-DDPM_EXPERIMENT) or
    # deeppointmap_amd.knobs.apply_env() would read -- some of them skip work.
    from deeppointmap_amd import knobs
    env_knobs = knobs.env_knobs()
    if env_knobs and not args.allow_knobs:
        raise SystemExit("bench.py: refusing to run with measurement knobs in the environment (" + ", ".join(env_knobs) +
                         "); unset them, or pass --allow-knobs to run an A/B measurement that records them in the JSON line")
    if args.allow_knobs:
        knobs.apply_env()

    local = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}")
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a GPU (the hot path has no CPU fallback)")
    # one rank per GPU; --backend gloo (+ ranks folded onto the visible GPUs) exists only to dry-run the N>1 code path on a
    # single-GPU box
    backend = args.backend
    local = local % torch.cuda.device_count() if backend != "nccl" else local
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    import datetime
    import torch.distributed as dist
    forced = args.force_collectives and world == 1   # one rank, collectives issued anyway
    pg_timeout = datetime.timedelta(seconds=args.collective_timeout)
    ranks_seen = None
    if world > 1 or forced:
        guard.phase("process-group rendezvous", args.collective_timeout + 30)
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29511")
        kw = dict(rank=0, world_size=1) if forced else {}
        if backend == "nccl":
            dist.init_process_group(backend="nccl", device_id=dev, timeout=pg_timeout, **kw)
        else:
            dist.init_process_group(backend=backend, timeout=pg_timeout, **kw)
        # who is here: the record must show N ranks on N distinct devices (a launcher that folded two ranks onto one GPU, or
        # a communicator that saw fewer ranks than --gpus, would otherwise produce a plausible line)
        guard.phase("rank census (first collective)", args.collective_timeout + 30)
        props = torch.cuda.get_device_properties(dev)
        me = {"rank": rank, "local_rank": local, "device": torch.cuda.current_device(),
              "pci": f"{props.pci_domain_id:04x}:{props.pci_bus_id:02x}:{props.pci_device_id:02x}", "uuid": str(getattr(props, "uuid", ""))}
        ranks_seen = [None] * dist.get_world_size()
        dist.all_gather_object(ranks_seen, me)
        if dist.get_world_size() != args.gpus:
            raise SystemExit(f"process group has {dist.get_world_size()} ranks, --gpus {args.gpus}")
        if backend == "nccl" and len({r["pci"] for r in ranks_seen}) != len(ranks_seen):
            raise SystemExit(f"ranks share devices: {ranks_seen}")

    from deeppointmap_amd import _lib, ops, synthetic
    if _lib.experimental() and not args.allow_knobs:
        raise SystemExit(f"bench.py: {_lib.LIB_PATH} is an experimental build (-DDPM_EXPERIMENT); refusing without --allow-knobs")
    from deeppointmap_amd.config import default_args
    from deeppointmap_amd.decoder import Decoder
    from deeppointmap_amd.encoder import Encoder
    from deeppointmap_amd.pipeline import HotPath
    from deeppointmap_amd.shard import gather_step_results
    from deeppointmap_amd.weights import init_procedural

    cfg = default_args()
    hot = HotPath(init_procedural(Encoder(cfg)).to(dev), init_procedural(Decoder(cfg)).to(dev))
    if args.geometry_depth is not None:
        hot.geometry_depth = args.geometry_depth
    if args.geometry_group is not None:
        hot.geometry_group = args.geometry_group
    if args.geometry_knn is not None:
        hot.encoder.presample_neighbours = bool(args.geometry_knn)
    if args.geometry_knn_from is not None:
        hot.encoder.presample_neighbours_from = args.geometry_knn_from if args.geometry_knn_from >= 0 else None
    if args.feature_streams is not None:
        hot.feature_streams = args.feature_streams
    if args.feature_split is not None:
        hot.feature_split = args.feature_split
    # hot.reserve_bytes stays at HotPath's default (16 GiB of allocator segments up front, pipeline.py): the shipped configuration
    hot.inputs_on_caller_stream = bool(args.wait_for_caller_stream)
    hot.chain = world > 1  # block-boundary edges come from the neighbour rank's last frame (shard.exchange_halo)
    F, N = args.frames, args.points
    pts, pad = synthetic.frames(F, N, start=rank * F)  # every rank owns its own block of the sequence
    pts, pad = pts.to(dev), pad.to(dev)
    pcd_m = (pts * synthetic.COOR_SCALE).contiguous()  # ScanPack.full_pcd: the scans in metres
    torch.cuda.synchronize()

    # --full: HIP events around the dominant kernel (first-stage FPS), recorded on the launch stream
    fps_events, fps_frames = [], [0]
    orig_fps = ops.fps

    def timed_fps(xyz, lengths, K, algo=0):
        fps_frames[0] = xyz.shape[0]
        if xyz.shape[1] != N:
            return orig_fps(xyz, lengths, K, algo)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = orig_fps(xyz, lengths, K, algo)
        e1.record()
        fps_events.append((e0, e1))
        return out

    import deeppointmap_amd.encoder as enc_mod
    if args.full:
        enc_mod.ops.fps = timed_fps

    # ... and around the widest dense contraction of the path (the decoder's 256 -> 768 attention projections over
    # all tokens of the batch), the MFMA-bound representative reported as `roofline_mfma`
    gemm_events, gemm_flops = [], [0]
    orig_linear = ops.linear

    def timed_linear(x, W, *a, **k):
        # only the launches over ALL token rows of the batch's pairs (2 * F sequences of 256 tokens: four per step); the two
        # per-frame projections of the first decoder block are half as long and would dilute the average
        if W.shape[0] != 768 or x.shape[0] != 2 * F * 256:
            return orig_linear(x, W, *a, **k)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = orig_linear(x, W, *a, **k)
        e1.record()
        gemm_events.append((e0, e1))
        gemm_flops[0] = 2 * x.shape[0] * W.shape[0] * W.shape[1]
        return out

    if args.full:
        ops.linear = timed_linear
    # (since round 5 that projection hands K / V to the attention kernel as operand planes: ops.linear_kvplanes, same contraction)
    orig_kvplanes = ops.linear_kvplanes
    gemm_kvp = [False]

    def timed_kvplanes(x, W, *a, **k):
        if W.shape[0] != 768 or x.shape[0] != 2 * F * 256:
            return orig_kvplanes(x, W, *a, **k)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = orig_kvplanes(x, W, *a, **k)
        e1.record()
        if out is not None:
            gemm_events.append((e0, e1))
            gemm_flops[0] = 2 * x.shape[0] * W.shape[0] * W.shape[1]
            gemm_kvp[0] = True
        return out

    if args.full:
        ops.linear_kvplanes = timed_kvplanes

    last_gathered = [None]

    timed = [False]

    def step():
        if inject[0] == "raise-in-step" and timed[0]:
            raise RuntimeError("injected failure (--inject-failure raise-in-step)")
        # Streaming mode (HotPath.submit): this batch's input staging + first-level FPS start on a side HIP
        # stream and overlap with the previous batch's remaining stages on the main stream.  Edges stay on the
        # device in `table` (header | information per frame); no host sync inside a step.
        if args.no_pipeline:
            desc, edges, table = hot.step(pts, pad, pcd_m, materialize=False)
            gather((desc, table))
            return
        done = hot.submit(pts, pad, pcd_m)
        if done is not None:
            gather(done)

    comm = torch.cuda.Stream(device=dev) if (world > 1 or forced) else None
    inject = [args.inject_failure]

    def gather(done):
        # the step's one collective runs on a stream of its own: the caller's stream carries the next batch's feature stage,
        # which must not wait for 8.6 MB per rank to cross xGMI (submit / flush made the caller's stream wait for the results)
        if comm is None:
            last_gathered[0] = gather_step_results(done[0].contiguous(), done[1])
            return
        if inject[0] == "hang-in-gather" and timed[0]:
            time.sleep(10 ** 6)          # a collective that never completes, as the guard sees it
        comm.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(comm):
            for t in done:
                t.record_stream(comm)
            last_gathered[0] = gather_step_results(done[0].contiguous(), done[1], force=forced)

    def drain():  # the batches still in the pipe are finished INSIDE the timed region
        for done in hot.flush():
            gather(done)

    def fence():
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    # One-time initialisation that is not a benchmark step: a two-frame, 20 000-point pass makes the HIP runtime load
    # the kernels' code objects and fills the weight-derived caches (a first launch of each kernel costs milliseconds),
    # so that a run with --warmup 0 measures the path and not the loader.  Nothing of the timed workload is computed.
    guard.phase("one-time initialisation (code objects, weight-derived caches)", 300)
    init_pts, init_pad = synthetic.frames(2, 20000, start=10_000)
    hot.step(init_pts.to(dev), init_pad.to(dev), (init_pts * synthetic.COOR_SCALE).contiguous().to(dev), materialize=False)
    torch.cuda.synchronize()
    del init_pts, init_pad
    torch.cuda.empty_cache()  # its (small) buffers do not stay behind in the caching allocator
    fps_events.clear()
    gemm_events.clear()

    guard.phase(f"warm-up ({args.warmup} steps)", args.collective_timeout + 60 + 1.0 * args.warmup)
    for _ in range(args.warmup):
        step()
    drain()
    fps_events.clear()
    gemm_events.clear()
    fence()
    guard.phase(f"timed region ({args.steps} steps)", args.collective_timeout + 1.0 * args.steps)
    timed[0] = True
    t0 = time.perf_counter()
    for _ in range(args.steps):
        step()
    drain()
    fence()
    dt = time.perf_counter() - t0
    timed[0] = False
    guard.phase("after the timed region (parity gate, extra measurements)" if args.full else "after the timed region", 600)
    if world > 1:
        tmax = torch.tensor([dt], device=dev, dtype=torch.float64)
        dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
        dt = float(tmax)
    # the rows the last timed step gathered: written out and held against the reference's results before anything else touches
    # the pipeline's buffers
    gate = None
    if rank == 0:
        gd, gt = last_gathered[0] if last_gathered[0] is not None else (None, None)
        if args.dump_outputs is not None:
            if gd is None:
                raise RuntimeError("--dump-outputs: the timed steps gathered nothing")
            dump_outputs(args.dump_outputs, gd, gt)
        if args.full:
            gate = parity_gate(gd, gt, N) if gd is not None else {"checked": False, "why": "nothing gathered"}
    fps_ms = sum(a.elapsed_time(b) for a, b in fps_events) / max(len(fps_events), 1)
    gemm_ms = sum(a.elapsed_time(b) for a, b in gemm_events) / max(len(gemm_events), 1)

    # ---- extra measurements, outside the timed region and never part of `value` ---------------------------------
    extras = {}
    alone = {}
    if args.full and not args.no_extras and not args.no_pipeline:
        # (-1) the same steps again for a few seconds (round-5 review: the timed region of the default run is 0.09 s, too short for a
        #      device monitor sampling beside the run to see a busy GPU): frames/s over >= 2.5 s with the parity gate on its last step.
        #      Every rank runs it (the steps carry the gather).
        n_sus = max(args.steps, int(2.5 / max(dt / args.steps, 1e-4)) + 1)
        fence()
        t1 = time.perf_counter()
        for _ in range(n_sus):
            step()
        drain()
        fence()
        sus = time.perf_counter() - t1
        if rank == 0:
            gd2, gt2 = last_gathered[0] if last_gathered[0] is not None else (None, None)
            g2 = parity_gate(gd2, gt2, N) if gd2 is not None else {"checked": False}
            extras["sustained"] = {"steps": n_sus, "seconds": round(sus, 2), "value": round(world * F * n_sus / sus, 1), "unit": "frames/s",
                                   "ms_per_step": round(sus / n_sus * 1e3, 3), "clock": "rank 0", "parity_gate_ok": g2.get("ok"),
                                   "max_dT_m": g2.get("max_dT_m"), "descriptor_max_err": g2.get("descriptor_max_err")}
    if args.full and not args.no_extras and rank == 0:
        # (0) the two roofline kernels ALONE on the chip (the figures inside the timed region include what the other
        #     pipeline stages cost them): first-stage sampling of one 64-frame batch, and the 256 -> 768 projection
        def alone_ms(fn, n):
            fn()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(n):
                fn()
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1) / n
        xyz0, len0 = ops.prepare_points(pts, pad)
        alone["fps_ms"] = alone_ms(lambda: orig_fps(xyz0, len0, cfg.encoder.npoint[0]), 3)
        if gemm_flops[0]:
            rows = gemm_flops[0] // (2 * 768 * 256)
            gx, gw, gb = torch.randn(rows, 256, device=dev), torch.randn(768, 256, device=dev) / 16, torch.randn(768, device=dev)
            go = torch.empty(rows, 768, device=dev)
            if gemm_kvp[0]:
                alone["gemm_ms"] = alone_ms(lambda: orig_kvplanes(gx, gw, gb, 256), 20)
            else:
                alone["gemm_ms"] = alone_ms(lambda: orig_linear(gx, gw, gb, out=go), 20)
            del gx, gw, gb, go
        del xyz0, len0
    if args.full and not args.no_extras:
        if world == 1 and not args.no_pipeline:
            # (1) PCIe-inclusive rate: the scans start in pinned host memory and are copied in every step (the metres copy
            #     for the information matrix is derived on the device, as a caller holding one scan buffer would)
            pts_h, pad_h = pts.cpu().pin_memory(), pad.cpu().pin_memory()
            up = torch.cuda.Stream(device=dev)

            def pcie_step():
                with torch.cuda.stream(up):
                    p = pts_h.to(dev, non_blocking=True)
                    q = pad_h.to(dev, non_blocking=True)
                    m = p * synthetic.COOR_SCALE
                    ev = up.record_event()
                torch.cuda.current_stream(dev).wait_event(ev)
                for g_ in hot.geometry_streams():
                    g_.wait_event(ev)
                hot.submit(p, q, m)
            for _ in range(3):
                pcie_step()
            hot.flush()
            fence()
            t1 = time.perf_counter()
            n_pcie = 20
            for _ in range(n_pcie):
                pcie_step()
            hot.flush()
            fence()
            extras["pcie_inclusive_fps"] = round(F * n_pcie / (time.perf_counter() - t1), 1)
            # (2) latency mode: one scan at a time, host to pose, as the reference's single-thread SlamSystem.step
            #     consumes them (system/core.py:360-393)
            lat_hot = HotPath(hot.encoder, hot.decoder)

            from deeppointmap_amd.registration import PoseTool, calculate_information_matrix_from_pcd

            def lat_run(frames):
                # per frame what SlamSystem.step + OdometryThread.odometry do (core.py:369-393, odometry.py:103-127): upload,
                # extract, registration_forward against the predecessor (R, T, rmse back on the host), information matrix
                prev = None
                for i in frames:
                    p1 = pts_h[i:i + 1].to(dev, non_blocking=True)
                    d1 = lat_hot.extract(p1, pad_h[i:i + 1].to(dev, non_blocking=True))[0]
                    m1 = p1[0] * synthetic.COOR_SCALE
                    if prev is not None:
                        R, T, conf, rmse = hot.decoder.registration_forward(prev[0], d1, num_sample=0.5)
                        calculate_information_matrix_from_pcd(prev[1], m1, PoseTool.SE3(R.cpu(), T.cpu()), device=dev)
                    prev = (d1, m1)
            lat_run(range(4))  # the one-frame shapes, warm (code objects, allocator, weight-derived caches)
            fence()
            t1 = time.perf_counter()
            n_lat = min(32, F)
            lat_run(range(n_lat))
            fence()
            extras["latency_mode_ms_per_frame"] = round((time.perf_counter() - t1) / n_lat * 1e3, 3)
        if world > 1:
            # (3) the sequential consumer on rank 0 (key-frame gating, scan-to-map against 16-scan tiles, pose-graph
            #     optimisation): the Amdahl term of the sharded path, measured on the last gathered step
            ms = None
            if rank == 0 and last_gathered[0] is not None and last_gathered[0][0] is not None:
                try:   # an extra must never cost the line (nor leave the other ranks alone at the fence below)
                    from deeppointmap_amd.consumer import Rank0Consumer
                    # the reference's step after the extraction on the gathered rows, with the SHIPPED thresholds
                    # (configs/infer/*.yaml: drop rules, 'auto' key-frame distance, loop closure).  Procedural weights give
                    # meaningless registrations -- rmse of metres, poses a random walk on which the partner search and the
                    # key-frame rule see no trajectory -- so the rows carry the synthetic sequence's TRUE relative poses and the
                    # quality figures of a good registration (rmse 0.15 m, confidence 0.9): the gating then meets what it meets in
                    # deployment (0.5 m per frame, a key-frame every ~20 frames, the predecessor chain intact).  Every device call
                    # of the step still runs on the real descriptors: scan-to-map per key-frame (its result is refused by
                    # mapping.py:193 -- rmse above both the threshold and the row's), the loop-detection batch per key-frame
                    # (nothing proposed above 0.7); `optimize_every` stands in for the optimiser runs verified loops would trigger.
                    slam = dict(enable_loop_closure=True)
                    cons = Rank0Consumer(hot.decoder, dev, slam_args=slam, optimize_every=16)
                    gd, gt = last_gathered[0]
                    gt = gt.clone()
                    truth = torch.stack([synthetic.relative_pose(g - 1, g) for g in range(gt.shape[0])]).to(gt)
                    gt[:, 0:9], gt[:, 9:12] = truth[:, :3, :3].reshape(-1, 9), truth[:, :3, 3]
                    gt[:, 12], gt[:, 16] = 0.15, 0.9
                    cons.consume(gd, gt)           # fills the map (first tiles are short), captures the registration shapes
                    cons.consume(gd, gt)
                    before = dict(cons.stats)
                    ms = [cons.consume(gd, gt) for _ in range(2)]
                    extras["rank0_serial_ms"] = round(sum(ms) / len(ms), 2)
                    extras["rank0_consumer"] = {"frames_per_step": int(gd.shape[0]), "key_frame_distance": "auto (shipped config)",
                                                "key_frames_per_step": (cons.stats["keyframes"] - before["keyframes"]) / 2,
                                                "scan_to_map_registrations_per_step": (cons.stats["s2m"] - before["s2m"]) / 2,
                                                "loop_detection_batches_per_step": (cons.stats["loop_batches"] - before["loop_batches"]) / 2,
                                                "registrations_on_rank0_per_step": (cons.stats["re_registrations"] - before["re_registrations"]) / 2,
                                                "pose_graph_optimisations": cons.stats["optimisations"],
                                                "synthetic_rows": True,
                                                "note": "sequential SLAM work that stays on rank 0 (mapping.py:52-201, "
                                                        "loop_closure.py:56-307); not part of `value`.  The gathered edge rows "
                                                        "are OVERWRITTEN with the synthetic sequence's true relative poses and a fixed "
                                                        "rmse 0.15 / confidence 0.9 (procedural weights give meaningless "
                                                        "registrations); under these rows every scan-to-map result is refused and no "
                                                        "loop is proposed, so the figure prices the device calls and the gating of a "
                                                        "loop-free drive, not a measured SLAM run; the same rows are consumed on every "
                                                        "call (row 0 = the edge from the previous call's last frame)"}
                except Exception as e:  # noqa: BLE001
                    extras["rank0_consumer_error"] = f"{type(e).__name__}: {e}"
            fence()

    if args.stages and rank == 0:
        def tm(fn, n=3):
            fn()
            torch.cuda.synchronize()
            t = time.perf_counter()
            for _ in range(n):
                fn()
            torch.cuda.synchronize()
            return (time.perf_counter() - t) / n * 1e3
        desc = hot.extract(pts, pad)
        pairs = [((f - 1) % F, f) for f in range(F)]
        print(f"[stages] encode {tm(lambda: hot.extract(pts, pad)):.2f} ms | "
              f"register x{F} {tm(lambda: hot.register(desc, None, pairs)):.2f} ms | "
              f"register+info x{F} {tm(lambda: hot.register(desc, pcd_m, pairs)):.2f} ms | fps0 kernel pair " +
              (f"{fps_ms:.3f} ms" if args.full else "timed with --full"), file=sys.stderr)

    if rank == 0:
        value = world * F * args.steps / dt
        alg = fps0_algorithmic_bytes(N, cfg.encoder.npoint[0]) * F  # one launch handles the rank's F frames
        achieved = alg / (fps_ms * 1e-3) / 1e9 if fps_ms > 0 else 0.0
        line = {
            "metric": METRIC,
            "value": round(value, 3), "unit": "frames/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": round(dt / args.steps * 1e3, 3), "higher_is_better": True, "scaling": "weak",
            "vs_baseline": None,
            "dtype": "f32 (attention scores K Q^T and P V" + (f", Linear / Conv1d (+ LayerNorm) layers with K <= {knobs.BF16X3_MAX_K}" if knobs.GEMM_BF16X3 else "") +
                     " as exact three-way bf16 splits: 6 bf16 products per fp32 product, fp32 accumulate -- fp32 accuracy, bf16 matrix "
                     "pipe; all else fp32)",
            "data": "synthetic",
            "config": {"workload": f"synthetic {F}x{N}-pt scans per GPU: Encoder.forward + consecutive-frame "
                                   "registration_forward (256x256) + information matrix per frame",
                       "frames_per_gpu_per_step": F, "points_per_frame": N,
                       "parallelism": f"frame-sharded x{world}, one RCCL gather of descriptors+edges per step" +
                                      ("" if backend == "nccl" or world == 1 else f" (DRY RUN over {backend}, ranks folded onto the visible GPUs)") +
                                      (" (ONE rank, collectives forced: --force-collectives)" if forced else ""),
                       "pipeline": "none" if args.no_pipeline else "HIP-stream pipeline: geometry (staging+FPS chain) of batches i, i-1 on two alternating streams | features of batch i-2 | registration+information matrices of batch i-3",
                       "weights": "procedural (deeppointmap_amd/weights.py)",
                       "allocator_reserve_gib": 0 if args.no_pipeline else hot.reserve_bytes >> 30,
                       "geometry_waits_for_caller_stream": bool(hot.inputs_on_caller_stream)},
        }
        if args.full:   # the dominant kernel, HIP-event timed inside the timed region
            line["roofline"] = {"kernel": "str_chunk/str_xoffsets/str_ysort kernels + fps_bucket_kernel (stage-0 farthest point sampling: Sort-Tile-Recursive packing, then the sampling rounds)",
                                "bound": "hbm", "achieved": round(achieved, 3), "peak": HBM_PEAK / 1e9, "unit": "GB/s",
                                "frac": round(achieved / (HBM_PEAK / 1e9), 6), "traffic": pmc_traffic_bytes(F),
                                "traffic_source": "profiles/pmc_traffic.json (rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes of these "
                                                  "kernels at this batch size, committed; not re-measured in this run)",
                                "avg_launch_ms": round(fps_ms, 4), "algorithmic_bytes_per_launch": alg,
                                "whole_path_frac": round(value / world * B_ALG_FRAME / HBM_PEAK, 6),
                                "us_per_round": round(fps_ms * 1e3 / (cfg.encoder.npoint[0] - 1), 3),
                                "note": "avg_launch_ms exceeds ms_per_step because two launches (two batches' geometry stages) are "
                                        "in flight on alternating streams; "
                                        "FPS is a chain of 4095 dependent argmax rounds per frame, one CU per frame: latency-"
                                        "bound by construction (us_per_round is the figure that matters); traffic > algorithmic "
                                        "bytes because each round re-reads the ~7 buckets the new point can change -- the "
                                        "reference's loop re-reads the WHOLE frame every round (4095 x 65536 x 16 B = 4.3 GB "
                                        "per frame, 275 GB per launch), the bucket pruning cuts that ~85x; see DESIGN.md"}
        if ranks_seen is not None:    # N ranks on N distinct devices, as the process group itself reported them
            line["ranks"] = {"world_size": dist.get_world_size(), "backend": dist.get_backend(), "collective_timeout_s": args.collective_timeout,
                             "members": ranks_seen}
        if args.full:
            line["parity_gate"] = gate   # what the timed steps computed against the reference's results for this workload
        if "fps_ms" in alone:   # the same kernel pair with the chip to itself (outside the timed region)
            line["roofline"]["alone"] = {"launch_ms": round(alone["fps_ms"], 4),
                                         "us_per_round": round(alone["fps_ms"] * 1e3 / (cfg.encoder.npoint[0] - 1), 3),
                                         "frac": round(alg / (alone["fps_ms"] * 1e-3) / HBM_PEAK, 6)}
        if args.allow_knobs:   # an A/B measurement, not a headline number: say what was different
            line["config"]["knobs"] = dict(env_knobs, experimental_library=_lib.experimental(), library=_lib.LIB_PATH,
                                           host={"FPS_ALGO": knobs.FPS_ALGO, "FUSED_LN": knobs.FUSED_LN,
                                                 "DEDUP_FRAMES": knobs.DEDUP_FRAMES})
        line.update(extras)
        if "rank0_serial_ms" in extras:
            line["value_with_rank0_consumer"] = round(world * F / (dt / args.steps + extras["rank0_serial_ms"] * 1e-3), 1)
        if args.full and gemm_ms > 0:
            rows = gemm_flops[0] // (2 * 768 * 256)
            if knobs.GEMM_BF16X3:
                # the projection runs on the bf16 matrix pipe: every fp32 operand split exactly into three bf16 terms, six
                # term products per fp32 product.  `achieved` counts the EXECUTED bf16 flops against the dense bf16 peak;
                # `fp32_equivalent` is the fp32 product it delivers against the fp32 matrix peak it would otherwise run at.
                PEAK, mult = 2500.0, 6
                kern = (("gemm_b3_kvp_kernel<128,1>" if gemm_kvp[0] else "gemm_b3_kernel<64,128>") +
                        " (csrc/gemm_b3.hip: fp32 GEMM as an exact three-way bf16 split, 6 products, fp32 "
                        f"accumulate) on the decoder's 256->768 attention projections ({rows} token rows per launch" +
                        ("; K / V leave the epilogue as the attention kernel's bf16 operand planes" if gemm_kvp[0] else "") + ")")
                note = ("v_mfma_f32_16x16x32_bf16, dense bf16 peak ~2500 TFLOP/s; achieved = 6 x the fp32 product's flops; timed "
                        "with HIP events on its launch stream while the other pipeline stages share the chip")
            else:
                PEAK, mult = 157.3, 1
                kern = f"gemm_nt_mfma_kernel<64,64> on the decoder's 256->768 attention projections ({rows} token rows per launch)"
                note = ("exact-fp32 MFMA (v_mfma_f32_16x16x4_f32, 157.3 TFLOP/s dense peak); timed with HIP events on its "
                        "launch stream while the other pipeline stages share the chip")
            tf = gemm_flops[0] / (gemm_ms * 1e-3) / 1e12
            line["roofline_mfma"] = {"kernel": kern, "bound": "mfma", "achieved": round(mult * tf, 2), "peak": PEAK,
                                     "unit": "TFLOP/s", "frac": round(mult * tf / PEAK, 4), "avg_launch_ms": round(gemm_ms, 4),
                                     "flops_per_launch": mult * gemm_flops[0], "note": note}
            if mult > 1:
                line["roofline_mfma"]["fp32_equivalent"] = {"achieved": round(tf, 2), "peak": 157.3, "frac": round(tf / 157.3, 4),
                                                            "flops_per_launch": gemm_flops[0]}
            if "gemm_ms" in alone:  # the same launch with the chip to itself (outside the timed region)
                ta = gemm_flops[0] / (alone["gemm_ms"] * 1e-3) / 1e12
                line["roofline_mfma"]["alone"] = {"launch_ms": round(alone["gemm_ms"], 4), "achieved": round(mult * ta, 2),
                                                  "frac": round(mult * ta / PEAK, 4)}
                if mult > 1:
                    line["roofline_mfma"]["alone"]["fp32_equivalent_frac"] = round(ta / 157.3, 4)
        if args.full and world == 1 and args.cpu_frames > 0:
            guard.phase("cpu_baseline (oracle on the host cores)", 1200)
            # torch's intra-op pool stops scaling (and then collapses) well below the box's core count on
            # these small ops: 16 threads measured fastest on the 256-core GPU host (8: 0.83, 16: 0.63,
            # 32: 0.75, 64: 1.09 s/frame encode); `cores` reports the threads actually used
            cores = min(os.cpu_count() or 1, 16)
            os.environ["OMP_NUM_THREADS"] = str(cores)
            v, enc_s, reg_s = cpu_baseline(min(args.cpu_frames, F), N, cores)
            line["cpu_baseline"] = {"value": round(v, 4), "unit": "frames/s", "cores": cores, "kind": "port",
                                    "sample": f"{min(args.cpu_frames, F)} frames x {N} pts: oracle encode {enc_s:.2f} s/frame "
                                              f"(C farthest-point sampling), register+information matrix {reg_s:.2f} s/frame"}
        # RCCL writes its version banner through C stdio (fully buffered on a pipe: it would surface at exit, AFTER this line);
        # flushed first, the JSON line is the last thing on stdout
        import ctypes
        ctypes.CDLL(None).fflush(None)
        gate_failed = args.full and line["parity_gate"].get("checked") and not line["parity_gate"]["ok"]
        if gate_failed:   # like Guard.fail: a run that did not reproduce the reference has no headline number
            line["value_measured_but_void"], line["value"] = line["value"], None
            line["error"] = "parity gate failed: the timed steps did not reproduce the reference's results (see parity_gate)"
        print(json.dumps(line), flush=True)
    else:
        gate_failed = False
    if world > 1 or forced:
        guard.phase("process-group teardown", args.collective_timeout)
        dist.destroy_process_group()
    if gate_failed:   # the line above already carries parity_gate.ok = false: no second line, a non-zero exit
        print("bench.py: PARITY GATE FAILED -- the timed steps did not reproduce the reference's results: " +
              json.dumps(line["parity_gate"]), file=sys.stderr, flush=True)
        guard.finish()
        sys.exit(1)


if __name__ == "__main__":
    main()
