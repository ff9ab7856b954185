"""Geometric loop closure (deeppointmap_amd/loop_closure.py) over two laps of a simulated circuit, with poses from two sources:
  drift     the exact poses with a yaw-rate drift injected into every step
  odometry  odometry.LidarOdometry on the same frames (GeometricSlam)
For each: the candidates the Scan Context search proposed, the accepted edges, the wrong ones among them (the two frames
further apart in truth than max_offset, or the edge more than --wrong-t metres / --wrong-r radians from the true relative
pose) and the ATE against the exact poses before and after the optimisation.  `--survey` also verifies EVERY candidate the
search returns, with all gates open, and tabulates distance, true separation, fitness and pose error: the table the
defaults of max_distance, min_fitness, max_offset and max_yaw_change were read from.  Last, GeometricSlam with and without
rewrite_map (the local map rebuilt from the stored frames after a correction) over two laps of circuit(radius=30).  A report,
not a target: nothing is asserted.

  python scripts/sim_loop_closure_eval.py [--spacing 4.0] [--beams 16] [--columns 256] [--sigma 0.0] [--drift 0.002] [--survey]
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

DEV = "cuda"


def drifted(poses, bias):
    """the exact poses with Rz(bias) appended to every step: an odometry whose yaw rate is off"""
    c, s = np.cos(bias), np.sin(bias)
    B = np.eye(4)
    B[:2, :2] = [[c, -s], [s, c]]
    out = [poses[0].copy()]
    for k in range(1, len(poses)):
        out.append(out[-1] @ (np.linalg.inv(poses[k - 1]) @ poses[k]) @ B)
    return np.stack(out)


def edge_errors(edges, truth):
    """[(true separation m, translation error m, rotation error rad)] of edges (source, target, pose) against the exact poses"""
    from deeppointmap_amd import evaluate
    out = []
    for e in edges:
        X = np.linalg.inv(truth[e.target]) @ truth[e.source]
        D = np.linalg.inv(X) @ e.pose
        out.append((float(np.linalg.norm(X[:3, 3])), float(np.linalg.norm(D[:3, 3])), float(evaluate.rotation_angle(D[:3, :3]))))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--spacing", type=float, default=4.0)
    ap.add_argument("--beams", type=int, default=16)
    ap.add_argument("--columns", type=int, default=256)
    ap.add_argument("--sigma", type=float, default=0.0)
    ap.add_argument("--drift", type=float, default=0.002)
    ap.add_argument("--blocks", type=int, default=1)
    ap.add_argument("--wrong-t", type=float, default=0.5)
    ap.add_argument("--wrong-r", type=float, default=0.05)
    ap.add_argument("--survey", action="store_true")
    ap.add_argument("--rewrite-spacing", type=float, default=1.0, help="spacing of the rewrite_map comparison's circuit")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sim_loop_closure_eval.md"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("sim_loop_closure_eval.py runs on a GPU; none is visible")
    from deeppointmap_amd import augment, evaluate, lidar_sim as LS
    from deeppointmap_amd.loop_closure import GeometricSlam, LoopCloser, close_loops
    scene = LS.street_scene(2, blocks=(a.blocks, a.blocks))
    model = LS.LidarModel(np.linspace(10.0, -20.0, a.beams), a.columns, 0.9, 80.0, range_sigma=a.sigma)
    truth = LS.circuit(scene, spacing=a.spacing, laps=2)
    F = len(truth)
    rng = torch.Generator(device=DEV)
    rng.manual_seed(1)
    sim = LS.LidarSimulator(scene, model, rng=rng if a.sigma > 0 else None, device=DEV)
    frames = sim.frames(truth)
    loop_kw = dict(capacity=F, points_per_frame=model.rays, sc=dict(max_range=model.max_range, z_offset=LS.SENSOR_HEIGHT))
    defaults = LoopCloser(**loop_kw)
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    def report(name, before, after, closer, seconds, syncs):
        errs = edge_errors(closer.loops, truth)
        wrong = sum(sep > closer.max_offset or t > a.wrong_t or r > a.wrong_r for sep, t, r in errs)
        b, c = evaluate.ate(before, truth), evaluate.ate(after, truth)
        say(f"| {name} | {len(closer.candidates)} | {len(closer.loops)} | {wrong} | {b['rmse']:.3f} | {b['max']:.3f} | {c['rmse']:.3f} | "
            f"{c['max']:.3f} | {max([t for _, t, _ in errs], default=0):.3f} | {max([r for _, _, r in errs], default=0):.4f} | "
            f"{seconds / F * 1e3:.1f} | {syncs / F:.2f} |")

    say("# Geometric loop closure on two laps of a simulated circuit\n")
    say(f"`python scripts/sim_loop_closure_eval.py --spacing {a.spacing} --beams {a.beams} --columns {a.columns} --sigma {a.sigma} "
        f"--drift {a.drift} --blocks {a.blocks}{' --survey' if a.survey else ''}` on {torch.cuda.get_device_name(0)}: "
        f"lidar_sim.street_scene(2, blocks=({a.blocks}, {a.blocks})), {F} poses of circuit(spacing={a.spacing}, laps=2), {a.beams} beams x "
        f"{a.columns} columns, range noise {a.sigma} m.  LoopCloser with its defaults (max_distance {defaults.max_distance}, min_fitness "
        f"{defaults.min_fitness}, max_offset {defaults.max_offset} m, max_yaw_change {defaults.max_yaw_change} rad, exclude_recent "
        f"{defaults.exclude_recent}, k {defaults.k}, sample {defaults.sample} m, metric {defaults.metric}) except capacity, "
        f"points_per_frame = {model.rays} and the descriptor's max_range {model.max_range} m, z_offset {LS.SENSOR_HEIGHT} m.  wrong: the frames "
        f"further apart in truth than max_offset, or the edge more than {a.wrong_t} m / {a.wrong_r} rad from the true relative pose.  "
        "A report, not a target.\n")
    say("| poses from | candidates verified | accepted edges | wrong edges | ATE rmse before m | ATE max before m | ATE rmse after m | "
        "ATE max after m | worst edge error m | worst edge error rad | ms per frame | host syncs per frame |")
    say("|---|---|---|---|---|---|---|---|---|---|---|---|")

    # (a) exact poses with an injected yaw-rate drift, online
    given = drifted(truth, a.drift)
    lc = LoopCloser(**loop_kw)
    s0, t0 = augment.host_syncs(), time.perf_counter()
    for f, p in zip(frames, given):
        lc.add(f, p)
    after = lc.optimise()
    report(f"exact + {a.drift} rad yaw drift a step, online", given, after, lc, time.perf_counter() - t0, augment.host_syncs() - s0)
    online_edges = [(e.source, e.target) for e in lc.loops]

    # the same, offline
    s0, t0 = augment.host_syncs(), time.perf_counter()
    after_off, edges_off, off = close_loops(frames, given, return_closer=True, **loop_kw)
    report("the same, close_loops", given, after_off, off, time.perf_counter() - t0, augment.host_syncs() - s0)
    same = online_edges == [(e.source, e.target) for e in edges_off]

    # (b) the odometry
    slam = GeometricSlam(odometry=dict(max_range=model.max_range, first_pose=truth[0], initial_motion=LS.sweep_delta(truth[0], truth[1]),
                                       sample_map=0.25, sample_register=0.75, metric="plane", voxel_size=1.0),
                         loop=loop_kw)
    s0, t0 = augment.host_syncs(), time.perf_counter()
    for f in frames:
        slam.step(f)
    raw = np.stack(slam.odometry.poses)
    if np.isfinite(raw).all():
        report("LidarOdometry (GeometricSlam)", raw, slam.poses, slam.loop_closer, time.perf_counter() - t0, augment.host_syncs() - s0)
        bad = sum(s.status not in (0, 1) for s in slam.odometry.steps)
        say(f"\nLidarOdometry: {bad} of {F} steps failed to register; its position error at every tenth frame "
            f"{[round(float(np.linalg.norm(raw[k][:3, 3] - truth[k][:3, 3])), 2) for k in range(0, F, 10)]} m.")
    else:
        say("\nLidarOdometry: poses not finite, no row.")
    say(f"\nOnline and offline accepted the same edges: {same}.")

    # recall: frames of lap 2 whose nearest lap-1 frame (in truth) lies within max_offset, and how many of them got an edge
    per_lap = F // 2
    have = {e.source for e in lc.loops}
    could = [i for i in range(per_lap, F) if i - lc.exclude_recent > 0 and
             np.linalg.norm(truth[:i - lc.exclude_recent, :3, 3] - truth[i, :3, 3], axis=1).min() <= lc.max_offset]
    say(f"Drift run: {len(could)} frames have an earlier frame (older than exclude_recent) within max_offset in truth; "
        f"{len(have & set(could))} of them got at least one edge (recall), {len(have - set(could))} frames got an edge without one.")

    # (c) the odometry with and without the local map rebuilt after a correction, over gentle corners
    truth_c = LS.circuit(scene, spacing=a.rewrite_spacing, laps=2, radius=30.0)
    frames_c = sim.frames(truth_c)
    Fc = len(truth_c)
    say(f"\n## GeometricSlam with and without rewrite_map: {Fc} poses of circuit(spacing={a.rewrite_spacing}, laps=2, radius=30)\n")
    say("The corners of 30 m keep the odometry away from the loss at 6 m corners noted above, which this comparison does not "
        "address.  With rewrite_map the local map is rebuilt from the loop closer's stored frames under the corrected poses after "
        "every accepted loop and the odometry rebased (rewrite_min_shift (0, 0)); `odometry ATE` is then over poses that changed "
        "frame at every rebase.  lap 2: the mean position error of the reported trajectory over the second lap.\n")
    say("| rewrite_map | accepted edges | rebases | steps that failed to register | odometry ATE rmse m | reported ATE rmse m | "
        "reported ATE max m | lap 2 mean error m | ms per frame | host syncs per frame |")
    say("|---|---|---|---|---|---|---|---|---|---|")
    along = []
    for rewrite in (False, True):
        slam = GeometricSlam(odometry=dict(max_range=model.max_range, first_pose=truth_c[0], initial_motion=LS.sweep_delta(truth_c[0], truth_c[1]),
                                           sample_map=0.25, sample_register=0.75, metric="plane", voxel_size=1.0),
                             loop=dict(loop_kw, capacity=Fc), rewrite_map=rewrite)
        s0, t0 = augment.host_syncs(), time.perf_counter()
        try:
            for f in frames_c:
                slam.step(f)
        except ValueError as e:
            say(f"| {rewrite} | stopped at frame {len(slam.odometry.poses)}: {e} | | | | | | | | |")
            continue
        seconds, syncs = time.perf_counter() - t0, augment.host_syncs() - s0
        raw, out = np.stack(slam.odometry.poses), slam.poses
        if not (np.isfinite(raw).all() and np.isfinite(out).all()):
            say(f"| {rewrite} | poses not finite | | | | | | | | |")
            continue
        bad = sum(st.status not in (0, 1) for st in slam.odometry.steps)
        r, c = evaluate.ate(raw, truth_c), evaluate.ate(out, truth_c)
        lap2 = float(np.linalg.norm(out[Fc // 2:, :3, 3] - truth_c[Fc // 2:, :3, 3], axis=1).mean())
        say(f"| {rewrite} | {len(slam.loops)} | {len(slam.odometry.rebases)} | {bad} | {r['rmse']:.3f} | {c['rmse']:.3f} | {c['max']:.3f} | "
            f"{lap2:.3f} | {seconds / Fc * 1e3:.1f} | {syncs / Fc:.2f} |")
        along.append(f"rewrite_map {rewrite}: position error of the reported trajectory at every 40th frame "
                     f"{[round(float(np.linalg.norm(out[k][:3, 3] - truth_c[k][:3, 3])), 2) for k in range(0, Fc, 40)]} m; steps that "
                     f"failed to register: {[k for k, st in enumerate(slam.odometry.steps) if st.status not in (0, 1)]}.")
    say("\n" + "\n".join(along))
    say("An error of metres before the first loop (frame " + str(Fc // 2) + " starts lap 2) means the odometry was lost on lap 1: neither "
        "form can then show what the rewrite is for, the loop edges cannot repair odometry edges wrong by metres.")

    if a.survey:
        wide = LoopCloser(max_distance=2.0, min_fitness=0.0, max_offset=1e9, max_yaw_change=4.0, **loop_kw)
        for f, p in zip(frames, given):
            wide.add(f, p)
        errs = edge_errors(wide.loops, truth)
        say("\n## Survey: every candidate the search returned, verified with all gates open\n")
        say("| source | target | SC distance | true separation m | fitness | rmse m | edge |t| m | yaw change rad | error m | error rad |")
        say("|---|---|---|---|---|---|---|---|---|---|")
        from deeppointmap_amd.loop_closure import _rz, yaw_between
        for e, (sep, t, r) in zip(wide.loops, errs):
            dyaw = float(yaw_between(_rz(wide.sc.yaw(e.shift))[None], e.pose[None])[0])
            say(f"| {e.source} | {e.target} | {e.distance:.4f} | {sep:.2f} | {e.fitness:.3f} | {e.rmse:.3f} | "
                f"{np.linalg.norm(e.pose[:3, 3]):.2f} | {dyaw:+.3f} | {t:.3f} | {r:.4f} |")
        say(f"\n{len(wide.candidates)} candidates, {len(wide.loops)} of them with a finite registration.")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
