#!/usr/bin/env python3
"""Replays a rosbag2 recording (or a synthetic stream) through the reference's frame loop with the MI355X
path doing the per-frame work, writes the trajectory in TUM format and prints the reference's stage timers.

usage: python tools/replay.py --bag run_0.db3 [--imu-topic /alphasense/imu] [--lidar-topic /hesai/pandar]
       python tools/replay.py --synthetic 20 --points 60000          (GPU box; no recording needed)
options: --out traj.tum   --device-map (keep the voxel grid on the GPU only)   --write-bag file.db3
         --resident (the scan never leaves the GPU between the raw sweep and the pose)
         --raw-points-on-device (with --resident: the map keeps its raw points, VGICP_OPTION_MAP_RAW_POINTS; their
         export is timed at the end)
         --robust-kernel none|huber|cauchy  --robust-scale C  --gate G (robust rounds, include/vgicp_hip_robust.h: in the
         library's regularised units, ~0.1; off by default)
         --robust-scale-quantile Q (registration.robust_scale_quantile: before each frame's align the scan is reported at
         the predicted pose, include/vgicp_hip_points.h, and the scale becomes sqrt(quantile Q of d^2); off by default)
         --insert-gate G (local_map.insert_gate, with --resident: points that are matched at the frame's
         pose and fail max(d^2, 0) <= G are kept out of the map, include/vgicp_hip_map_gated.h; off by default)
         --carve-range R [--carve-margin M --carve-min-hits H --carve-stride S] (local_map.carve, with --resident: before
         every map update the voxels that at least H of the scan's rays cross within R metres, stopping M metres short of
         their returns, and that hold no return of the scan, are removed, include/vgicp_hip_map_carve.h; off by default)
         --ray-report RANGE [--ray-margin M --ray-beyond B --ray-stride S] (with --resident: the read-only ray report of
         every frame's scan at its aligned pose, before the map update, include/vgicp_hip_map_rays.h: the first map voxel
         on every ray within RANGE metres and B metres behind the return; the class totals of the run are printed)
         --levels 3,2,1,0 [--coarse-max-iteration N --coarse-translation-sq-threshold T --coarse-cosine-threshold C]
         (registration.coarse_to_fine, with --resident: every frame's align runs in stages against the map's coarser
         levels, include/vgicp_hip_map_levels.h, every stage but the last with the coarse thresholds; off by default)
         --prior-update (kalman_filter.update.iterated: the filter's pose covariance enters every round of the align as a
         prior, include/vgicp_hip_prior.h, and the update is the iterated one; off by default)
The configuration is the reference's config/hilti_config.yaml as a dict (eskf_lio_amd/replay.py:DEFAULT_CONFIG);
--config file.yaml overrides it with a file of the reference's own layout."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from eskf_lio_amd import capi, replay, synth  # noqa: E402


def config_from_yaml(path):
    import yaml
    y = yaml.safe_load(open(path))
    imu = y["sensors"]["imu"]
    par = imu["intrinsics"]["parameters"]
    cfg = {k: (dict(v) if isinstance(v, dict) else v) for k, v in replay.DEFAULT_CONFIG.items()}
    cfg["imu"] = dict(update_rate=imu["update_rate"], bias_a=par["bias_a"], bias_g=par["bias_g"], gravity=par["gravity"],
                      accel_noise_density=par["accel_noise_density"], accel_zero_g_offset=par["accel_zero_g_offset"],
                      gyro_noise_density=par["gyro_noise_density"], gyro_zero_rate_offset=par["gyro_zero_rate_offset"])
    ext = y["sensors"]["lidar"]["extrinsics"]
    T = np.eye(4)
    T[:3, :3] = replay.quat_to_matrix(np.array(ext["quaternion"], dtype=np.float64))   # Eigen::Map: x y z w
    T[:3, 3] = ext["translation"]
    cfg["lidar_extrinsic"] = T
    cfg["kalman_filter"] = dict(y["kalman_filter"]["update"])
    lm = y["local_map"]
    cfg["local_map"] = dict(voxel_size=lm["voxel_size"], max_num_points_per_voxel=lm["max_num_points_per_voxel"],
                            translation_sq_threshold=lm["update"]["translation_sq_threshold"],
                            cosine_threshold=lm["update"]["cosine_threshold"],
                            remove_distant_points=lm["remove_distant_points"]["enabled"],
                            distance_threshold=lm["remove_distant_points"]["distance_threshold"],
                            removing_period=lm["remove_distant_points"]["removing_period"])
    cfg["cloud_preprocessor"] = dict(voxel_size=y["cloud_preprocessor"]["voxel_size"])
    cfg["registration"] = dict(y["registration"])
    return cfg, imu["topic_name"], y["sensors"]["lidar"]["topic_name"]


def carve_config(cfg, args):
    """The configuration with local_map.carve from the --carve-* flags (the same object when none is given)."""
    given = {k: v for k, v in (("max_range", args.carve_range), ("margin", args.carve_margin), ("min_hits", args.carve_min_hits),
                               ("stride", args.carve_stride)) if v is not None}
    if not given:
        return cfg
    if "max_range" not in given:
        raise ValueError("--carve-margin, --carve-min-hits and --carve-stride need --carve-range")
    return dict(cfg, local_map=dict(cfg["local_map"], carve=given))


def coarse_to_fine_config(cfg, args):
    """The configuration with registration.coarse_to_fine from --levels / --coarse-* (the same object when none is given)."""
    coarse = {k: v for k, v in (("max_iteration", args.coarse_max_iteration),
                                ("translation_sq_threshold", args.coarse_translation_sq_threshold),
                                ("cosine_threshold", args.coarse_cosine_threshold)) if v is not None}
    if args.levels is None:
        if coarse:
            raise ValueError("--coarse-* needs --levels")
        return cfg
    levels = [int(l) for l in args.levels.split(",")]
    ctf = dict(levels=levels, coarse=coarse) if coarse else dict(levels=levels)
    return dict(cfg, registration=dict(cfg["registration"], coarse_to_fine=ctf))


def ray_report_params(args):
    """What DeviceBackend.set_ray_report takes, from the --ray-* flags; None without --ray-report."""
    if args.ray_report is None:
        return None
    return dict(max_range=args.ray_report, margin=args.ray_margin or 0.0, beyond=args.ray_beyond or 0.0,
                stride=args.ray_stride or 1)


def ray_report_line(totals, params):
    names = capi.RAY_CLASS_NAMES
    classes = ", ".join(f"{names[c]} {totals['by_class'][c]}" for c in range(len(names)))
    return (f"ray report within {params['max_range']} m (margin {params['margin']}, beyond {params['beyond']}, stride "
            f"{params['stride']}) at {totals['frames']} aligned poses: {totals['rays']} rays, {totals['visits']} voxels visited; "
            f"{classes}")


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--bag")
    ap.add_argument("--synthetic", type=int, default=0, help="number of synthetic LiDAR frames")
    ap.add_argument("--points", type=int, default=20_000, help="points per synthetic frame")
    ap.add_argument("--config")
    ap.add_argument("--imu-topic", default=None)
    ap.add_argument("--lidar-topic", default=None)
    ap.add_argument("--out", default="trajectory.tum")
    ap.add_argument("--write-bag", default=None, help="also store the synthetic stream as a rosbag2 file")
    ap.add_argument("--device-map", action="store_true")
    ap.add_argument("--resident", action="store_true",
                    help="scan stays on the GPU from the raw sweep to the pose (vgicp_scan_prepare chain)")
    ap.add_argument("--raw-points-on-device", action="store_true",
                    help="with --resident: the device map keeps every voxel's raw points (VGICP_OPTION_MAP_RAW_POINTS)")
    ap.add_argument("--robust-kernel", choices=("none", "huber", "cauchy"), default=None,
                    help="robust weight of every registration round (registration.robust_kernel)")
    ap.add_argument("--robust-scale", type=float, default=None, help="its scale c (registration.robust_scale)")
    ap.add_argument("--gate", type=float, default=None,
                    help="gate on the squared Mahalanobis residual, 0 = none (registration.gate)")
    ap.add_argument("--robust-scale-quantile", type=float, default=None,
                    help="the scale follows this quantile of d^2 at each frame's predicted pose "
                         "(registration.robust_scale_quantile)")
    ap.add_argument("--insert-gate", type=float, default=None,
                    help="gate of the map insertion on d^2 at the frame's pose, 0 = none (local_map.insert_gate)")
    ap.add_argument("--prior-update", action="store_true",
                    help="the iterated filter update with the pose prior in every align (kalman_filter.update.iterated)")
    ap.add_argument("--carve-range", type=float, default=None,
                    help="free-space carving before every map update: metres a ray is followed (local_map.carve.max_range)")
    ap.add_argument("--carve-margin", type=float, default=None, help="metres a ray stops short of its return (local_map.carve.margin)")
    ap.add_argument("--carve-min-hits", type=int, default=None, help="rays that must cross a voxel (local_map.carve.min_hits)")
    ap.add_argument("--carve-stride", type=int, default=None, help="every S-th point casts a ray (local_map.carve.stride)")
    ap.add_argument("--levels", default=None, metavar="L,L,..",
                    help="the level of every stage of each frame's align, e.g. 3,2,1,0 (registration.coarse_to_fine.levels)")
    ap.add_argument("--coarse-max-iteration", type=int, default=None,
                    help="rounds of every stage but the last (registration.coarse_to_fine.coarse.max_iteration, default 30)")
    ap.add_argument("--coarse-translation-sq-threshold", type=float, default=None,
                    help="... its translation threshold (registration.coarse_to_fine.coarse.translation_sq_threshold, default 1e-4)")
    ap.add_argument("--coarse-cosine-threshold", type=float, default=None,
                    help="... its rotation threshold (registration.coarse_to_fine.coarse.cosine_threshold, default 0.999)")
    ap.add_argument("--ray-report", type=float, default=None, metavar="RANGE",
                    help="the ray report at every aligned pose before the map update: metres a ray is followed (vgicp_hip_map_rays.h)")
    ap.add_argument("--ray-margin", type=float, default=None, help="metres in front of a return within which a hit is near, not blocked")
    ap.add_argument("--ray-beyond", type=float, default=None, help="metres a ray is followed behind its return")
    ap.add_argument("--ray-stride", type=int, default=None, help="every S-th point casts a ray")
    args = ap.parse_args(argv)
    if any(v is not None for v in (args.ray_report, args.ray_margin, args.ray_beyond, args.ray_stride)):
        if not args.resident:
            ap.error("--ray-* needs --resident")
        if args.ray_report is None:
            ap.error("--ray-margin, --ray-beyond and --ray-stride need --ray-report")
    if args.raw_points_on_device and not args.resident:
        ap.error("--raw-points-on-device needs --resident")
    if any(v is not None for v in (args.carve_range, args.carve_margin, args.carve_min_hits, args.carve_stride)):
        if not args.resident:
            ap.error("--carve-* needs --resident")
        if args.carve_range is None:
            ap.error("--carve-margin, --carve-min-hits and --carve-stride need --carve-range")
    if any(v is not None for v in (args.levels, args.coarse_max_iteration, args.coarse_translation_sq_threshold,
                                   args.coarse_cosine_threshold)):
        if not args.resident:
            ap.error("--levels and --coarse-* need --resident")
        if args.levels is None:
            ap.error("--coarse-* needs --levels")
    args.parser = ap
    return args


def main(argv=None):
    """Runs the replay; returns its summary: poses, and with --ray-report the class totals of the run (ray_report)."""
    args = parse_args(argv)
    ap = args.parser
    cfg, imu_topic, lidar_topic = replay.DEFAULT_CONFIG, replay.IMU_TOPIC, replay.LIDAR_TOPIC
    if args.config:
        cfg, imu_topic, lidar_topic = config_from_yaml(args.config)
    imu_topic, lidar_topic = args.imu_topic or imu_topic, args.lidar_topic or lidar_topic
    robust = {k: v for k, v in (("robust_kernel", args.robust_kernel), ("robust_scale", args.robust_scale),
                                ("gate", args.gate), ("robust_scale_quantile", args.robust_scale_quantile))
              if v is not None}
    if robust:
        cfg = dict(cfg, registration=dict(cfg["registration"], **robust))
    if args.insert_gate is not None:
        if not args.resident:
            ap.error("--insert-gate needs --resident")
        cfg = dict(cfg, local_map=dict(cfg["local_map"], insert_gate=args.insert_gate))
    if args.prior_update:
        cfg = dict(cfg, kalman_filter=dict(cfg["kalman_filter"], iterated=True))
    cfg = carve_config(cfg, args)
    cfg = coarse_to_fine_config(cfg, args)
    truth = None
    if args.bag:
        events = replay.read_rosbag2(args.bag, imu_topic, lidar_topic)
    elif args.synthetic > 0:
        raw, truth = synth.make_sensor_stream(frames=args.synthetic, points_per_frame=args.points,
                                              world_points=max(3 * args.points, 60_000))
        events = [(a, replay.ImuMeasurement(e[1], e[2], e[3]) if e[0] == "imu" else replay.LidarMeasurement(e[1], e[2]))
                  for a, e in raw]
        if args.write_bag:
            replay.write_rosbag2(args.write_bag, events, imu_topic, lidar_topic)
    else:
        ap.error("one of --bag / --synthetic is required")
    backend = replay.DeviceBackend(cfg) if args.resident else replay.GpuBackend(cfg, device_resident_map=args.device_map)
    if args.raw_points_on_device:
        backend.ctx.set_option(capi.OPTION_MAP_RAW_POINTS, 1)   # the map is empty here, as the option wants
    ray_params = ray_report_params(args)
    if ray_params is not None:
        backend.set_ray_report(**ray_params)
    odo = replay.Odometry(cfg, backend)
    traj = odo.run(events)
    summary = dict(poses=len(traj), ray_report=None, trajectory=traj)
    replay.write_tum(args.out, traj)
    print(f"{len(traj)} poses -> {args.out}; Gauss-Newton rounds per frame: {odo.backend.iterations}")
    print(odo.report())
    if backend.scales:
        cs = [c for _, c in backend.scales]
        print(f"robust scale from the {args.robust_scale_quantile} quantile of d^2 at each predicted pose: "
              f"min {min(cs):.4f}, median {float(np.median(cs)):.4f}, max {max(cs):.4f}")
    if args.levels is not None:
        print(f"align in stages against levels {args.levels}: rounds per stage and frame {backend.stage_iterations}; "
              f"voxels per level {backend.ctx.map_levels_build(max(cfg['registration']['coarse_to_fine']['levels'])).voxels}")
    if args.insert_gate:
        points, refused = backend.ctx.map_gated_totals()
        print(f"map insertion gated at d^2 <= {args.insert_gate}: {refused} of {points} points kept out of the map")
    if args.carve_range is not None:
        rays, removed = backend.ctx.map_carve_totals()
        print(f"free-space carving within {args.carve_range} m: {removed} voxels removed by {rays} rays")
    if ray_params is not None:
        summary["ray_report"] = dict(backend.ray_totals, classes=dict(zip(capi.RAY_CLASS_NAMES, backend.ray_totals["by_class"])))
        print(ray_report_line(backend.ray_totals, ray_params))
    if args.raw_points_on_device:
        t0 = time.perf_counter()
        keys, _ = backend.ctx.map_points_export()
        print(f"raw points kept on the device: {len(keys)} in {backend.ctx.map_size()[0]} voxels; "
              f"map_points_export (size query + export) {1e3 * (time.perf_counter() - t0):.2f} ms")
    if truth is not None:
        err = [np.linalg.norm(T[:3, 3] - G[:3, 3]) for (_, T), (_, G) in zip(traj, truth)]
        print(f"synthetic stream: position error against the generating motion, max {max(err):.4f} m")
    return summary


if __name__ == "__main__":
    main()
