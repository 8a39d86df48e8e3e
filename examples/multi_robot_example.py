#!/usr/bin/env python3
"""Multi-robot pose graph optimization example on one MI355X -- the counterpart of the reference's
examples/MultiRobotExample.cpp: contiguous partition into N robots (:71-119), greedy block selection with Nesterov
acceleration (:170-255), one line per iteration in the reference's format, then the rounded trajectory of every robot in
the frame of robot 0's first pose (the global anchor, :249-254) is written as CSV (PGOLogger::logTrajectory format).

  python examples/multi_robot_example.py 5 data/smallGrid3D.g2o [--out-dir /tmp/traj] [--no-acceleration]

--robust-cost {L1,Huber,TLS,GM,GNC_TLS} runs the reference's robust agent protocol instead (coloured schedule, weight
updates by PGOAgent::shouldUpdateMeasurementWeights, dpgo_amd.robust.DistributedRobustPGO) and prints the global robust
cost of every weight update.

--staircase runs the distributed Riemannian staircase instead (dpgo_amd.solveCertifiedDistributedPGO, from rank d: RBCD
sweeps, the team's certificate, escape to the next rank while the iterate is a saddle); --iterations bounds the sweeps per
rank; one line per escape, the verdict on the last line.

--local-frames starts distributed: no centralised initialisation, every robot initialises in its own frame (odometry, or
--local-init chordal) and joins robot 0's frame by robust frame alignment on the device, printing the reference's
"Robot a attempts initialization from neighbor b: finds i/m inliers." for every attempt.
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def local_frame_agents(args, meas, n, r):
    """--local-frames: what the reference's agents do without a central initialisation.  Every robot computes a trajectory
    from its OWN measurements in its own frame (PGOAgent::initialize, src/PGOAgent.cpp:219-289: odometry by default, or
    chordal), robot 0's frame is the global one, and the others join it through their loop closures with an initialised
    neighbour (computeRobustNeighborTransformTwoStage + initializeInGlobalFrame, :550-602, :308-352) -- on the device."""
    import dpgo_amd
    from dpgo_amd.agent import DeviceAgent, ExchangePlan, RBCDCluster, build_pose_graphs
    from dpgo_amd.initialization import chordal_initialization, odometry_initialization
    ranges, graphs = build_pose_graphs(meas, n, args.num_robots, r)
    plan = ExchangePlan(graphs)
    agents = {}
    for a, pg in enumerate(graphs):
        m = pg.measurements()
        own = m.select((m.r1 == a) & (m.r2 == a))
        if args.local_init == "chordal":
            T_local = chordal_initialization(own, pg.n())
        else:
            T_local = odometry_initialization(own.select(own.p1 + 1 == own.p2), pg.n())
        agents[a] = DeviceAgent.from_local_frame(graphs, plan, a, T_local, params=dpgo_amd.ROptParameters())
    records, waiting = RBCDCluster(plan, agents).initialize_in_global_frame(on_attempt=lambda rec: print(
        "Robot %d attempts initialization from neighbor %d: finds %d/%d inliers." % (
            rec.agent, rec.neighbour, rec.inliers, rec.candidates)))  # (src/PGOAgent.cpp:583-584)
    if waiting:
        raise SystemExit("Robots %s found no neighbour to initialise from." % waiting)
    return agents, graphs, plan


def staircase(args, meas, n):
    """--staircase: the team's Riemannian staircase from rank d; one line per escape, the final verdict last."""
    import numpy as np
    import dpgo_amd
    from dpgo_amd.trajectory import log_trajectory
    d = meas.d
    if args.robust_cost or args.local_frames:
        raise SystemExit("--staircase takes neither --robust-cost nor --local-frames.")
    print("Running the distributed staircase from rank %d..." % d)
    res = dpgo_amd.solveCertifiedDistributedPGO(meas, n, args.num_robots, max_sweeps=args.iterations)
    for e in res.escapes:
        print("Escape | rank = %d -> %d | lambda_min = %.6g | alpha = %.4g | cost = %.6g -> %.6g | sweeps = %d" % (
            e["rank"], e["rank"] + 1, e["lambda_min"], e["alpha"], 2 * e["f_before"], 2 * e["f_after"], e["sweeps"]))
    if args.out_dir:
        os.makedirs(args.out_dir, exist_ok=True)
        path = os.path.join(args.out_dir, "team.csv")
        if log_trajectory(d, n, np.asfortranarray(res.trajectory), path):
            print("wrote %s" % path)
    c = res.certificate
    print("Certificate of the team's iterate: %s | rank = %d | lambda_min = %s | cost = %.6g | rounded cost = %.6g | "
          "sweeps per rank = %s" % (res.status, res.rank, "%.6g" % c.lambda_min if c is not None else "n/a", 2 * res.f,
                                    2 * res.f_rounded, res.sweeps))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("num_robots", type=int)
    ap.add_argument("g2o")
    ap.add_argument("--rank", type=int, default=5)
    ap.add_argument("--iterations", type=int, default=1000)
    ap.add_argument("--no-acceleration", action="store_true")
    ap.add_argument("--out-dir", default=None)
    ap.add_argument("--certify", action="store_true",
                    help="certify the assembled global iterate on one central handle (QuadraticProblem.certify)")
    ap.add_argument("--certify-team", action="store_true",
                    help="certify the team's iterate from the agents' own blocks on the device (RBCDCluster.certify)")
    ap.add_argument("--staircase", action="store_true",
                    help="distributed Riemannian staircase from rank d (dpgo_amd.solveCertifiedDistributedPGO): RBCD sweeps, "
                         "the team's certificate (implies --certify-team), escape to the next rank while it is a saddle")
    ap.add_argument("--robust-cost", choices=["L1", "Huber", "TLS", "GM", "GNC_TLS"], default=None,
                    help="robust agent protocol with this cost: weights re-computed on the device between blocks of iterations")
    ap.add_argument("--weight-updates", type=int, default=10, help="robustOptNumWeightUpdates")
    ap.add_argument("--inner-iterations", type=int, default=30, help="robustOptInnerIters")
    ap.add_argument("--local-frames", action="store_true",
                    help="every robot initialises from its own measurements, in its own frame, and joins the global frame "
                         "through robust frame alignment with its neighbours (no centralised initialisation)")
    ap.add_argument("--local-init", choices=["odometry", "chordal"], default="odometry",
                    help="localInitializationMethod of --local-frames (include/DPGO/PGOAgent.h:134)")
    args = ap.parse_args()
    print("Multi-robot pose graph optimization example. ")
    if args.num_robots <= 0:
        raise SystemExit("Number of robots must be positive!")
    print("Simulating %d robots." % args.num_robots)
    import numpy as np
    import dpgo_amd
    from dpgo_amd.agent import DeviceAgent, ExchangePlan, RBCDCluster, build_pose_graphs
    from dpgo_amd.initialization import chordal_initialization
    from dpgo_amd.synthetic import lift_tiles
    from dpgo_amd.trajectory import log_trajectory

    meas, n = dpgo_amd.read_g2o_file(args.g2o)
    print("Loaded dataset from file %s." % args.g2o)
    r, d = args.rank, meas.d
    if args.staircase:
        return staircase(args, meas, n)
    if args.local_frames:
        agents, graphs, plan = local_frame_agents(args, meas, n, r)
    else:
        X0 = lift_tiles(chordal_initialization(meas, n), r)  # PGOAgent's default: chordal initialisation
        ranges, graphs = build_pose_graphs(meas, n, args.num_robots, r)
        plan = ExchangePlan(graphs)
        agents = {a: DeviceAgent(graphs, plan, a, X0[ranges[a][0]:ranges[a][1]], dpgo_amd.ROptParameters())
                  for a in range(args.num_robots)}
    if args.robust_cost:
        from dpgo_amd.agent import PGOAgentParameters
        from dpgo_amd.robust import DistributedRobustPGO, RobustCostParameters
        cluster = RBCDCluster(plan, agents)
        driver = DistributedRobustPGO(cluster, RobustCostParameters(args.robust_cost),
                                      PGOAgentParameters(robustOptNumWeightUpdates=args.weight_updates,
                                                         robustOptInnerIters=args.inner_iterations,
                                                         maxNumIters=args.iterations))
        print("Running the robust protocol (%s), at most %d iterations..." % (args.robust_cost, args.iterations))
        info = driver.run(on_update=lambda h: print(
            "Weight update | mu = %.4g | inliers = %d | outliers = %d | undecided = %d | skipped = %d | robust cost = %.6g" % (
                h["mu"], h["inliers"], h["outliers"], h["undecided"], h["skipped"], h["cost"])))
        print("Terminated after %d iterations, %d weight updates (inner iterations %s) | robust cost = %.6g | "
              "weighted cost = %.6g | gradnorm = %.5g" % (info["iterations"], info["updates"], info["inner_iterations"],
                                                          info["robust_cost"], info["cost"], info["gradnorm"]))
    else:
        if not args.no_acceleration:
            for ag in agents.values():
                ag.enable_acceleration(args.num_robots)
        cluster = RBCDCluster(plan, agents)
        print("Running %d iterations..." % args.iterations)
        out = cluster.run_greedy(max_iters=args.iterations, gradnorm_stop=0.1)
        for it, (rob, (cost, gn)) in enumerate(zip(out["selected"], out["trace"])):
            print("Iter = %d | robot = %d | cost = %.5g | gradnorm = %.5g" % (it, rob, cost, gn))
    if args.certify:
        X = np.concatenate([agents[a].X.cpu().numpy() for a in range(args.num_robots)])  # tiles [n, d+1, r]
        pg = dpgo_amd.PoseGraph(0, r, d)
        pg.setMeasurements(meas)
        central = dpgo_amd.QuadraticProblem(pg)
        c = central.certify(np.ascontiguousarray(X).reshape(-1, r).T)
        print("Certificate of the global iterate: %s | lambda_min = %.6g | |rgrad| = %.3g | %d LOBPCG iterations" % (
            c.status, c.lambda_min, c.gradnorm, c.iterations))
    if args.certify_team:
        c = cluster.certify()
        print("Certificate of the team's iterate: %s | lambda_min = %.6g | |rgrad| = %.3g | %d LOBPCG iterations | "
              "symmetry defect = %.2g" % (c.status, c.lambda_min, c.gradnorm, c.iterations, c.symmetry_defect))
    if args.out_dir:
        os.makedirs(args.out_dir, exist_ok=True)
        for a, T in cluster.trajectories_in_global_frame().items():
            Tm = np.ascontiguousarray(T.cpu().numpy()).reshape(-1, d).T  # tiles [n, d+1, d] -> d x (d+1)n
            if log_trajectory(d, graphs[a].n(), np.asfortranarray(Tm), os.path.join(args.out_dir, "robot%d.csv" % a)):
                print("wrote %s" % os.path.join(args.out_dir, "robot%d.csv" % a))


if __name__ == "__main__":
    main()
