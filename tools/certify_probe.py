"""Certificate probe: one JSON line per (case, preconditioner) with the time, LOBPCG iterations, products with C and
lambda_min of dpgo_problem_certify.

    python tools/certify_probe.py [--cases sphere2500,torus3D,kitti_00,grid100k] [--max-iterations 2000]

sphere2500 / torus3D / kitti_00 (one agent): solved with the multilevel RTR to |rgrad| <= 1e-6 from the chordal
initialisation, then certified.  grid100k: the benchmark's 100k-pose grid (bench.py make_workload) after its 5 settling
local solves -- not a critical point, so its certificate answers for a non-stationary iterate.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="sphere2500,torus3D,kitti_00,grid100k")
    ap.add_argument("--preconds", default="none,jacobi,multilevel")
    ap.add_argument("--max-iterations", type=int, default=2000)
    ap.add_argument("--tol-rel", type=float, default=1e-7)
    args = ap.parse_args()
    import numpy as np
    import dpgo_amd
    from dpgo_amd import synthetic
    from dpgo_amd.initialization import chordal_initialization

    r = 5
    for case in args.cases.split(","):
        if case == "grid100k":
            meas, n, Ttrue = synthetic.synthetic_grid(50, 50, 40, seed=0)
            X0 = synthetic.lift_tiles(synthetic.perturbed_truth(Ttrue, seed=2), r)
            prm, solves = dpgo_amd.ROptParameters(precond="multilevel"), 5
        else:
            meas, n = dpgo_amd.read_g2o_file(os.path.join(ROOT, "data", case + ".g2o"))
            X0 = synthetic.lift_tiles(chordal_initialization(meas, n), r)
            prm = dpgo_amd.ROptParameters(precond="multilevel", gradnorm_tol=1e-6, RTR_iterations=100,
                                          RTR_tCG_iterations=500, time_bound_s=120.0)
            solves = 20
        d = meas.d
        pg = dpgo_amd.PoseGraph(0, r, d)
        pg.setMeasurements(meas)
        prob = dpgo_amd.QuadraticProblem(pg)
        opt = dpgo_amd.QuadraticOptimizer(prob, prm)
        X = np.ascontiguousarray(X0).reshape(-1, r).T
        for _ in range(solves):
            X = opt.optimize(X)
            if opt.getOptResult().gradNormOpt <= prm.gradnorm_tol and case != "grid100k":
                break
        for pc in args.preconds.split(","):
            prob.certify(X, precond=pc, tol_rel=args.tol_rel, max_iterations=5)  # warm-up (hierarchy, factors)
            c = prob.certify(X, precond=pc, tol_rel=args.tol_rel, max_iterations=args.max_iterations)
            print(json.dumps(dict(case=case, poses=n, precond=pc, status=c.status, lambda_min=c.lambda_min,
                                  residual=c.residual, gradnorm=c.gradnorm, iterations=c.iterations,
                                  products=c.products, deflated=c.deflated, ms=round(c.elapsedMs, 2))), flush=True)


if __name__ == "__main__":
    main()
