// QuadraticProblem::robustReweight of the C++ mirror (include/dpgo_hip.hpp): Huber re-weighting of a 3-pose triangle whose
// closing edge is an outlier.  The weights must be RobustCost::weight of the residuals the call returns.
// Exit 77 without a HIP device (no CPU fallback), 0 when every check holds.
#include <cmath>
#include <cstdio>

#include "dpgo_hip.hpp"

using namespace dpgo_hip;

int main() {
  int devices = 0;
  if (dpgo_device_count(&devices) != DPGO_OK || devices == 0) {
    std::printf("no HIP device\n");
    return 77;
  }
  const int n = 3, d = 3, r = 3, b = d + 1;
  Matrix I = Matrix::Identity(3, 3), step(3, 1), far(3, 1);
  step(0, 0) = 1.0;
  far(0, 0) = 2.0, far(1, 0) = 7.0;  // truth: (2, 0, 0) -- the closing edge is off by 7
  std::vector<RelativeSEMeasurement> ms;
  ms.push_back(RelativeSEMeasurement(0, 0, 0, 1, I, step, 1.0, 1.0));
  ms.push_back(RelativeSEMeasurement(0, 0, 1, 2, I, step, 1.0, 1.0));
  ms.push_back(RelativeSEMeasurement(0, 0, 0, 2, I, far, 1.0, 1.0));
  ms[0].fixedWeight = ms[1].fixedWeight = true;  // odometry
  auto pg = std::make_shared<PoseGraph>(0, r, d);
  pg->setMeasurements(ms);
  QuadraticProblem problem(pg);
  Matrix X(r, b * n);  // poses on the x axis at 0, 1.25, 2: odometry residuals 0.25^2
  const double px[3] = {0.0, 1.25, 2.0};
  for (int i = 0; i < n; ++i) {
    for (int k = 0; k < d; ++k) X(k, i * b + k) = 1.0;
    X(0, i * b + d) = px[i];
  }
  if (problem.setReweightableEdges() != 3) return 1;
  RobustCostParameters prm;
  prm.costType = RobustCostParameters::Type::Huber;
  RobustCost cost(prm);  // threshold 3
  const dpgo_reweight_stats st = problem.robustReweight(X, cost, 1e-8, true);
  std::vector<double> w, rsq;
  problem.getEdgeWeights(w, rsq);
  bool ok = w.size() == 3 && w[0] == 1.0 && w[1] == 1.0 && rsq[0] == 0.0625 && rsq[1] == 0.0625 && rsq[2] == 49.0;
  ok = ok && std::fabs(w[2] - cost.weight(std::sqrt(rsq[2]))) <= 4e-16 && std::fabs(w[2] - 3.0 / 7.0) <= 4e-16;
  ok = ok && st.inliers == 0 && st.outliers == 0 && st.undecided == 1 && st.skipped == 0 && st.max_rsq == 49.0;
  // Huber beyond the threshold: 3 * 7 - 9 / 2, plus the two fixed edges' w r^2 / 2
  ok = ok && std::fabs(st.cost - (16.5 + 0.0625)) <= 1e-14;
  std::printf("w %.17g %.17g %.17g  rsq %.17g %.17g %.17g  counts %d %d %d %d  cost %.17g\n", w[0], w[1], w[2], rsq[0], rsq[1],
              rsq[2], st.inliers, st.outliers, st.undecided, st.skipped, st.cost);
  // an L1 update at a zero residual is skipped, not stored
  prm.costType = RobustCostParameters::Type::L1;
  const double at[3] = {0.0, 1.0, 2.0};
  for (int i = 0; i < n; ++i) X(0, i * b + d) = at[i], X(1, i * b + d) = i == 2 ? 7.0 : 0.0;
  const dpgo_reweight_stats s1 = problem.robustReweight(X, RobustCost(prm), 1e-8, true);
  problem.getEdgeWeights(w, rsq);
  ok = ok && rsq[2] == 0.0 && s1.skipped == 1 && std::fabs(w[2] - 3.0 / 7.0) <= 4e-16;
  std::printf(ok ? "robust costs: ok\n" : "robust costs: FAILED\n");
  return ok ? 0 : 1;
}
