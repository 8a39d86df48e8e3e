// QuadraticProblem::certify / certificateApply of the C++ mirror (include/dpgo_hip.hpp) on the 16-pose ring with identity
// measurements, iterate at winding number 1 (a saddle: lambda_min(C) = -2 (1 - cos(2 pi / 16)), multiplicity 2).
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
  const int n = 16, d = 3, r = 3, b = d + 1;
  std::vector<RelativeSEMeasurement> ms;
  Matrix I = Matrix::Identity(3, 3), t(3, 1);
  for (int i = 0; i < n; ++i) ms.push_back(RelativeSEMeasurement(0, 0, i, (i + 1) % n, I, t, 1.0, 1.0));
  auto pg = std::make_shared<PoseGraph>(0, r, d);
  pg->setMeasurements(ms);
  QuadraticProblem problem(pg);
  Matrix X(r, b * n);
  for (int i = 0; i < n; ++i) {
    const double th = 2 * M_PI * i / n;
    X(0, i * b + 0) = std::cos(th), X(1, i * b + 0) = std::sin(th);
    X(0, i * b + 1) = -std::sin(th), X(1, i * b + 1) = std::cos(th);
    X(2, i * b + 2) = 1.0;
  }
  const Matrix XC = problem.certificateApply(X, X);
  dpgo_certify_params prm;
  dpgo_certify_params_default(&prm);
  prm.tol_rel = 1e-9;
  std::vector<double> w;
  const dpgo_certify_result res = problem.certify(X, &prm, &w);
  const double lam = -2 * (1 - std::cos(2 * M_PI / n));
  double wn = 0;
  for (double v : w) wn += v * v;
  std::printf("|X C| %.3e  status %d  lambda_min %.9f (%.9f)  deflated %d  |w| %.12f\n", XC.norm(), res.status,
              res.lambda_min, lam, res.deflated, std::sqrt(wn));
  const bool ok = XC.norm() < 1e-12 && res.status == DPGO_CERT_NOT_CERTIFIED && std::fabs(res.lambda_min - lam) < 1e-8 &&
                  res.deflated == d + 1 && std::fabs(std::sqrt(wn) - 1) < 1e-10;
  std::printf(ok ? "certify: ok\n" : "certify: FAILED\n");
  return ok ? 0 : 1;
}
