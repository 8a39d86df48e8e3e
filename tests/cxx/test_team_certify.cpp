// certifyTeam of the C++ mirror (include/dpgo_hip.hpp) on the 16-pose ring with identity measurements as TWO agents of 8
// poses, iterate at winding number 1 (a saddle: lambda_min(C) = -2 (1 - cos(2 pi / 16))): the team's certificate from the
// agents' own handles against the formula and against the central handle of the same ring.
// Exit 77 without a HIP device (no CPU fallback), 0 when every check holds.
#include <cmath>
#include <cstdio>
#include <memory>

#include "dpgo_hip.hpp"

using namespace dpgo_hip;

int main() {
  int devices = 0;
  if (dpgo_device_count(&devices) != DPGO_OK || devices == 0) {
    std::printf("no HIP device\n");
    return 77;
  }
  const int n = 16, half = 8, d = 3, r = 3, b = d + 1;
  Matrix I = Matrix::Identity(3, 3), t(3, 1);
  std::vector<RelativeSEMeasurement> central_ms, team_ms;
  for (int i = 0; i < n; ++i) {
    const int j = (i + 1) % n;
    central_ms.push_back(RelativeSEMeasurement(0, 0, i, j, I, t, 1.0, 1.0));
    team_ms.push_back(RelativeSEMeasurement(i / half, j / half, i % half, j % half, I, t, 1.0, 1.0));
  }
  Matrix X(r, b * n);
  for (int i = 0; i < n; ++i) {
    const double th = 2 * M_PI * i / n;
    X(0, i * b + 0) = std::cos(th), X(1, i * b + 0) = std::sin(th);
    X(0, i * b + 1) = -std::sin(th), X(1, i * b + 1) = std::cos(th);
    X(2, i * b + 2) = 1.0;
  }
  dpgo_certify_params prm;
  dpgo_certify_params_default(&prm);
  prm.tol_rel = 1e-9;

  auto pgc = std::make_shared<PoseGraph>(0, r, d);
  pgc->setMeasurements(central_ms);
  QuadraticProblem central(pgc);
  const dpgo_certify_result cen = central.certify(X, &prm);

  std::vector<std::unique_ptr<QuadraticProblem>> agents;
  std::vector<QuadraticProblem*> team;
  std::vector<int> firsts;
  std::vector<std::vector<int32_t>> nbr_pose;
  for (int a = 0; a < 2; ++a) {
    auto pg = std::make_shared<PoseGraph>(a, r, d);
    pg->setMeasurements(team_ms);
    agents.emplace_back(new QuadraticProblem(pg, 0, false));
    check(dpgo_problem_set_stream(agents.back()->handle(), nullptr));
    firsts.push_back(a * half);
    std::vector<int32_t> np;
    for (const PoseGraph::PoseID& id : agents.back()->setCouplingFromPoseGraph())
      np.push_back((int32_t)(id.first * half + id.second));
    nbr_pose.push_back(np);
    team.push_back(agents.back().get());
  }
  double *Xd = nullptr, *wd = nullptr;
  check(dpgo_device_malloc((void**)&Xd, sizeof(double) * r * b * n, 0));
  check(dpgo_device_malloc((void**)&wd, sizeof(double) * b * n, 0));
  check(dpgo_device_memcpy(Xd, X.data(), sizeof(double) * r * b * n, DPGO_COPY_H2D, nullptr));
  check(dpgo_device_synchronize(nullptr));
  const dpgo_team_certify_result res = certifyTeam(team, firsts, nbr_pose, Xd, &prm, wd);
  std::vector<double> w((size_t)b * n);
  check(dpgo_device_memcpy(w.data(), wd, sizeof(double) * b * n, DPGO_COPY_D2H, nullptr));
  // a table that does not tile [0, N) is refused, not run
  dpgo_team_member bad[2] = {{team[0]->handle(), 0, nbr_pose[0].data()}, {team[1]->handle(), half + 1, nbr_pose[1].data()}};
  dpgo_team_certify_result dummy{};
  const int rc_bad = dpgo_team_certify_device(bad, 2, Xd, &prm, &dummy, nullptr);
  dpgo_device_free(Xd);
  dpgo_device_free(wd);

  const double lam = -2 * (1 - std::cos(2 * M_PI / n));
  double wn = 0;
  for (double v : w) wn += v * v;
  std::printf("status %d (central %d)  lambda_min %.9f (formula %.9f, central %.9f)  deflated %d  |w| %.12f  defect %.2e  "
              "members %d poses %d  bad table rc %d\n", res.cert.status, cen.status, res.cert.lambda_min, lam, cen.lambda_min,
              res.cert.deflated, std::sqrt(wn), res.symmetry_defect, res.members, res.poses, rc_bad);
  const bool ok = res.cert.status == DPGO_CERT_NOT_CERTIFIED && cen.status == res.cert.status &&
                  std::fabs(res.cert.lambda_min - lam) < 1e-8 && std::fabs(res.cert.lambda_min - cen.lambda_min) < 1e-8 &&
                  res.cert.deflated == d + 1 && std::fabs(std::sqrt(wn) - 1) < 1e-10 && res.members == 2 && res.poses == n &&
                  res.symmetry_defect <= 8.0 * b * n * std::ldexp(1.0, -53) && rc_bad == DPGO_ERR_INVALID;
  std::printf(ok ? "team certify: ok\n" : "team certify: FAILED\n");
  return ok ? 0 : 1;
}
