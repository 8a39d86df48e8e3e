// evalTeam and escapeTeam of the C++ mirror (include/dpgo_hip.hpp) on the 16-pose ring with identity measurements as TWO
// agents of 8 poses, iterate at winding number 1 (a saddle: f = 16 (1 - cos(2 pi / 16)) 2, |rgrad| = 0): the team's cost and
// gradient norm in one launch, the witness of certifyTeam, and the escape to rank r + 1 along it -- the first trial step
// alpha0 = 0.1 sqrt(16) is accepted, f falls from 2.435855 to 2.423796 (tests/test_team_staircase_reference_cpu.py pins
// both on the numpy reference) and the rank-4 agents evaluate the new iterate to the same f.
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
  std::vector<RelativeSEMeasurement> team_ms;
  for (int i = 0; i < n; ++i) {
    const int j = (i + 1) % n;
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

  // the same two agents at rank r and at rank r + 1
  std::vector<std::unique_ptr<QuadraticProblem>> agents;
  std::vector<QuadraticProblem*> team[2];
  std::vector<int> firsts;
  std::vector<std::vector<int32_t>> nbr_pose;
  for (int lift = 0; lift < 2; ++lift)
    for (int a = 0; a < 2; ++a) {
      auto pg = std::make_shared<PoseGraph>(a, r + lift, d);
      pg->setMeasurements(team_ms);
      agents.emplace_back(new QuadraticProblem(pg, 0, false));
      check(dpgo_problem_set_stream(agents.back()->handle(), nullptr));
      std::vector<int32_t> np;
      for (const PoseGraph::PoseID& id : agents.back()->setCouplingFromPoseGraph())
        np.push_back((int32_t)(id.first * half + id.second));
      if (lift == 0) {
        firsts.push_back(a * half);
        nbr_pose.push_back(np);
      }
      team[lift].push_back(agents.back().get());
    }
  double *Xd = nullptr, *wd = nullptr, *Xn = nullptr;
  check(dpgo_device_malloc((void**)&Xd, sizeof(double) * r * b * n, 0));
  check(dpgo_device_malloc((void**)&wd, sizeof(double) * b * n, 0));
  check(dpgo_device_malloc((void**)&Xn, sizeof(double) * (r + 1) * b * n, 0));
  check(dpgo_device_memcpy(Xd, X.data(), sizeof(double) * r * b * n, DPGO_COPY_H2D, nullptr));
  check(dpgo_device_synchronize(nullptr));
  const TeamEval e0 = evalTeam(team[0], firsts, nbr_pose, Xd);
  const dpgo_team_certify_result res = certifyTeam(team[0], firsts, nbr_pose, Xd, &prm, wd);
  const dpgo_team_escape_result esc = escapeTeam(team[1], firsts, nbr_pose, r, Xd, wd, 1e-9, Xn);
  const TeamEval e1 = evalTeam(team[1], firsts, nbr_pose, Xn);
  // members of rank r are refused, not run
  int rc_bad = DPGO_OK;
  try {
    escapeTeam(team[0], firsts, nbr_pose, r, Xd, wd, 1e-9, Xn);
  } catch (const Error& err) {
    rc_bad = err.code;
  }
  dpgo_device_free(Xd);
  dpgo_device_free(wd);
  dpgo_device_free(Xn);

  const double f0 = n * (1 - std::cos(2 * M_PI / n)) * 2;
  std::printf("f %.9f (formula %.9f) |rgrad| %.2e  status %d  escape: alpha %.3f trials %d f %.9f -> %.9f |rgrad| %.3e  "
              "rank-%d evaluation f %.9f |rgrad| %.3e  rank-%d members rc %d\n", e0.f, f0, e0.gradnorm, res.cert.status,
              esc.alpha, esc.trials, esc.f_before, esc.f_after, esc.gradnorm_after, r + 1, e1.f, e1.gradnorm, r, rc_bad);
  const bool ok = std::fabs(e0.f - f0) < 1e-12 * f0 && e0.gradnorm < 1e-12 && res.cert.status == DPGO_CERT_NOT_CERTIFIED &&
                  esc.alpha == 0.1 * std::sqrt((double)n) && esc.trials == 1 && esc.f_before == e0.f &&
                  std::fabs(esc.f_after - 2.423796) < 1e-6 && esc.f_after == e1.f && esc.gradnorm_after == e1.gradnorm &&
                  esc.gradnorm_after > 1e-9 && rc_bad == DPGO_ERR_INVALID;
  std::printf(ok ? "team escape: ok\n" : "team escape: FAILED\n");
  return ok ? 0 : 1;
}
