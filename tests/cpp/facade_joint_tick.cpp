// facade_joint_tick.cpp -- drives CfManager::selectClearAgainst (include/bimanual_planning_ros/cf_manager.h) inside the
// intended tick on the static1 task scene, against two paths of "the other arm" given by a formula, and prints, per
// tick, the selection and the next set-point. tests/test_pair_clear_gpu.py compares the output with the same calls made
// through the C-ABI (pmaf_select_clear_tracks).
//   usage: facade_joint_tick <n_agents> <max_prediction_steps> <n_ticks> <random_vecs.bin> <margin> <horizon>
//                            <separation> <pair_margin> <late> <other_late>      (late < 0: step against step)
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "bimanual_planning_ros/cf_manager.h"

using namespace ghostplanner::cfplanner;

int main(int argc, char **argv) {
  if (argc < 11) return 2;
  const int N = atoi(argv[1]), cap = atoi(argv[2]), ticks = atoi(argv[3]);
  const double margin = atof(argv[5]);
  const int horizon = atoi(argv[6]);
  const double separation = atof(argv[7]), pair_margin = atof(argv[8]);
  const int late = atoi(argv[9]), other_late = atoi(argv[10]);
  // static1 scene: 9 spheres + repulsive sentinel (values as in pmaf scenes.static1_obstacles)
  std::vector<Obstacle> obstacles;
  const double xs[3] = {0.125, 0.125, -0.35}, zs[3] = {1.0, 0.7, 0.6}, ys[3] = {0.0, 0.125, -0.125};
  for (int g = 0; g < 3; ++g)
    for (int k = 0; k < 3; ++k) obstacles.push_back(Obstacle(Vector3d(xs[g], ys[k], zs[g]), Vector3d(0, 0, 0), 0.1));
  obstacles.push_back(Obstacle(Vector3d(100.0, 100.0, 100.0), Vector3d(0, 0, 0), 0.1));
  std::vector<double> rv((size_t)N * obstacles.size() * 3);
  FILE *f = fopen(argv[4], "rb");
  if (!f || fread(rv.data(), sizeof(double), rv.size(), f) != rv.size()) return 3;
  fclose(f);

  const Vector3d start(-0.6, 0.0, 0.75), goal(0.5, 0.0, 0.7);
  const double dt = 0.01;
  Vector6d ws;
  const double wsv[6] = {1.0, -1.0, 0.3, -0.3, 1.1, 0.2};
  for (int i = 0; i < 6; ++i) ws(i) = wsv[i];
  // the other arm: a line beside this arm's start that closes in, cap points; and a short path that ends after 5
  std::vector<std::vector<Vector3d>> other(2);
  for (int k = 0; k < cap; ++k) other[0].push_back(Vector3d(-0.6 + 0.002 * k, 0.25 - 0.001 * k, 0.75));
  for (int k = 0; k < 5; ++k) other[1].push_back(Vector3d(-0.6 + 0.002 * k, -0.3, 0.75));

  CfManager m;
  m.setInitialPosition(start);
  m.setRandomVectors(rv);
  m.init(goal, dt, obstacles, std::vector<double>(N, 4.0), std::vector<double>(N, 0.025), std::vector<double>(N, 0.08),
         std::vector<double>(N, 3.0), std::vector<double>(N, 0.0), std::vector<double>(1, 0.02), 0.2, 0.25, 0.35, cap, 1);
  m.setInitialPosition(start);
  for (int t = 0; t < ticks; ++t) {
    m.stopPrediction();
    m.evaluateAgents(obstacles, 100.0, 10.0, 0.001, 1.0, ws);
    const JointSelection s = late < 0 ? m.selectClearAgainst(obstacles, margin, horizon, other, separation, pair_margin, true)
                                      : m.selectClearAgainst(obstacles, margin, horizon, other, separation, pair_margin, late,
                                                             other_late, true);
    if (s.pick < 0) return 4;
    m.moveRealEEAgent(obstacles, dt, 1, s.pick);
    double p[3], v[3];
    if (pmaf_get_real_state(m.handle(), p, v, nullptr) != 0) return 5;
    m.resetEEAgents(Vector3d(p[0], p[1], p[2]), Vector3d(v[0], v[1], v[2]), obstacles);
    m.startPrediction();
    printf("%d %d %d %d %d %d %d %d %d %.17g %.17g %.17g %.17g %.17g %.17g %.17g %d\n", t, s.pick, s.track, s.rule, s.n_feasible,
           s.n_clear, s.first_violation, s.step, s.other_step, s.cost, s.clearance, s.obstacle_clearance, s.worst_excess, p[0],
           p[1], p[2], m.getBestAgentType());
  }
  m.stopPrediction();
  return 0;
}
