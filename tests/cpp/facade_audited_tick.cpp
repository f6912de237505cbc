// facade_audited_tick.cpp -- drives CfManager::planTickAudited (include/bimanual_planning_ros/cf_manager.h) on the
// static1 task scene and prints, per tick, the selection and the next set-point. tests/test_select_clear_gpu.py compares
// the output with the same six calls made through the C-ABI.
//   usage: facade_audited_tick <n_agents> <max_prediction_steps> <n_ticks> <random_vecs.bin> <margin> <horizon>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "bimanual_planning_ros/cf_manager.h"

using namespace ghostplanner::cfplanner;

int main(int argc, char **argv) {
  if (argc < 7) return 2;
  const int N = atoi(argv[1]), cap = atoi(argv[2]), ticks = atoi(argv[3]);
  const double margin = atof(argv[5]);
  const int horizon = atoi(argv[6]);
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

  CfManager m;
  m.setInitialPosition(start);
  m.setRandomVectors(rv);
  m.init(goal, dt, obstacles, std::vector<double>(N, 4.0), std::vector<double>(N, 0.025), std::vector<double>(N, 0.08),
         std::vector<double>(N, 3.0), std::vector<double>(N, 0.0), std::vector<double>(1, 0.02), 0.2, 0.25, 0.35, cap, 1);
  m.setInitialPosition(start);
  for (int t = 0; t < ticks; ++t) {
    Vector3d np;
    ClearSelection s;
    const int pick = m.planTickAudited(obstacles, dt, 100.0, 10.0, 0.001, 1.0, ws, margin, horizon, &np, &s);
    if (pick != s.pick) return 4;
    printf("%d %d %d %d %d %.17g %.17g %.17g %.17g %.17g %d\n", t, s.pick, s.rule, s.n_clear, s.first_violation, s.cost,
           s.clearance, np.x(), np.y(), np.z(), m.getBestAgentType());
  }
  m.stopPrediction();
  return 0;
}
