// facade_slack_tick.cpp -- drives CfManager::planTickAudited(..., tracked = true, late, early), selectClearSlack and
// evaluatePathsSlack (include/bimanual_planning_ros/cf_manager.h) on the static1 task scene: the nine spheres follow
// the tracks of facade_ftracked_tick.cpp, uploaded once; every tick but the first advances the offset by one. Per tick
// it prints the slacked selection, the set-point, then -- behind stopPrediction -- the slacked audit of the new paths at
// the handle's offset and a slacked selection at an explicit one. tests/test_obstacle_slack_audit_gpu.py compares the
// output with the same calls made through the C-ABI.
//   usage: facade_slack_tick <n_agents> <max_prediction_steps> <n_ticks> <random_vecs.bin> <track_points> <margin> <horizon>
//                            <late> <early>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "bimanual_planning_ros/cf_manager.h"

using namespace ghostplanner::cfplanner;

int main(int argc, char **argv) {
  if (argc < 10) return 2;
  const int N = atoi(argv[1]), cap = atoi(argv[2]), ticks = atoi(argv[3]), L = atoi(argv[5]), horizon = atoi(argv[7]);
  const int late = atoi(argv[8]), early = atoi(argv[9]);
  const double margin = atof(argv[6]);
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
  // the tracks: sphere 0 beside the arm, closing in; the others drift along x with a velocity of their own
  std::vector<std::vector<Obstacle>> tracks;
  for (int k = 0; k < L; ++k) {
    std::vector<Obstacle> step;
    for (int i = 0; i < 9; ++i) {
      const Vector3d p0 = obstacles[i].getPosition();
      if (i == 0) step.push_back(Obstacle(Vector3d(-0.6 + 0.002 * k, 0.3 - 0.001 * k, 0.75), Vector3d(0.2, -0.1, 0.0), 0.1));
      else step.push_back(Obstacle(Vector3d(p0.x() + 0.0005 * k, p0.y(), p0.z()), Vector3d(0.05, 0.0, 0.01 * i), 0.1));
    }
    tracks.push_back(step);
  }
  m.setObstacleTracks(tracks, 2);
  m.startPrediction();
  for (int t = 0; t < ticks; ++t) {
    if (t > 0) m.advanceObstacleTracks();
    Vector3d next;
    ClearSelection s;
    const int pick = m.planTickAudited(obstacles, dt, 100.0, 10.0, 0.001, 1.0, ws, margin, horizon, &next, &s, true, late, early);
    m.stopPrediction();
    const PathAudit a = m.evaluatePathsSlack(obstacles, margin, late, early);
    const ClearSelection c = m.selectClearSlack(obstacles, margin, horizon, early, late, false, std::vector<int>(1, 7), true);
    printf("%d %d %d %d %d %.17g %.17g %.17g %.17g %.17g %.17g %d %d %d %d %d %d %.17g\n", t, pick, s.rule, s.n_clear,
           s.first_violation, s.cost, s.clearance, next.x(), next.y(), next.z(), a.clearance[pick], a.step[pick],
           a.obstacle_step[pick], a.obstacle[pick], a.first_violation[pick], c.pick, c.first_violation, c.clearance);
  }
  return 0;
}
