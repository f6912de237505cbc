// facade_ftracked_tick.cpp -- drives CfManager::setObstacleTracks / advanceObstacleTracks
// (include/bimanual_planning_ros/cf_manager.h) in front of planTick on the static1 task scene: the nine spheres follow
// tracks given by a formula -- the first one travels beside the arm -- uploaded once; every tick but the first advances
// the offset by one, and the last tick runs detached. Prints, per tick, the selection, the set-point and the selected
// agent's predicted path end. tests/test_field_track_gpu.py compares the output with the same calls made through the
// C-ABI (pmaf_set_obstacle_tracks + pmaf_set_obstacle_track_offset + pmaf_tick).
//   usage: facade_ftracked_tick <n_agents> <max_prediction_steps> <n_ticks> <random_vecs.bin> <track_points>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "bimanual_planning_ros/cf_manager.h"

using namespace ghostplanner::cfplanner;

int main(int argc, char **argv) {
  if (argc < 6) return 2;
  const int N = atoi(argv[1]), cap = atoi(argv[2]), ticks = atoi(argv[3]), L = atoi(argv[5]);
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
  m.startPrediction();
  // the tracks: sphere 0 beside the arm, closing in; the others drift along x with a velocity of their own
  std::vector<std::vector<Obstacle>> tracks;
  for (int k = 0; k < L; ++k) {
    std::vector<Obstacle> step;
    for (int i = 0; i < 9; ++i) {
      const Vector3d p0 = obstacles[i].getPosition();
      if (i == 0) step.push_back(Obstacle(Vector3d(-0.6 + 0.002 * k, 0.3 - 0.001 * k, 0.75), Vector3d(0.2, -0.1, 0.0), 0.1));
      else step.push_back(Obstacle(Vector3d(p0.x() + 0.0005 * k, p0.y(), p0.z()), Vector3d(0.05, 0.0, 0.01 * i), 0.1));
    }
    if (k % 2) step.push_back(obstacles.back());   // (M + 1 entries: the last is ignored)
    tracks.push_back(step);
  }
  for (int t = 0; t < ticks; ++t) {
    if (t == 0) m.setObstacleTracks(tracks, 2);
    else if (t + 1 < ticks) m.advanceObstacleTracks();
    else m.setObstacleTracks(std::vector<std::vector<Obstacle>>());
    Vector3d next;
    const int best = m.planTick(obstacles, dt, 100.0, 10.0, 0.001, 1.0, ws, &next);
    m.stopPrediction();
    const std::vector<std::vector<Vector3d>> &paths = m.getPredictedPaths();
    const Vector3d e = paths[best].back();
    printf("%d %d %zu %.17g %.17g %.17g %.17g %.17g %.17g\n", t, best, paths[best].size(), next.x(), next.y(), next.z(), e.x(),
           e.y(), e.z());
  }
  return 0;
}
