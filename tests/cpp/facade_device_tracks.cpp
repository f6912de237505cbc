// facade_device_tracks.cpp -- drives CfManager::setObstacleTracksDevice (include/bimanual_planning_ros/cf_manager.h) in
// front of planTick on the static1 task scene: the tracks of facade_ftracked_tick.cpp -- nine spheres on a formula, the
// first one beside the arm -- as float positions only ([L][9][3]), allocated with hipMalloc and copied to the device;
// attached once at offset 2, advanced by one in front of the later ticks, attached again (a shorter run, from the device)
// in front of the last but one, detached for the last. Prints, per tick, the selection, the set-point and the selected
// agent's predicted path end. tests/test_track_ingest_gpu.py compares the output with the same calls made through the
// binding.
//   usage: facade_device_tracks <n_agents> <max_prediction_steps> <n_ticks> <random_vecs.bin> <track_points>
#include <hip/hip_runtime_api.h>

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
  // the positions: sphere 0 beside the arm, closing in; the others drift along x (rounded to float as a predictor's
  // output would be)
  std::vector<float> pts((size_t)L * 9 * 3);
  for (int k = 0; k < L; ++k)
    for (int i = 0; i < 9; ++i) {
      const Vector3d p0 = obstacles[i].getPosition();
      float *p = &pts[((size_t)k * 9 + i) * 3];
      if (i == 0) { p[0] = (float)(-0.6 + 0.002 * k); p[1] = (float)(0.3 - 0.001 * k); p[2] = 0.75f; }
      else { p[0] = (float)(p0.x() + 0.0005 * k); p[1] = (float)p0.y(); p[2] = (float)p0.z(); }
    }
  void *d_pts = nullptr;
  if (hipMalloc(&d_pts, pts.size() * sizeof(float)) != hipSuccess) return 4;
  if (hipMemcpy(d_pts, pts.data(), pts.size() * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) return 4;
  for (int t = 0; t < ticks; ++t) {
    if (t == 0) m.setObstacleTracksDevice(d_pts, L, 3, PMAF_TRACK_F32, nullptr, 2);
    else if (t + 2 < ticks) m.advanceObstacleTracks();
    else if (t + 2 == ticks) m.setObstacleTracksDevice(d_pts, L / 2, 3, PMAF_TRACK_F32);
    else m.setObstacleTracksDevice(d_pts, 0, 3, PMAF_TRACK_F32);
    Vector3d next;
    const int best = m.planTick(obstacles, dt, 100.0, 10.0, 0.001, 1.0, ws, &next);
    m.stopPrediction();
    const std::vector<std::vector<Vector3d>> &paths = m.getPredictedPaths();
    const Vector3d e = paths[best].back();
    printf("%d %d %zu %.17g %.17g %.17g %.17g %.17g %.17g\n", t, best, paths[best].size(), next.x(), next.y(), next.z(), e.x(),
           e.y(), e.z());
  }
  (void)hipFree(d_pts);
  return 0;
}
