// Stand-alone driver of csrc/pmaf_route.hpp for tests/test_route_field_track.py: tests/cpp/route_table.cpp's records with
// the `tracked` and `field_tracked` inputs in front of each and Route::carries_track / carries_field_tracks behind each
// result. No library, no device.
//   in:  tracked field_tracked N P M n_simds lanes_request math plain_step external mw_refused force_generic mw mw_per mw_lds_kb dpp_sum w64_slice
//   out: family lpa slots tiles waves per mw_lds_kb sliced dpp_sum plain math closest_table tuned_real_step n_blocks lds_rollout carries_track carries_field_tracks
#include <cstdio>

#include "pmaf_route.hpp"

int main() {
  pmaf_route::Input in;
  int tracked, ftracked, plain, ext, refused, fg, dpp, slice;
  while (std::scanf("%d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d", &tracked, &ftracked, &in.N, &in.P, &in.M, &in.n_simds,
                    &in.lanes_request, &in.math, &plain, &ext, &refused, &fg, &in.mw, &in.mw_per, &in.mw_lds_kb, &dpp, &slice) == 17) {
    in.tracked = tracked != 0; in.field_tracked = ftracked != 0;
    in.plain_step = plain != 0; in.external = ext != 0; in.mw_refused = refused != 0;
    in.force_generic = fg != 0; in.dpp_sum = dpp != 0; in.w64_slice = slice != 0;
    const pmaf_route::Route r = pmaf_route::route(in);
    std::printf("%d %d %d %d %d %d %d %d %d %d %d %d %d %d %zu %d %d\n", (int)r.family, r.lpa, r.slots, r.tiles, r.waves, r.per,
                r.mw_lds_kb, (int)r.sliced, (int)r.dpp_sum, (int)r.plain, r.math, (int)r.closest_table,
                (int)r.tuned_real_step, r.n_blocks, r.lds_rollout, (int)r.carries_track, (int)r.carries_field_tracks);
  }
  return 0;
}
