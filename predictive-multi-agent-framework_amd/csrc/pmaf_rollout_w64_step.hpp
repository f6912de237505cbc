// pmaf_rollout_w64_step.hpp -- the TEXT of one step of the wave-per-agent rollout: the body of rollout_w64_body's step
// loop (pmaf_rollout_w64_body.hpp), which includes this file once per step loop, inside the function, with
// PMAF_STEP_LONG defined to the loop's `LONG` argument of circ_and_scale_w64 (pmaf_rollout_w64.hpp): false -- the short
// loop, every instantiation; true -- the long loop of the one-slot DPP sum, which adds the list's second chunk in the
// block of the attractor-scaling chain. PMAF_STEP_FLAG is the tail of the call's argument list: `, &short_cap` in those two
// loops (the hand-over, see circ_and_scale_w64), empty in every other instantiation's single loop, whose call is then
// the one it always was. No include guard and nothing but statements: every name is a local or a
// template parameter of rollout_w64_body. A file and not a macro, a lambda or a helper: the two loops share the text, and
// the short loop's tokens are those of the single loop it was (NOTES.md 1: anything between kernel and body moves the
// one-slot schedule).
#ifndef PMAF_STEP_LONG
#error "include from rollout_w64_body with PMAF_STEP_LONG defined"
#endif
    unsigned long long clk = 0ull;
    if (SLICE) clk = wall_clock64();
    // repulsive track: the point of the COMING step (step n, held at the last one) is requested here, a whole step ahead
    // of the tail that consumes it
    V3 trk_next = mk(0.0, 0.0, 0.0);
    if (TRACK && SENT == 1) {
      const gptr tp = trk_v + 3 * ((n < trk_last) ? n : trk_last);
      trk_next = mk(tp[0], tp[1], tp[2]);
    }
    // obstacle tracks: likewise -- step n's point min(ftrk_at + n, last), six loads per lane
    V3 ftrk_np = mk(0.0, 0.0, 0.0), ftrk_nv = mk(0.0, 0.0, 0.0);
    if (FTRACK) {
      const int fi = (n < ftrk_last - ftrk_at) ? (ftrk_at + n) : ftrk_last;
      const gptr fp = ftrk_v + (size_t)fi * 384;
      ftrk_np = mk(fp[0], fp[64], fp[128]);
      ftrk_nv = mk(fp[192], fp[256], fp[320]);
    }
    // gate, :315-317
    // |v| < 0.5 vmax and |p - init| < 0.2 on exact squared thresholds
    // (as a lane mask built from single compares: pmaf_rollout_w64.hpp, "lane predicates as masks")
    const lmask gate_m = ~(PMAF_BAL(dg < C.approach) | (PMAF_BAL(zv < C.zvhalf_lt) & PMAF_BAL(z_init < C.zinit_lt)));
    const bool gate = gate_m != 0ull;
    V3 F = mk(0.0, 0.0, 0.0);
    double scale = 1.0;
    PMAF_SEC(ST, 0);
    // (called with the gate closed too: the sweep's few compares then find no obstacle -- one branch less in the step)
    if (PRE || gate)
      circ_and_scale_w64<TILES, TYPE, MATH, PRE, DPPSUM, decltype(EK), (STATICV ? (SENT == 1 ? 59 : 60) : -1), PMAF_STEP_LONG>(lane, p, v, zv, goal, g, dg, gn, C, k_circ, n_obs, rot_g, known_bits,
                                                 O, clist, lane_min, F, scale, ST, EK, 0, s_pre, ron_pre,
                                                 gate_m, cidx PMAF_STEP_FLAG);
    PMAF_SEC(ST, 5);
    // attractorForce (:183-193), updatePositionAndVelocity (:253-268)
    // repelForce (:159-181): `repel` was evaluated for this step's start state at the end of the previous step; it is
    // +0.0 when the obstacle cannot come into range, and F -- a sum that started from +0.0 -- is never -0.0, so the
    // unconditional addition is exact (no masked block between the force sum and the tail)
    F = F + (mk(0.0, 0.0, 0.0) + repel);
    // attractorForce (:183-193), updatePositionAndVelocity (:253-258): a = F / mass, |a| <= 13
    V3 acc;
    if (PLAIN) {
      F = F + (scale * k_damp) * verr;
      acc = F;
      const double az = sqn(F);
      if (PMAF_RARE(wave_any(az >= C.zacc_gt))) acc = acc * (13.0 / __builtin_sqrt(az));  // norm(acc) > 13.0
    } else if (PRE) {
      // one slot per lane: as few blocks as possible between the force sum and the tail -- the k_attr == 0 case is a
      // select, and unit mass without clamp (the common case) skips ONE rare block instead of two
      const V3 Fa = F + (scale * k_damp) * verr;
      const bool attr = (k_attr != 0.0);
      F.x = attr ? Fa.x : F.x; F.y = attr ? Fa.y : F.y; F.z = attr ? Fa.z : F.z;
      acc = F;
      double az = sqn(F);
      // (wave-uniform and rare: __any makes the branch a scalar one the block placement can move out of line)
      if (PMAF_RARE(wave_any((C.mass != 1.0) || (az >= C.zacc_gt)))) {
        if (C.mass != 1.0) { acc = F / C.mass; az = sqn(acc); }
        if (az >= C.zacc_gt) acc = acc * (13.0 / __builtin_sqrt(az));  // norm(acc) > 13.0
      }
    } else {
      if (k_attr != 0.0) F = F + (scale * k_damp) * verr;
      acc = F;
      if (C.mass != 1.0) acc = F / C.mass;
      const double az = sqn(acc);
      if (az >= C.zacc_gt) acc = acc * (13.0 / __builtin_sqrt(az));  // norm(acc) > 13.0 (rare)
    }
    PMAF_SEC(ST, 6);
    // ---- one block: integrate, clamp the speed, the next step's norms ----
    const V3 half = ((0.5 * acc) * C.dt) * C.dt;
    const V3 new_pos = (p + half) + (v * C.dt);
    const V3 nv = v + acc * C.dt;
    p = new_pos;
    g = goal - p;
    // predictObstacles, B/src/cf_agent.cpp:270-276, in registers. Obstacles at
    // rest: p + (+-0) dt is idempotent after its first application (which turns
    // a -0.0 coordinate into +0.0), so later steps skip it. (Lanes 63 / 61 of the one-slot kernel hold the goal with
    // velocity -0.0: the update leaves it bit for bit.)
    // (one slot per lane: unconditionally -- for obstacles at rest every further application is the identity, and
    // three multiply-adds are cheaper than a branch in the middle of the tail. The STATICV body without the repulsive
    // obstacle drops it: the FIRST application is the identity there too, field_obstacles_at_rest says so -- three
    // multiplies and three adds per step, -ffp-contract=off. With the obstacle in lane 60 it stays: that lane moves.)
    if (PRE && !(STATICV && SENT == 0)) O.p[0] = O.p[0] + O.v[0] * C.dt;
    if (TRACK && SENT == 1) {   // lane 60 takes the track's point in place of o + v dt (three selects, no masked block)
      const bool tl = PMAF_LANE(trk_m);
      O.p[0].x = tl ? trk_next.x : O.p[0].x; O.p[0].y = tl ? trk_next.y : O.p[0].y; O.p[0].z = tl ? trk_next.z : O.p[0].z;
    }
    if (FTRACK) {   // lanes 0 .. M-1 take the point's position and velocity (six selects under a loop-invariant mask)
      const bool fl = PMAF_LANE(ftrk_m);
      O.p[0].x = fl ? ftrk_np.x : O.p[0].x; O.p[0].y = fl ? ftrk_np.y : O.p[0].y; O.p[0].z = fl ? ftrk_np.z : O.p[0].z;
      O.v[0].x = fl ? ftrk_nv.x : O.v[0].x; O.v[0].y = fl ? ftrk_nv.y : O.v[0].y; O.v[0].z = fl ? ftrk_nv.z : O.v[0].z;
    }
    {
      // ONE sqrt / reciprocal / divide sequence for the whole tail: lane 63 goal distance and direction (|g|,
      // g.normalized()), lane 62 the speed clamp (|nv|, vel_max / |nv|), lane 61 attractorForce's limit
      // (vel_max / |vel_des|) and, in the one-slot kernel, lanes 0..M-1 the next step's |ro| and ro.normalized():
      // the same operations on the same operands as separate sequences, read back with v_readlane.
      const V3 vel_des = (k_attr / k_damp) * g;
      const bool l_nv = (lane == 62), l_des = (lane == 61);
      const V3 other = PRE ? (O.p[0] - p) : g;   // one-slot kernel: lanes 63 and 61 hold the goal, O.p - p = g there
      const V3 vec = l_nv ? nv : (other * lane_scale);   // lane 61: (k_attr / k_damp) * g = vel_des, the same product
      V3 num = vec;
      num.x = (l_nv || l_des) ? C.vel_max : vec.x;
      // normalized(): the vector itself unless squaredNorm > 0 -- by ONE select on the divisor (x / 1.0 == x for every
      // x, zeros keep their sign, a NaN stays one) instead of three on the quotients; the riders' lanes divide by their
      // norm whatever it is (vel_max / 0 = inf: the fixup of the x component supplies it)
      const double zvec = sqn(vec);
      const double s = MT::sqrt(zvec);
      const double sd = PMAF_LANE(PMAF_BAL(zvec > 0.0) | (3ull << 61)) ? s : 1.0;
      const double rs = MT::rcp_for(sd);
      // (y and z: direction components only; x also carries the riders' vel_max / |.| quotients)
      const V3 q = mk(MT::div_n(num.x, sd, rs), MT::div_n_pos(num.y, sd, rs), MT::div_n_pos(num.z, sd, rs));
      const V3 u = q;
      if (PRE) { s_pre = s; ron_pre = u; }
      const double vn = readlane_d(s, 62), f_nv = readlane_d(q.x, 62), f_des = readlane_d(q.x, 61);
      // (the clamp as a select on the FACTOR: nv * 1.0 is nv exactly -- two selects instead of six)
      v = nv * ((vn > C.vel_max) ? f_nv : 1.0);
      dg = readlane_d(s, 63);
      gn = readlane_v3(u, 63);
      verr = vel_des * smin(1.0, f_des) - v;
      if (SRIDE) {
        // repelForce (:159-181) of the coming step from lane 60's norm and direction: z = |sent_pos - p|^2 is the squared
        // norm of dist_vec (same components up to sign), otr = normalized(p - sent_pos) = -(ro / |ro|) (a zero component's
        // sign differs: F + (0 + repel) below does not see it)
        const double z60 = readlane_d(zvec, 60);
        repel = mk(0.0, 0.0, 0.0);
        if (z60 < zsent_lt) {
          const double s60 = readlane_d(s, 60);
          const V3 u60 = readlane_v3(u, 60);
          double d = s60 - (C.rad + sent_r);
          d = smax(d, 1e-5);
          const V3 otr = -u60;
          const double t = MT::div_pos(1.0, d) - inv_shell;
          const double dd = d * d;
          const V3 num2 = (k_repel * otr) * t;
          repel = MT::div3_n_pos(num2, dd, MT::rcp_for(dd));
        }
      }
    }
    zv = sqn(v);
    z_init = sqn(p - init_pos);
    // every lane stores the (wave-uniform) point to the same address: one transaction, and no exec-masked block
    // in the middle of the tail
    PMAF_BOUND(n < D.cap);
    path[n * 3] = p.x; path[n * 3 + 1] = p.y; path[n * 3 + 2] = p.z;
    n++;
    ran = true;
    if (!PRE && advance) {
#pragma unroll
      for (int t = 0; t < TILES; t++) O.p[t] = O.p[t] + O.v[t] * C.dt;
      advance = moving;
    }
    // (decided at run time in the multi-slot kernels: out of line there -- in the shipped scenes the obstacle sits 170 m
    // away, and a block that is skipped costs a taken branch per step)
    if (SRIDE) {
    } else if ((SENT == 2) ? PMAF_RARE(sent_reachable) : sent_reachable) {  // the only masked block of the step for the repulsive obstacle: advance it, next step's repelForce
      sent_p = sent_p + sent_v * C.dt;
      repel = sentinel_repel_m<MATH>(p, C, k_repel, sent_p, sent_r, zsent_lt, inv_shell);
    }
    PMAF_SEC(ST, 7);
    if (SLICE) {
      if (((((unsigned)(clk >> slice_log2)) & 7u) < younger_of_8) == younger) __builtin_amdgcn_s_setprio(1);
      else __builtin_amdgcn_s_setprio(0);
    }
