"""Every one-slot wave-per-agent rollout instantiation that meets a list of more than 16 circular terms, written once:
the rows that tests/test_variant_matrix.py routes on the CPU (csrc/pmaf_route.hpp through tests/cpp/route_ftrack_table.cpp)
and that tests/test_variant_matrix_gpu.py runs over the K-varying scenes of tests/long_loop_scenes.py and
tests/sum_chunk_scenes.py. The default instantiation -- strict default policy, DPP sum, PLAIN step -- is not a row: it is
what tests/test_long_loop_gpu.py and tests/test_sum_chunks_gpu.py run, as are its track, ftrack and sliced kernels.

A row: a name; the keyword arguments of PmafPlanner that select the arithmetic policy; the environment to set before the
handle is created; whether the handle needs more agents than the device has SIMDs; whether a repulsive track or obstacle
tracks are attached; and the instantiation it stands for. launch_config() reports neither the policy nor the step nor
the sum, so what a row claims is checked against the route function on the CPU, not on the device.

Imports neither oracle/ nor the package."""
from collections import namedtuple

import numpy as np

# pmaf_device.hpp's policies, in pmaf_route.hpp's numbering
MATH = {"ieee": 0, "fast": 1, "xact": 2, "fma": 3}
POLICY_KW = {"xact": {}, "ieee": {"ieee_sequences": True}, "fast": {"fast_math": True}, "fma": {"contracted": True}}
WAVE_PER_AGENT = 2          # pmaf_route::Family

Row = namedtuple("Row", "name group policy kw env crowded track ftrack inst")


def _row(group, policy, dpp, plain, kernel="w64", crowded=False, forced=True):
    """forced: the general step is forced through the environment (else the scene's inputs have to ask for it)"""
    env = {}
    if not dpp:
        env["PMAF_SUM"] = "lds"
    if not plain and forced:
        env["PMAF_PLAIN_STEP"] = "0"
    name = "%s-%s-%s-%s" % (kernel, policy, "dpp" if dpp else "lds", "plain" if plain else "general" if forced else "general-by-input")
    inst = dict(family=WAVE_PER_AGENT, slots=1, dpp_sum=dpp, plain=plain, math=MATH[policy], sliced=crowded, kernel=kernel)
    return Row(name, group, policy, dict(POLICY_KW[policy]), env, crowded, kernel == "track", kernel == "ftrack", inst)


_SUM_STEP = [(dpp, plain) for dpp in (True, False) for plain in (True, False)]

# strict k_rollout_w64: bit for bit against the oracle
STRICT = [_row("strict", p, d, pl) for p in ("xact", "ieee") for d, pl in _SUM_STEP if (p, d, pl) != ("xact", True, True)]
# k_rollout_w64_track / _ftrack (default policy only): the three instantiations beside the DPP + PLAIN one
TRACK = [_row("track", "xact", d, pl, kernel="track") for d, pl in _SUM_STEP if (d, pl) != (True, True)]
FTRACK = [_row("ftrack", "xact", d, pl, kernel="ftrack") for d, pl in _SUM_STEP if (d, pl) != (True, True)]
# the policies that are not bit-exact: held to the high-precision reference's bound
BOUNDED = [_row("bounded", p, d, pl) for p in ("fast", "fma") for d, pl in _SUM_STEP]
# k_rollout_w64_sliced<3>: the contracted policy at more than one wave per SIMD
SLICED = [_row("sliced", "fma", True, True, kernel="sliced", crowded=True)]

ROWS = STRICT + TRACK + FTRACK + BOUNDED + SLICED

# the general step because the INPUTS need it (a non-unit mass, agents without attraction), nothing forced: the same
# instantiations as the strict rows' forced-general ones, reached the way a user reaches them
GENERAL_BY_INPUT = [_row("strict", p, d, False, forced=False) for p in ("xact", "ieee") for d in (True, False)]

GENERAL_MASS = 2.5
GENERAL_NO_ATTR = (1, 4)
GENERAL_VARIANTS = ("mass", "mass_noattr")
GENERAL_KS = (17, 33)


def general_scene(sc, variant):
    """a sum_chunk_scenes scene with inputs the PLAIN step is not valid for: agent_mass = 2.5 ("mass"), and on top of
    that k_attr = 0 for agents 1 and 4 ("mass_noattr")"""
    assert variant in GENERAL_VARIANTS
    out = dict(sc, name="%s_%s" % (sc["name"], variant), agent_mass=GENERAL_MASS)
    if variant == "mass_noattr":
        k = np.full(int(sc["n_agents"]), float(sc["k_attr"]))
        k[list(GENERAL_NO_ATTR)] = 0.0
        out["k_attr"] = k
    return out


def plain_input(row, sc):
    """Input::plain_step as the host derives it (pmaf_host.cpp refresh_plain_step): unit mass, every k_attr non-zero,
    and PMAF_PLAIN_STEP not "0" """
    k = np.broadcast_to(np.asarray(sc["k_attr"], dtype=np.float64), (int(sc["n_agents"]),))
    return bool(sc.get("agent_mass", 1.0) == 1.0 and (k != 0.0).all() and row.env.get("PMAF_PLAIN_STEP", "1")[:1] != "0")


def dpp_input(row):
    """Input::dpp_sum as pmaf_create reads PMAF_SUM"""
    v = row.env.get("PMAF_SUM", "")
    return v[:1] == "d" if v else True


def crowded_agents(n_simds):
    """the population of a crowded row: 1.5 waves per SIMD"""
    return n_simds + n_simds // 2


def apply_env(monkeypatch, row):
    """the row's environment, on a clean one"""
    for k in ("PMAF_SUM", "PMAF_FORCE_GENERIC", "PMAF_PLAIN_STEP", "PMAF_MW", "PMAF_W64_SLICE"):
        monkeypatch.delenv(k, raising=False)
    for k, v in row.env.items():
        monkeypatch.setenv(k, v)


# ---- the cases of each leg ----------------------------------------------------------------------------------------------
SUM_CHUNK_STRICT_FLAGS = ((False, False), (True, True))          # (moving, sent_near) run over every sum_chunk_scenes.KS
TRACK_KS = (17, 33)
# The bounded legs: one shadowed tick per case, tick 0. The condition (tests/test_variant_matrix.py): with the oracle in
# the planner's place every case has 0 undecidable samples under the fast and the contracted policy's bound.
# Measured, all seven long_loop_scenes cases x ticks 0 ... 2 under that bound (16 samples per tick):
#   sent_near = True:  ("runs", False) ticks 0, 1: 0, tick 2: 7;  ("runs", "cluster") tick 0: 0, ticks 1, 2: 7;
#                      ("bounds", False) tick 0: 0, ticks 1, 2: 7 (all seven rollouts at vel_clamp)
#   sent_near = False: ("runs", False), ("runs", "cluster"), ("bounds", False), ("bounds", "far"): 8 or 9 at EVERY tick --
#                      the real step (vel_clamp) and all seven rollouts (setvel_clamp). With the repulsive obstacle far
#                      away the agents fly at exactly vel_max along the x axis; the strict policies' exact root decides
#                      |v| > vel_max with bound 0 there, a policy with a rounded root cannot.
# So of the four cases first meant for this leg, ("runs", False, False) is replaced by ("runs", False, True), and
# ("bounds", "far", False) has no decidable substitute among the seven: ("bounds", False, True) is the only "bounds" case
# with 0. That leaves the long-loop leg on the bodies that carry the repulsive obstacle in range, at rest and advancing.
# The bodies for a far repulsive obstacle, at rest and advancing, run the sum-chunk scenes instead, which start slowly
# and are decided (0 of 16 each): K = 17 at (False, False) and K = 33 at (True, False), beside K = 17, 33, 49 at (True, True).
BOUNDED_LONG_LOOP = (("runs", False, True), ("runs", "cluster", True), ("bounds", False, True))
BOUNDED_SUM_CHUNK = ((17, True, True), (33, True, True), (49, True, True), (17, False, False), (33, True, False))
SLICED_LONG_LOOP = (("runs", False, True), ("bounds", False, True))       # (("runs", False, False): undecidable, see above)
BOUNDED_TICK = 0
MIN_ROLLOUT_SAMPLES = 7

_MEMO = {}      # the reference's rollouts, shared by every planner shadowed from the same inputs (hp_shadow.check_rollouts)


def shadow_first_tick(pl, sc, init, start, policy, name, agents=None):
    """tick 0 of a fresh planner on a K scene, shadowed by the high-precision reference under `policy`
    (tests/hp_shadow.py shadow_tick): the Stats, with the number of ROLLOUT samples that were compared (a tick's
    samples are the sampled agents' costs, the selection, the real step and the rollouts) in st.rollouts_compared"""
    import hp_reference as hp
    import hp_shadow as sh
    A = hp.Arith(policy)
    st = sh.Stats("%s [%s]" % (name, policy))
    st.rollouts_compared = 0

    def rollouts(A, st, *args):
        c0 = st.compared
        sh.check_rollouts(A, st, *args, memo=_MEMO)
        st.rollouts_compared += st.compared - c0
    ip = sh.start(pl, sc, init_pos=init, real_pos=start)
    sh.shadow_tick(pl, sc, sc["obstacles"], ip, A, st, agents=agents, rollouts=rollouts)
    return st
