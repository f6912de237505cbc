"""Reference of the obstacle tracks' device-memory source (include/pmaf.h "obstacle tracks from device memory",
pmaf_set_obstacle_tracks_device) at tolerance 0, in NumPy: widening float32 to float64 is exact, and x[1:] - x[:-1] and
/ dt on float64 arrays are single correctly rounded operations. The cases tests/test_track_ingest.py (CPU) and
tests/test_track_ingest_gpu.py (device) share are here too, with the mutants of the rule that the CPU suite tells apart
from it on exactly these cases.

Test infrastructure: imports neither the package nor the oracle."""
import numpy as np

MUTANTS = ("backward", "lastvel", "f32diff", "recip", "padding", "swapped", "largest")
LO, HI = 2.0 ** -100, 2.0 ** 100
DTYPES = {"f64": np.float64, "f32": np.float32}
PAIRS = (("f64", 6), ("f64", 3), ("f32", 6), ("f32", 3))


def in_range(x):
    """check_range's rule, elementwise"""
    a = np.abs(np.asarray(x, dtype=np.float64))
    with np.errstate(invalid="ignore"):
        return np.isfinite(a) & ((a == 0.0) | ((a >= LO) & (a <= HI)))


def _velocities(x, src, dt, mutant):
    """[L][M][3]: forward difference over dt, +0.0 at the last point; x the widened positions, src as given"""
    L = len(x)
    v = np.zeros_like(x)
    if L < 2:
        if mutant == "lastvel" and L:
            v[-1] = 1.0
        return v
    with np.errstate(all="ignore"):
        if mutant == "f32diff" and src.dtype == np.float32:
            d = (src[1:] - src[:-1]).astype(np.float64)
        else:
            d = x[1:] - x[:-1]
        q = d * (np.float64(1.0) / np.float64(dt)) if mutant == "recip" else d / np.float64(dt)
    if mutant == "backward":
        v[1:] = q
    else:
        v[:-1] = q
    if mutant == "lastvel":
        v[-1] = v[-2]
    return v


def expected_tracks(src, components, dt, mutant=None):
    """what pmaf_get_obstacle_tracks returns after ingesting src [L][M][components] (float64 or float32): [L][M][6]"""
    src = np.asarray(src)
    assert src.dtype in (np.float32, np.float64) and src.ndim == 3 and src.shape[2] == components
    L, M, c = src.shape
    if mutant == "swapped":
        src = np.ascontiguousarray(src.reshape(L, c, M).transpose(0, 2, 1))
    x = src.astype(np.float64)
    if components == 6:
        return x.copy()
    out = np.zeros((L, M, 6))
    out[:, :, 0:3] = x
    out[:, :, 3:6] = _velocities(x, src, dt, mutant)
    return out


def first_offender(src, lengths, components, dt, mutant=None):
    """src [P][max_len][M][components], lengths [P]: None when every ingested value passes, else (population, point,
    obstacle, component) of the first offender: the smallest flat index of [P][max_len][M][6], components 3 .. 5 the
    velocities. A derived velocity is judged only where both positions it is taken from pass themselves."""
    src = np.asarray(src)
    P, max_len, M, c = src.shape
    bad = []
    for p in range(P):
        L = max_len if mutant == "padding" else int(lengths[p])
        s = src[p, :L]
        t = expected_tracks(s, components, dt)
        ok = in_range(t)
        if components == 3 and L > 1:
            both = ok[:-1, :, 0:3] & ok[1:, :, 0:3]
            ok[:-1, :, 3:6] |= ~both
        for k, i, cc in np.argwhere(~ok):
            bad.append((p, int(k), int(i), int(cc)))
    if not bad:
        return None
    return max(bad) if mutant == "largest" else min(bad)


def make_source(M, L, components, dtype, seed=0, dt=0.01):
    """valid tracks [L][M][components] of `dtype` ("f64" / "f32"): positions inside [-1, 1] m that drift by up to 2 mm
    per point (differences with full mantissas: the reciprocal multiply differs from the division in about an eighth
    of them), velocities inside [-0.5, 0.5] m/s. Every fourth point's z jumps across the origin: two float32 neighbours
    that are close subtract exactly in float32, these do not -- which is what tells a difference taken before the
    widening from one taken after it."""
    rng = np.random.default_rng(1000 * seed + 7 * M + L + components)
    x = rng.uniform(-0.8, 0.8, (1, M, 3)) + np.cumsum(rng.uniform(-2e-3, 2e-3, (L, M, 3)), axis=0)
    x[1::4, :, 2] = 0.11 - 0.37 * x[1::4, :, 2]
    out = np.concatenate([x, rng.uniform(-0.5, 0.5, (L, M, 3))], axis=2) if components == 6 else x
    return np.ascontiguousarray(out.astype(DTYPES[dtype]))


# ---- the cases both suites run ----
# parity: name -> (M, cap); the scene is sentinel_track_reference.build_scene(name) except for M = 1
PARITY_SHAPES = {"M3-cap9": (3, 9), "M59-cap70-moving": (59, 70), "M60-cap70": (60, 70), "M1-cap9": (1, 9)}
DT = 0.01          # every scene's rollout step (the suites assert it)


def parity_source(shape, dtype, components):
    M, cap = PARITY_SHAPES[shape]
    return make_source(M, cap, components, dtype, seed=1)


# the bad values of the validation cases: name -> (value, the dtypes it is placed in)
BAD_VALUES = {
    "nan": (np.nan, ("f64", "f32")),
    "inf": (np.inf, ("f64", "f32")),
    "2^101": (2.0 ** 101, ("f64", "f32")),
    "2^-101": (2.0 ** -101, ("f64", "f32")),
    "f32-subnormal": (float(np.float32(1e-40)), ("f32",)),
}
VALID_M, VALID_L, VALID_MAX = 5, 6, 8      # the validation cases' tracks: P = 2, len (6, 4), max_len 8
VALID_LEN = (VALID_L, 4)


def validation_source(dtype, components):
    """[2][VALID_MAX][M][c], valid inside the lengths; NaN and 1e35 in the padding (never read)"""
    s = np.stack([make_source(VALID_M, VALID_MAX, components, dtype, seed=2 + p) for p in range(2)])
    for p, L in enumerate(VALID_LEN):
        s[p, L:] = np.nan
        s[p, L:, 0] = 1e35
    return s


def validation_places(components):
    """name -> (population, point, obstacle, component) of the element a bad value is placed at"""
    c = components
    return {"first": (0, 0, 0, 0), "last-read": (1, VALID_LEN[1] - 1, VALID_M - 1, c - 1),
            "last-obstacle": (0, 2, VALID_M - 1, c - 1), "middle": (0, 3, 2, 1)}


def validation_cases():
    """(dtype, components, value name, place name, bad source, expected offender)"""
    out = []
    for dtype, c in PAIRS:
        for vname, (val, dts) in BAD_VALUES.items():
            if dtype not in dts:
                continue
            for pname, at in validation_places(c).items():
                s = validation_source(dtype, c)
                s[at] = val
                out.append((dtype, c, vname, pname, s, at))
        if c == 3:
            # two positions whose difference over dt leaves the range: the velocity at the first of them
            for pname, at in validation_places(c).items():
                p, k, i, cc = at
                k = min(k, VALID_LEN[p] - 2)
                s = validation_source(dtype, c)
                s[p, k, i, cc], s[p, k + 1, i, cc] = -2.0 ** 99, 2.0 ** 99
                # (the point before k differs from -2^99 by 2^99 + ..., over dt out of range too, where there is one)
                want = (p, k - 1, i, 3 + cc) if k > 0 else (p, k, i, 3 + cc)
                out.append((dtype, c, "difference", pname, s, want))
    return out


def two_bad(dtype, components):
    """two offenders: the later one in population 0, the earlier one ... also in population 0 at an earlier point"""
    s = validation_source(dtype, components)
    s[0, 4, 1, 2] = np.inf
    s[0, 1, 3, 0] = np.nan
    s[1, 0, 0, 0] = np.nan
    return s, (0, 1, 3, 0)
