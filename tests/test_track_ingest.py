"""The obstacle tracks' device-memory source (include/pmaf.h "obstacle tracks from device memory",
pmaf_set_obstacle_tracks_device) without a device: the symbol is declared, exported and bound; the new kernels' resource
record shows no scratch; the binding refuses what it cannot hand over in front of the C call; the reference of
tests/track_ingest_reference.py is told apart from every mutant of the rule by the committed cases, and the committed
inputs themselves pass the validation -- so that no case of tests/test_track_ingest_gpu.py is refused by accident."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import conftest
import track_ingest_reference as tref


def test_symbol_is_declared_exported_and_bound(pmaf, hip_lib):
    hdr = open(os.path.join(conftest.ROOT, "include", "pmaf.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert re.search(r"\bint\s+pmaf_set_obstacle_tracks_device\s*\(", hdr)
    assert re.search(r"#define\s+PMAF_TRACK_F64\s+0\b", hdr) and re.search(r"#define\s+PMAF_TRACK_F32\s+1\b", hdr)
    assert hasattr(C.CDLL(pmaf.LIB_PATH), "pmaf_set_obstacle_tracks_device")
    assert "pmaf_set_obstacle_tracks_device" in pmaf.SYMBOLS
    assert len(pmaf.SYMBOLS["pmaf_set_obstacle_tracks_device"][1]) == 7
    assert callable(getattr(pmaf.PmafPlanner, "set_obstacle_tracks_device"))
    assert (pmaf.PmafPlanner.TRACK_F64, pmaf.PmafPlanner.TRACK_F32) == (0, 1)
    assert hip_lib.pmaf_abi_version() == 7
    fac = open(os.path.join(conftest.ROOT, "include", "bimanual_planning_ros", "cf_manager.h")).read()
    assert "void setObstacleTracksDevice(const void *d_tracks, int len, int components, int dtype" in fac


def test_ftingest_kernels_use_no_scratch(pmaf, hip_lib):
    path = os.path.join(os.path.dirname(os.path.abspath(pmaf.LIB_PATH)), "resource_usage.txt")
    blocks = re.split(r"(?=Function Name: )", open(path).read())
    mine = [b for b in blocks if re.match(r"Function Name: _Z\d+k_ftingest_(check|store)", b)]
    # two kernels x (double | float) x (6 | 3 components)
    assert len(mine) == 8, [b.splitlines()[0] for b in mine]
    for b in mine:
        assert re.search(r"ScratchSize \[bytes/lane\]: 0\b", b), b
        assert re.search(r"VGPRs Spill: 0\b", b), b
        assert re.search(r"LDS Size \[bytes/block\]: 0\b", b), b
        assert int(re.search(r"Occupancy \[waves/SIMD\]: (\d+)", b).group(1)) >= 2, b
    # the names collide with none of the substrings the other modules look their kernels up by
    for other in ("k_select_audit", "k_track_from_best", "k_rollout_w64_ftrack", "k_audit_track", "k_fcouple_"):
        assert not any(other in b.splitlines()[0] for b in mine)


def test_existing_kernel_objects_disassemble_to_the_parents(pmaf, hip_lib):
    """Where both builds are at hand: PMAF_PARENT_OBJ names the object directory of a build of the PARENT commit
    (`PMAF_OUT=<dir> bash csrc/build.sh` in a checkout of it gives <dir>/obj). Every kernel object both builds have is
    disassembled and compared (tools/disasm_diff.sh); the new unit's object exists on this side only."""
    parent = os.environ.get("PMAF_PARENT_OBJ")
    if not parent:
        pytest.skip("PMAF_PARENT_OBJ is not set: no build of the parent commit to compare with")
    import subprocess
    mine = os.path.join(os.path.dirname(os.path.abspath(pmaf.LIB_PATH)), "obj")
    assert os.path.isdir(parent) and os.path.exists(os.path.join(mine, "ftingest.o"))
    assert not os.path.exists(os.path.join(parent, "ftingest.o")), "PMAF_PARENT_OBJ is not a build of the parent"
    out = subprocess.run(["bash", os.path.join(conftest.ROOT, "tools", "disasm_diff.sh"), parent, mine], capture_output=True,
                         check=True).stdout.decode().strip().split("\n")
    print("\n".join(out))
    assert len(out) >= 23, out
    assert all(line.endswith(": identical") for line in out), [line for line in out if not line.endswith(": identical")]


class _Tensor:
    """what the binding duck-types: data_ptr(), dtype, shape, is_contiguous()"""

    def __init__(self, shape, dtype="torch.float64", contiguous=True):
        self.shape, self.dtype, self._c = shape, dtype, contiguous

    def data_ptr(self):
        return 4096

    def is_contiguous(self):
        return self._c


def test_binding_refuses_in_front_of_the_c_call(pmaf):
    """no handle, no library call: the instance below has no C side at all, so reaching it would raise AttributeError"""
    pl = pmaf.PmafPlanner.__new__(pmaf.PmafPlanner)
    pl.P, pl.n_obs = 2, 4
    ok = (2, 5, 3, 6)
    with pytest.raises(AttributeError):      # (a tensor that passes does reach the C call)
        pl.set_obstacle_tracks_device(_Tensor(ok))
    for t, kw in ((_Tensor(ok, contiguous=False), {}), (_Tensor(ok, dtype="torch.float16"), {}),
                  (_Tensor(ok, dtype="torch.int64"), {}), (_Tensor((2, 5, 4, 6)), {}), (_Tensor((2, 5, 3, 4)), {}),
                  (_Tensor((3, 5, 3, 6)), {}), (_Tensor((5, 3, 6)), {}), (_Tensor((2, 0, 3, 6)), {}),
                  (_Tensor(ok), dict(components=3)), (_Tensor(ok), dict(dtype="float32")), (_Tensor(ok), dict(max_len=4)),
                  (4096, {}), (4096, dict(dtype="float64", max_len=5)), (4096.0, dict(dtype="float64", max_len=5, components=6)),
                  (4096, dict(dtype="bfloat16", max_len=5, components=6)),
                  # ("float" is float64 to NumPy and float32 to C: neither is guessed)
                  (4096, dict(dtype="float", max_len=5, components=6)), (4096, dict(dtype="double", max_len=5, components=6))):
        with pytest.raises(ValueError):
            pl.set_obstacle_tracks_device(t, **kw)
    pl.P = 1
    with pytest.raises(AttributeError):      # a single population's [L][M][c]
        pl.set_obstacle_tracks_device(_Tensor((5, 3, 3), dtype=np.dtype("float32")))
    # the tensor is duck-typed: the package still does not import torch
    assert not re.search(r"^\s*(import|from)\s+torch\b", open(pmaf.planner.__file__).read(), flags=re.M)


def _sources():
    for shape in tref.PARITY_SHAPES:
        for dtype, c in tref.PAIRS:
            yield shape, dtype, c, tref.parity_source(shape, dtype, c)


def test_identities_of_the_rule():
    for shape, dtype, c, s in _sources():
        t = tref.expected_tracks(s, c, tref.DT)
        assert t.dtype == np.float64 and t.shape == s.shape[:2] + (6,)
        np.testing.assert_array_equal(t[:, :, :c], s.astype(np.float64))          # verbatim, widened exactly
        assert (t[:, :, :c].astype(s.dtype) == s).all()
        if c == 3:
            x = s.astype(np.float64)
            np.testing.assert_array_equal(t[:-1, :, 3:6], (x[1:] - x[:-1]) / np.float64(tref.DT))
            assert not t[-1, :, 3:6].any() and not np.signbit(t[-1, :, 3:6]).any()
    one = tref.expected_tracks(np.full((1, 2, 3), 0.25, dtype=np.float32), 3, tref.DT)
    assert not one[0, :, 3:6].any() and not np.signbit(one[0, :, 3:6]).any()
    # F64 / 6 keeps the bit pattern, -0.0 included
    s = tref.parity_source("M3-cap9", "f64", 6)
    s[0, 0, 0], s[1, 1, 1], s[2, 2, 2] = -0.0, 2.0 ** -100, -2.0 ** 100
    assert tref.expected_tracks(s, 6, tref.DT).tobytes() == s.tobytes()
    assert tref.first_offender(s[None], [len(s)], 6, tref.DT) is None


def test_the_committed_inputs_pass_validation():
    """positions inside [-1, 1] m at the scenes' dt: every value and every derived velocity is inside the range"""
    for shape, dtype, c, s in _sources():
        assert np.abs(s[:, :, 0:3]).max() <= 1.0
        assert tref.first_offender(s[None], [len(s)], c, tref.DT) is None, (shape, dtype, c)
        assert tref.in_range(tref.expected_tracks(s, c, tref.DT)).all()
    for dtype, c in tref.PAIRS:
        s = tref.validation_source(dtype, c)
        assert tref.first_offender(s, tref.VALID_LEN, c, tref.DT) is None
        assert not tref.in_range(s[0, tref.VALID_LEN[0]:]).any()                    # the padding would not pass


def test_validation_cases_name_the_element():
    cases = tref.validation_cases()
    assert len(cases) == (4 + 4 + 5 + 5) * 4 + 2 * 4
    for dtype, c, vname, pname, s, want in cases:
        assert s.dtype == tref.DTYPES[dtype]
        assert tref.first_offender(s, tref.VALID_LEN, c, tref.DT) == want, (dtype, c, vname, pname)
        p, k = want[0], want[1]
        assert k < tref.VALID_LEN[p]
    for dtype, c in tref.PAIRS:
        s, want = tref.two_bad(dtype, c)
        assert tref.first_offender(s, tref.VALID_LEN, c, tref.DT) == want
    # an F32 subnormal is a number, not a zero, and lies below 2^-100
    v = np.float32(tref.BAD_VALUES["f32-subnormal"][0])
    assert v != 0 and float(v) < tref.LO and float(v) == tref.BAD_VALUES["f32-subnormal"][0]


@pytest.mark.parametrize("mutant", tref.MUTANTS)
def test_cases_tell_every_mutant_from_the_rule(mutant):
    hit = 0
    for shape, dtype, c, s in _sources():
        a, b = tref.expected_tracks(s, c, tref.DT), tref.expected_tracks(s, c, tref.DT, mutant=mutant)
        hit += a.tobytes() != b.tobytes()
    for dtype, c in tref.PAIRS:
        s = tref.validation_source(dtype, c)
        hit += tref.first_offender(s, tref.VALID_LEN, c, tref.DT) != tref.first_offender(s, tref.VALID_LEN, c, tref.DT, mutant=mutant)
        s, want = tref.two_bad(dtype, c)
        hit += tref.first_offender(s, tref.VALID_LEN, c, tref.DT, mutant=mutant) != want
    print(mutant, hit)
    assert hit >= 1, mutant
    if mutant in ("backward", "lastvel", "recip"):     # on every F64 / 3 parity source
        for shape, dtype, c, s in _sources():
            if (dtype, c) == ("f64", 3):
                assert tref.expected_tracks(s, c, tref.DT).tobytes() != tref.expected_tracks(s, c, tref.DT, mutant=mutant).tobytes(), shape
    if mutant == "f32diff":
        for shape, dtype, c, s in _sources():
            if (dtype, c) == ("f32", 3):
                assert tref.expected_tracks(s, c, tref.DT).tobytes() != tref.expected_tracks(s, c, tref.DT, mutant=mutant).tobytes(), shape
