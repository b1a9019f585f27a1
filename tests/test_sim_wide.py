"""Similarity sweep beyond the old native limits, host side: alphabets wider
than 255 characters (16-bit symbol ids, character-exact), values longer than
the GPU kernel takes, the route policy and the ``--check`` warnings.

All comparisons use ``LevenshteinSimilarityFn(5.0, 10.0)``: its inclusion
edge ``3d == la + lb`` has ``unit`` exactly 0.5 in fp32 and fp64, so every
implementation excludes an edge pair identically.
"""

from types import SimpleNamespace

import numpy as np
import pytest

from dblink_amd import ops
from dblink_amd.models.attribute_index import _python_sim_pairs
from dblink_amd.models.similarity import LevenshteinSimilarityFn

FN = LevenshteinSimilarityFn(5.0, 10.0)

needs_native = pytest.mark.skipif(not ops.have_native(),
                                  reason="native extension not built")


def _assert_matches_oracle(values):
    native = ops.sim_pairs(values, FN)
    ref = _python_sim_pairs(values, FN)
    np.testing.assert_array_equal(native.row_ptr, ref.row_ptr)
    np.testing.assert_array_equal(native.col, ref.col)
    np.testing.assert_allclose(native.expsim, ref.expsim, rtol=1e-6)
    return ref


@needs_native
def test_wide_alphabet_native_matches_oracle():
    """> 255 distinct CJK characters: the native pass is character-level,
    not UTF-8-byte-level (one differing character is d = 1 whatever its
    encoded width)."""
    wide = ["".join(chr(0x4E00 + 7 * i + j) for j in range(3)) for i in range(300)]
    # near-duplicates: one character of a base value replaced, at each position
    near = [wide[10][:2] + chr(0x9000), chr(0x9001) + wide[10][1:],
            wide[200][0] + chr(0x9002) + wide[200][2], wide[250][:2] + wide[3][0]]
    values = sorted(set(wide) | set(near) | {"ANNA", "ANNE", "ANNAH", "BOB", "BORB"})
    assert len({ch for v in values for ch in v}) > 255
    ref = _assert_matches_oracle(values)
    # the near-duplicates really are in the index (the check is not vacuous)
    i, j = values.index(wide[10]), values.index(near[0])
    assert j in ref.col[ref.row_ptr[i]:ref.row_ptr[i + 1]]


@needs_native
def test_long_values_cpu_pass_matches_oracle():
    """Values up to 300 characters stay on the OpenMP pass and stay exact."""
    rng = np.random.default_rng(5)
    master = "".join(rng.choice(list("abcd"), size=300))
    values = [master, master[1:], master[:257], master[:256], master[20:220],
              master[:130], master[:65], master[:64], master[:10], "abc",
              master[:150] + "x" + master[151:], ""]
    values = sorted(set(values))
    assert len(values) <= 12 and max(map(len, values)) == 300
    assert ops.sim_pairs_route(len(values), 300, 5, True) == "cpu"
    ref = _assert_matches_oracle(values)
    assert ref.col.size > len(values)  # off-diagonal pairs exist


def test_route_policy(monkeypatch):
    monkeypatch.delenv("DBLINK_SIM_GPU_MIN_V", raising=False)
    route = ops.sim_pairs_route
    assert route(10**4, 200, 100, True) == "gpu"
    assert route(10**4, 256, 100, True) == "gpu"
    assert route(10**4, 257, 100, True) == "cpu"
    assert route(10**4, 40, 300, True) == "gpu"
    assert route(10**4, 40, 65535, True) == "gpu"
    assert route(10**4, 40, 70000, True) == "python"
    assert route(10**4, 40, 70000, False) == "python"
    assert route(10**4, 200, 100, False) == "cpu"
    # minimum-V cutoff: 8192 by default, lowered by the env knob
    assert route(8192, 40, 100, True) == "cpu"
    assert route(8193, 40, 100, True) == "gpu"
    assert route(24, 40, 100, True) == "cpu"
    monkeypatch.setenv("DBLINK_SIM_GPU_MIN_V", "0")
    assert route(24, 40, 100, True) == "gpu"
    assert route(24, 257, 100, True) == "cpu"
    assert route(24, 40, 100, False) == "cpu"


def _limit_warnings(values):
    from dblink_amd.api.project import native_limit_problems

    attr = SimpleNamespace(name="addr", is_constant=False)
    project = SimpleNamespace(matching_attributes=[attr])
    table = SimpleNamespace(columns=[np.array(values, dtype=object)])
    errors, warnings = native_limit_problems(project, table)
    assert errors == []
    return warnings


def test_check_warnings_follow_the_new_limits():
    alphabet300 = [chr(0x4E00 + i) for i in range(300)]
    assert _limit_warnings(["".join(alphabet300[i:i + 3]) for i in range(0, 300, 3)]) == []
    assert _limit_warnings(["a" * 100, "b" * 64, "c"]) == []
    assert _limit_warnings(["a" * 256]) == []
    warns = _limit_warnings(["a" * 300, "b"])
    assert len(warns) == 1 and "300" in warns[0] and "256" in warns[0]
    # 70000 distinct characters (surrogates skipped): pure-Python fallback
    chars = [chr(c) for c in range(0x20, 0x20 + 72100) if not 0xD800 <= c < 0xE000]
    assert len(chars) > 65535
    warns = _limit_warnings(["".join(chars[i:i + 100]) for i in range(0, len(chars), 100)])
    assert len(warns) == 1 and "65535" in warns[0]
