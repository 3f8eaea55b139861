"""CPU: the size thresholds tests/test_hip_sizes.py derives its launch sizes from still read so in the kernels' source, so a change to one
of them cannot leave those tests on the near side of the threshold they are meant to cross."""
import os
import re

import pytest

import test_hip_sizes as T

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")


@pytest.mark.parametrize("name", sorted(T.TABLE))
def test_size_table_matches_the_source(name):
    value, path, pattern = T.TABLE[name]
    with open(os.path.join(ROOT, path)) as f:
        found = re.findall(pattern, f.read())
    assert found, f"{name}: {pattern!r} matches no line of {path}: the table in tests/test_hip_sizes.py is stale"
    for groups in found:                                        # (a launch written twice, e.g. march.hip's two entry points: every copy)
        product = 1
        for g in (groups if isinstance(groups, tuple) else (groups,)):
            product *= int(g)
        assert product == value, f"{name}: {path} now says {product}, the table {value}"


def test_multi_person_renderer_merges_three_actors_in_one_kernel():
    """render_multi_rays' one-kernel merge takes the background and MAX_MERGE_LISTS - 1 actors; more go list by list"""
    with open(os.path.join(ROOT, "ml-neuman_amd", "neuman_hip", "render_utils.py")) as f:
        src = f.read()
    n = T.C.MAX_MERGE_LISTS - 1
    assert f"if len(lists) <= {n}:" in src and f"len(human_nets) <= {n} and MULTI_COMPACT" in src
