"""Without a device: what the mesh clean-up, the mesh smoothing and the mesh simplification share stands once, in
ml-neuman_amd/csrc/mesh_device.h -- the sizes of a launch, the wave scan of the ranking, the in-place sort of a segment and the host's table
of remembered workspaces -- and none of the three files carries a copy of its own again."""
import os
import re

import pytest

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "ml-neuman_amd", "csrc")
FILES = ("mesh_components.hip", "mesh_smooth.hip", "mesh_simplify.hip")
COPIES = ("__shfl_up", "std::mutex", "constexpr int kSpan", "constexpr int kThreads", "constexpr int kSortInThread")
SORT_DEFINITION = r"\bvoid\s+sort_segment\s*\("


def source(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


@pytest.mark.parametrize("name", FILES)
def test_a_mesh_file_includes_the_header_and_keeps_no_copy(name):
    src = source(name)
    assert re.search(r'^#include "mesh_device\.h"$', src, re.M), f"{name} does not include mesh_device.h"
    for text in COPIES:
        assert text not in src, f"{name} has {text!r} of its own: it belongs to mesh_device.h"
    assert not re.search(SORT_DEFINITION, src), f"{name} defines a sort_segment of its own"


def test_the_header_holds_each_shared_piece_once():
    src = source("mesh_device.h")
    assert "#pragma once" in src and re.search(r"^namespace \w+ \{$", src, re.M)
    assert len(re.findall(SORT_DEFINITION, src)) == 1
    assert src.count("__shfl_up") == 1                                                # the wave scan of span_rank_kernel
    for text in COPIES[2:]:
        assert src.count(text) == 1, text
