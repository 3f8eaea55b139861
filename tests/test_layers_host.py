"""CPU: the layered merge's entries (include/neuman_hip.h: nm_merge_composite_layers, nm_merge_composite_layers_max_samples, nm_layers_to_rgba8) are
declared, bound and exported with matching signatures, validate their arguments before any device work and name the entry that was called, report
a staging limit of at least 2048 merged samples for every list count, and allocate and synchronise nothing."""
import ctypes
import os
import re

import pytest

from neuman_hip import _lib, render_utils

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
NEW = ("nm_merge_composite_layers", "nm_merge_composite_layers_max_samples", "nm_layers_to_rgba8")
P = 0x10000                                                       # a non-null, 16-byte aligned address nothing dereferences: validation comes first


def err():
    return _lib.lib().nm_last_error().decode()


def layers(k, z, raw, S, R=4, rows=None, ptr=P, layer_ptr=P, layer_depth=P):
    arr = ctypes.c_void_p * max(len(z), 1)
    return _lib.lib().nm_merge_composite_layers(k, arr(*z), arr(*raw), None if rows is None else arr(*rows), (ctypes.c_int * max(len(S), 1))(*S), R, ptr, 1,
                                                ptr, ptr, ptr, layer_ptr, layer_depth, layer_ptr, None)


def max_samples(k):
    return _lib.lib().nm_merge_composite_layers_max_samples(k)


def c_params(name, text):
    """the parameter list of `name`'s declaration or definition in C text -> list of parameter strings"""
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)", text)
    assert m, name
    return [p.strip() for p in m.group(1).split(",") if p.strip()]


def test_entries_are_declared_bound_exported_and_their_signatures_agree():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "neuman_hip.h")).read(), flags=re.S)
    csrc = os.path.join(ROOT, "ml-neuman_amd", "csrc")
    defs = open(os.path.join(csrc, "merge_layers.hip")).read() + open(os.path.join(csrc, "frame.hip")).read()
    lib = _lib.lib()
    for name in NEW:
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
        declared = c_params(name, header)
        assert [re.sub(r"\s+", " ", p) for p in declared] == [re.sub(r"\s+", " ", p) for p in c_params(name, defs)], name
        restype, argtypes = _lib.SIGNATURES[name]
        assert restype is ctypes.c_int32 or restype is ctypes.c_int, name
        assert len(argtypes) == len(declared), (name, len(argtypes), declared)
        for p, t in zip(declared, argtypes):                       # pointers bind to pointer types, integers to integers of the declared width
            if "*" in p:
                assert t in (_lib.c_f32p, ctypes.c_void_p, _lib.c_stream) or issubclass(t, ctypes._Pointer), (name, p, t)
            elif p.startswith("int64_t"):
                assert t is ctypes.c_int64, (name, p, t)
            elif p.startswith("nm_stream_t"):
                assert t is _lib.c_stream, (name, p, t)
            else:
                assert p.startswith("int ") and t in (ctypes.c_int32, ctypes.c_int), (name, p, t)
    # the layered merge takes nm_merge_composite_lists_wide's arguments, then the three layer outputs, then the stream
    wide = c_params("nm_merge_composite_lists_wide", header)
    lay = c_params("nm_merge_composite_layers", header)
    assert lay[:len(wide) - 1] == wide[:-1] and lay[-1] == wide[-1]
    assert [p.split("*")[-1].strip() for p in lay[len(wide) - 1:-1]] == ["layer_rgb", "layer_depth", "layer_acc"]


@pytest.mark.parametrize("k", [0, 33, -1])
def test_a_list_count_outside_1_to_32_is_refused(k):
    n = max(k, 1)
    assert layers(k, [P] * n, [P] * n, [4] * n) == -1
    assert "nm_merge_composite_layers" in err() and "32" in err()
    assert max_samples(k) == 0


def test_null_empty_and_misaligned_arguments_are_refused_without_a_device():
    assert layers(2, [P, None], [P, P], [4, 4]) == -1 and "nm_merge_composite_layers: list 1 is null" in err()
    assert layers(2, [P, P], [P, None], [4, 4]) == -1 and "nm_merge_composite_layers: list 1 is null" in err()
    assert layers(3, [P, P, P], [P, P, P], [4, 0, 4]) == -1 and "nm_merge_composite_layers: list 1 is empty" in err()
    assert layers(2, [P, P], [P, P + 8], [4, 4]) == -1 and "nm_merge_composite_layers" in err() and "aligned" in err()
    assert layers(2, [P, P], [P, P], [4, 4], ptr=None) == -1 and "nm_merge_composite_layers: null pointer" in err()
    assert layers(2, [P, P], [P, P], [4, 4], layer_ptr=None) == -1 and "nm_merge_composite_layers: null pointer" in err()
    assert layers(2, [P, P], [P, P], [4, 4], R=-1) == -1 and "nm_merge_composite_layers" in err()
    lib = _lib.lib()
    assert lib.nm_merge_composite_layers(2, None, None, None, None, 0, None, 1, None, None, None, None, None, None, None) == -1 and "nm_merge_composite_layers" in err()
    # the empty batch is an ordinary case, with null arrays
    assert layers(2, [None, None], [None, None], [4, 4], R=0, ptr=None, layer_ptr=None, layer_depth=None) == 0
    assert lib.nm_layers_to_rgba8(None, None, 4, None, None) == -1 and "nm_layers_to_rgba8: null pointer" in err()
    assert lib.nm_layers_to_rgba8(P, P, -1, P, None) == -1 and "nm_layers_to_rgba8" in err()
    assert lib.nm_layers_to_rgba8(P, P, 4, P + 2, None) == -1 and "nm_layers_to_rgba8" in err() and "aligned" in err()
    assert lib.nm_layers_to_rgba8(None, None, 0, None, None) == 0


@pytest.mark.parametrize("k", [1, 4, 5, 32])
def test_the_staging_limit_is_reported_is_at_least_2048_and_one_sample_more_is_refused(k):
    """the limit is checked before the empty batch returns, so it is exercised without a device"""
    M = max_samples(k)
    assert M >= 2048
    assert M <= render_utils.WIDE_MERGE_MAX_SAMPLES               # (the layered merge stages what the wide merge stages, never more)
    sizes = [M // k] * k
    sizes[0] += M - sum(sizes)
    assert layers(k, [None] * k, [None] * k, sizes, R=0) == 0
    sizes[-1] += 1
    assert layers(k, [None] * k, [None] * k, sizes, R=0) == -1
    assert "nm_merge_composite_layers" in err() and str(M) in err() and str(M + 1) in err()
    assert layers(k, [P] * k, [P] * k, sizes) == -1 and "nm_merge_composite_layers" in err()        # refused with rays as well: nothing is launched


def test_the_kernel_file_allocates_and_synchronises_nothing():
    src = open(os.path.join(ROOT, "ml-neuman_amd", "csrc", "merge_layers.hip")).read() + open(os.path.join(ROOT, "ml-neuman_amd", "csrc", "merge_wide_device.h")).read()
    for word in ("hipMalloc", "hipStreamSynchronize", "hipDeviceSynchronize", "hipMemcpy("):
        assert word not in src, word
    assert "atomic" not in src.lower().replace("no atomics", "")   # the layer sums are deterministic: no floating-point atomics


def test_host_mirror_has_the_new_names_and_install_is_unchanged():
    import inspect
    import neuman_hip
    for name in ("merge_composite_layers", "render_hybrid_layers_rays", "render_multi_layers_rays", "render_hybrid_nerf_layers",
                 "render_hybrid_nerf_multi_persons_layers", "layers_to_rgba_uint8", "compose_over"):
        assert callable(getattr(render_utils, name)), name
    for core, layered in (("render_hybrid_rays", "render_hybrid_layers_rays"), ("render_multi_rays", "render_multi_layers_rays")):
        assert list(inspect.signature(getattr(render_utils, core)).parameters) == list(inspect.signature(getattr(render_utils, layered)).parameters)
    for ref, layered in (("render_hybrid_nerf", "render_hybrid_nerf_layers"), ("render_hybrid_nerf_multi_persons", "render_hybrid_nerf_multi_persons_layers")):
        a, b = (inspect.signature(getattr(render_utils, n)).parameters for n in (ref, layered))
        assert [p for p in a if p != "return_depth"] == list(b) and all(a[p].default == b[p].default for p in b)
    assert "layers" not in inspect.getsource(neuman_hip.install)   # the reference has no such names: nothing is rebound
    for body in ("_render_hybrid_rays", "_render_multi_rays"):
        assert inspect.signature(getattr(render_utils, body)).parameters["layers"].default is None


def test_compose_over_is_the_stated_sum():
    import torch
    g = torch.Generator().manual_seed(0)
    layer_rgb, layer_acc, image = torch.rand((7, 3, 3), generator=g), torch.rand((7, 3), generator=g) / 3, torch.rand((7, 3), generator=g)
    out = render_utils.compose_over(layer_rgb, layer_acc, image)                                    # default: the actor layers, 1 .. L-1
    assert torch.equal(out, layer_rgb[:, 1:].sum(1) + (1 - layer_acc[:, 1:].sum(1))[:, None] * image)
    out = render_utils.compose_over(layer_rgb, layer_acc, image, layers=[0, 2])
    assert torch.equal(out, layer_rgb[:, [0, 2]].sum(1) + (1 - layer_acc[:, [0, 2]].sum(1))[:, None] * image)
    white = render_utils.compose_over(layer_rgb, layer_acc, torch.ones(3), layers=range(3))
    assert torch.equal(white, layer_rgb.sum(1) + (1 - layer_acc.sum(1))[:, None])
