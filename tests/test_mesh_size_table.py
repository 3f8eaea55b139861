"""CPU: the size thresholds tests/test_hip_mesh_sizes.py derives its shapes from (tests/helpers/mesh_sizes.py) still read so in the kernels'
source, and every derived shape lies on the far side of its threshold -- so a change to one of the constants cannot leave those tests on the
near side of what they are meant to cross."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import mesh_sizes as MS  # noqa: E402

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")


@pytest.mark.parametrize("name", sorted(MS.TABLE))
def test_size_table_matches_the_source(name):
    value, path, pattern = MS.TABLE[name]
    with open(os.path.join(ROOT, path)) as f:
        found = re.findall(pattern, f.read())
    assert found, f"{name}: {pattern!r} matches no line of {path}: the table in tests/helpers/mesh_sizes.py is stale"
    for groups in found:                                        # (a launch written twice: every copy)
        product = 1
        for g in (groups if isinstance(groups, tuple) else (groups,)):
            product *= int(g)
        assert product == value, f"{name}: {path} now says {product}, the table {value}"


def test_the_scan_kernels_and_their_launches_agree():
    """the kernels hard-code their workgroup size (part[256], part[1024], kThreads): the launches must use that size"""
    C = MS.C
    assert C.SCAN_THREADS == C.SCAN_THREADS_RASTER == C.SCAN_THREADS_SILHOUETTE
    assert C.BATCH_SCAN_THREADS == C.BATCH_SCAN_PER == C.BATCH_CAMERA_STRIDE
    assert C.ISO_SPAN == 8 * C.ISO_THREADS                      # (isosurface.hip asserts this itself: a thread of the span kernel takes one word)


def test_every_derived_shape_is_past_its_threshold():
    C = MS.C
    # a, b: tiles per image against raster_scan_kernel's SCAN_THREADS
    want = {'one_tile_over_4112x16': (4112, 16, 257, 2), 'three_per_thread_528x256': (528, 256, 528, 3), 'square_272x272': (272, 272, 289, 2)}
    for name, (W, H, T, per) in want.items():
        _, w, h, shift = MS.RASTER_CASES[name]
        assert (w, h, shift) == (W, H, (0, 0)) and MS.tiles(w, h) == T > C.SCAN_THREADS and MS.per_thread(T, C.SCAN_THREADS) == per, name
    for name, (_, w, h, _) in MS.RASTER_CASES.items():
        assert MS.tiles(w, h) > C.SCAN_THREADS and MS.per_thread(MS.tiles(w, h), C.SCAN_THREADS) >= 2, name
    T = MS.tiles(*MS.RASTER_CASES['one_tile_over_4112x16'][1:3])
    assert T % 2 == 1 and (T - 1) // 2 < C.SCAN_THREADS - 1     # the last busy thread holds one tile, threads past it hold none
    assert set(MS.SILHOUETTE_CASES) <= set(MS.RASTER_CASES) and set(MS.REACHES_PAST_THE_THREAD_COUNT) <= set(MS.RASTER_CASES)
    # c: one handle from below the threshold to beyond it and back
    assert MS.SMALL_IMAGE == (96, 64) and MS.tiles(*MS.SMALL_IMAGE) < C.SCAN_THREADS < MS.tiles(*MS.BIG_IMAGE) and MS.BIG_IMAGE == (528, 256)
    # d: B T against sil_scan_batch_kernel's BATCH_SCAN_THREADS, B against its camera loop's stride
    n = MS.BATCH_FRAMES * MS.tiles(MS.BATCH_SIDE, MS.BATCH_SIDE)
    assert (MS.BATCH_FRAMES, MS.BATCH_SIDE, n) == (5, 240, 1125) and n > C.BATCH_SCAN_THREADS and MS.per_thread(n, C.BATCH_SCAN_THREADS) == 2
    assert MS.MANY_FRAMES == 1030 > C.BATCH_CAMERA_STRIDE and MS.per_thread(MS.MANY_FRAMES * MS.tiles(C.TILE, C.TILE), C.BATCH_SCAN_THREADS) == 2
    assert MS.MANY_CHECKED == (0, 1023, 1024, 1029) and MS.MANY_BAD == 1027
    assert C.BATCH_CAMERA_STRIDE <= MS.MANY_BAD < MS.MANY_FRAMES - 1 and MS.MANY_BAD not in MS.MANY_CHECKED      # only the second pass sees it
    # e: spans per grid against iso_scan_kernel's ISO_THREADS
    want = {'two_per_thread_131x67x63': ((131, 67, 63), 270, 2), 'three_per_thread_97x81x135': ((97, 81, 135), 518, 3)}
    for name, (dims, s, per) in want.items():
        assert MS.ISO_CASES[name][0] == dims and MS.spans(dims) == s > C.ISO_THREADS and MS.per_thread(s, C.ISO_THREADS) == per, name
    assert MS.PRODUCTION_MESH in MS.ISO_CASES
    # f: V against the cluster table
    V = MS.V_TABLE_FULL
    assert V == 32768 and (V + C.CLUSTER - 1) // C.CLUSTER == C.MAX_CLUSTERS < (V + 1 + C.CLUSTER - 1) // C.CLUSTER
    assert MS.N_RAYS == 320


def test_the_images_cover_tiles_that_many_scan_threads_own():
    """From the float64 helper: in every image the body covers tiles owned by at least three raster_scan_kernel threads (a wrong partial sum
    moves the lists of every later tile, so a wrong offset must show), and in the listed images it reaches tiles with index >= SCAN_THREADS.
    In the two centred images it cannot (tiles 59-221 of 257 and 89-237 of 289): the two views with a moved principal point are there for that."""
    import raster_ref as RR
    from neuman_hip import synthetic
    spans = {}
    for name, (shape, W, H, shift) in MS.RASTER_CASES.items():
        verts, faces = synthetic.capsule_mesh(*shape)
        r = RR.rasterize(verts, faces, RR.camera_of(MS.capture(W, H, shift)), np.float64, analyse=True)
        covered = r['face_id'] >= 0
        t, threads = MS.tile_census(covered, W, H)
        spans[name] = (int(t.min()), int(t.max()))
        assert len(threads) >= 3, name
        assert int(r['ambiguous'].sum()) <= 0.01 * int(covered.sum()), name      # the cap of tests/test_hip_raster.py holds for the helper alone
        if name in MS.REACHES_PAST_THE_THREAD_COUNT:
            assert t.max() >= MS.C.SCAN_THREADS, name
    assert spans['one_tile_over_4112x16'] == (59, 221) and spans['three_per_thread_528x256'] == (74, 527) and spans['square_272x272'] == (89, 237)
    assert spans['one_tile_over_4112x16_at_the_right_end'][1] == MS.tiles(*MS.RASTER_CASES['one_tile_over_4112x16'][1:3]) - 1      # the very last tile


def test_the_cloud_at_the_cluster_tables_end():
    """V = 32 768 exactly, sorted along the body; and the seeds are such that the oracle's float64 and float32 evaluations agree on every
    ray's hit decision, so that no ray of the GPU test needs excluding (rays that hit and rays that miss both occur)"""
    from oracle import ray_ops as O
    v = MS.body_cloud()
    assert v.shape == (MS.V_TABLE_FULL, 3) and v.dtype == np.float32
    key = v[:, 1] * 7 + v[:, 0]
    assert (np.diff(key) >= 0).all()
    o, d = MS.rays_at(v, MS.CLOUD_RAY_SEED)
    assert o.shape == d.shape == (MS.N_RAYS, 3) and np.abs(np.linalg.norm(d.astype(np.float64), axis=1) - 1).max() < 1e-6
    n64, f64 = O.geometry_guided_near_far(o, d, v, MS.NEAR_FAR_TAU, chunk=32, dtype=np.float64)
    n32, f32 = O.geometry_guided_near_far(o, d, v, MS.NEAR_FAR_TAU, chunk=32)
    hit = n64 < f64
    assert 0.2 < hit.mean() < 0.95 and not ((n32 < f32) != hit).any()
