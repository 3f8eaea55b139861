"""The sizes at which the mesh smoothing kernels (ml-neuman_amd/csrc/mesh_smooth.hip, and the scan and the sort it
takes from csrc/mesh_device.h) change behaviour, and the meshes
tests/test_hip_mesh_smooth.py crosses them with.

TABLE has the form of tests/helpers/mesh_sizes.py's: name -> (value, source file, pattern whose integer groups multiply to the value);
tests/test_mesh_smooth_host.py checks on the CPU that every entry still reads so in the source and that every derived size lies past its
threshold.  Everything here is numpy."""
import types

import numpy as np

CSRC = 'ml-neuman_amd/csrc/'
TABLE = {
    # span_rank_kernel: a workgroup scans kSpan counters, kSpan / kThreads consecutive ones per thread
    'SPAN': (1024, CSRC + 'mesh_device.h', r'constexpr int kSpan = (\d+);'),
    # span_scan_kernel: ONE workgroup of kThreads scans the spans' sums, ceil(spans / kThreads) spans per thread
    'THREADS': (256, CSRC + 'mesh_device.h', r'constexpr int kThreads = (\d+);'),
    # sort_segment: up to kSortInThread entries by insertion, more by heap sort
    'SORT': (32, CSRC + 'mesh_device.h', r'constexpr int kSortInThread = (\d+);'),
}
C = types.SimpleNamespace(**{k: v[0] for k, v in TABLE.items()})
SEED = 31

TWO_SPANS_AND_ONE = 2 * C.SPAN + 1                            # 2049 vertices: three spans, the last holds one counter
GRID_SMALL = (3, 683)                                         # rows x columns = 2049
GRID_PAST_THE_SCAN = (512, 513)                               # 262 656 vertices = 256.5 spans: a scan thread owns two spans
CONE_JUST_PAST = C.SORT + 1                                   # the apex's list: one entry more than the insertion sort takes
CONE_FAR_PAST = 4 * C.SORT                                    # ... and the rim's neighbour lists stay short
CONE_NEIGHBOURS_PAST = C.SORT // 2 + 4                        # 20 faces sorted in-thread, their 40 neighbour ids by the heap sort


def spans(n):
    return (n + C.SPAN - 1) // C.SPAN


def per_thread(n_spans):
    return (n_spans + C.THREADS - 1) // C.THREADS


def grid_mesh(rows, cols, seed=SEED, noise=0.2):
    """a planar grid of rows x cols vertices (row-major), two triangles per cell, counter-clockwise seen from +z, the vertices moved by
    seeded noise of `noise` cells in x, y and z -> (verts [V,3] float32, faces [F,3] int32).  Every face is proper; the rim is the open edge."""
    rng = np.random.default_rng(seed)
    j, i = np.meshgrid(np.arange(rows), np.arange(cols), indexing='ij')
    verts = np.stack([i, j, np.zeros_like(i)], -1).reshape(-1, 3).astype(np.float64)
    verts += rng.uniform(-noise, noise, size=verts.shape)
    r, c = np.meshgrid(np.arange(rows - 1), np.arange(cols - 1), indexing='ij')
    v00 = (r * cols + c).reshape(-1)
    v01, v10, v11 = v00 + 1, v00 + cols, v00 + cols + 1
    faces = np.concatenate([np.stack([v00, v01, v11], 1), np.stack([v00, v11, v10], 1)], 0)
    faces = faces[rng.permutation(faces.shape[0])]            # a vertex's faces are not met in index order
    return verts.astype(np.float32), faces.astype(np.int32)


def grid_rim(rows, cols):
    """bool [V]: the vertices of the grid's open edge"""
    j, i = np.meshgrid(np.arange(rows), np.arange(cols), indexing='ij')
    return ((i == 0) | (j == 0) | (i == cols - 1) | (j == rows - 1)).reshape(-1)


def cone(valence, apex_last, seed=SEED):
    """`valence` triangles (apex, r_i, r_i+1) around one apex, the rim closed (r_valence = r_0): V = valence + 1, the apex vertex 0 or vertex
    V - 1; the faces in seeded random order, so that the apex's list is filled out of order whatever the interleaving
    -> (verts [V,3] float32, faces [F,3] int32, apex)"""
    rng = np.random.default_rng(seed + valence)
    V = valence + 1
    apex = V - 1 if apex_last else 0
    rim = np.arange(valence, dtype=np.int64) + (0 if apex_last else 1)
    faces = np.stack([np.full(valence, apex), rim, np.roll(rim, -1)], 1)
    faces = faces[rng.permutation(valence)]
    ang = 2 * np.pi * np.arange(valence) / valence
    verts = np.zeros((V, 3))
    verts[rim] = np.stack([np.cos(ang), np.sin(ang), np.zeros(valence)], 1)
    verts[apex] = (0.05, -0.03, 1.0)
    verts += rng.uniform(-0.01, 0.01, size=verts.shape)
    return verts.astype(np.float32), faces.astype(np.int32), apex


# ---- the hand-written mesh: 21 vertices ------------------------------------------------------------------------------------------------------
# two tetrahedra sharing nothing (0-3, 4-7), an open strip of two rows (8-12 below, 13-17 above), vertex 18 in no face, vertices 19 and 20
# only in a degenerate face; face 3 is repeated as face 16; vertex 6 has a NaN coordinate
HAND_VERTS = 21
HAND_FACES = np.array([
    [0, 2, 1], [0, 1, 3], [1, 2, 3], [0, 3, 2],                          # tetrahedron A, outward
    [4, 6, 5], [4, 5, 7], [5, 6, 7], [4, 7, 6],                          # tetrahedron B
    [8, 9, 13], [9, 14, 13], [9, 10, 14], [10, 15, 14], [10, 11, 15], [11, 16, 15], [11, 12, 16], [12, 17, 16],      # the strip
    [0, 3, 2],                                                           # face 3 again
    [19, 20, 19],                                                        # degenerate: joins no list
], np.int32)
HAND_STRIP = np.arange(8, 18)
HAND_BOUNDARY = np.zeros(HAND_VERTS, np.uint8)
HAND_BOUNDARY[HAND_STRIP] = 1                                 # every strip vertex lies on its rim; the repeated face makes edges of THREE faces: no boundary
HAND_INC_OFF = np.array([0, 4, 7, 11, 15, 18, 21, 24, 27, 28, 31, 34, 37, 39, 41, 44, 47, 50, 51, 51, 51, 51], np.int32)      # counted by hand
HAND_LIST_OF_0 = [0, 1, 3, 16]                                # the repeated face is in the list twice over: as face 3 and as face 16
HAND_N_INCIDENT = 3 * 17


def hand_rows(width):
    """seeded rows [21, width] float32 with one NaN, at vertex 6"""
    rng = np.random.default_rng(SEED + 7 + width)
    x = rng.normal(size=(HAND_VERTS, width)).astype(np.float32)
    x[6, width - 1] = np.nan
    return x


# ---- the noisy sphere of the property test --------------------------------------------------------------------------------------------------
SPHERE_BOX = (-1.0, -1.0, -1.0, 1.0, 1.0, 1.0)
SPHERE_DIMS = (33, 33, 33)
SPHERE_CENTRE = (0.013, -0.021, 0.017)
SPHERE_RADIUS = 0.6
SPHERE_NOISE = 0.02                                           # a third of a grid cell (1 / 16): the ripple of a learned density, no floaters


def noisy_sphere_field():
    """[33,33,33] float32: the sphere's signed distance (positive inside) plus seeded white noise per grid vertex; the level is 0"""
    import isosurface_ref as IR
    f = IR.sphere_field(SPHERE_DIMS, SPHERE_BOX, SPHERE_CENTRE, SPHERE_RADIUS)
    rng = np.random.default_rng(SEED + 3)
    return (f + rng.uniform(-SPHERE_NOISE, SPHERE_NOISE, size=f.shape)).astype(np.float32)
