"""The sizes at which the mesh clean-up kernels (ml-neuman_amd/csrc/mesh_components.hip, and the ranking it
takes from csrc/mesh_device.h) change behaviour, and the meshes
tests/test_hip_mesh_components.py crosses them with.

TABLE has the form of tests/helpers/mesh_sizes.py's: name -> (value, source file, pattern whose integer groups multiply to the value);
tests/test_mesh_components_host.py checks on the CPU that every entry still reads so in the source and that every derived size lies past
its threshold.  Everything here is numpy: the meshes' expected labels are known by construction."""
import types

import numpy as np

CSRC = 'ml-neuman_amd/csrc/'
TABLE = {
    # span_rank_kernel: a workgroup ranks kSpan items (vertices or faces), kSpan / kThreads consecutive ones per thread
    'SPAN': (1024, CSRC + 'mesh_device.h', r'constexpr int kSpan = (\d+);'),
    # span_scan_kernel: ONE workgroup of kThreads scans the spans' sums, ceil(spans / kThreads) spans per thread
    'THREADS': (256, CSRC + 'mesh_device.h', r'constexpr int kThreads = (\d+);'),
}
C = types.SimpleNamespace(**{k: v[0] for k, v in TABLE.items()})

PAST_ONE_SPAN = C.SPAN + 1                                    # two spans: the second holds one item
PAST_THE_SCAN = C.SPAN * C.THREADS + 1                        # 262 145: THREADS + 1 spans, a scan thread owns two
STRIP_VERTS = PAST_THE_SCAN
DISJOINT_VERTS = C.SPAN * C.THREADS + 3                       # 262 147 = 3 x 87 382 + 1: the last vertex is in no triangle
FAN_FACES = 65536
SEED = 20


def spans(n):
    return (n + C.SPAN - 1) // C.SPAN


def per_thread(n_spans):
    return (n_spans + C.THREADS - 1) // C.THREADS


def strip(n_verts, order='ascending', cuts=()):
    """a triangle strip (i, i+1, i+2) over n_verts positions, position p carrying vertex index order[p]; the faces that span a cut (a
    position where a new piece starts) are left out -> (faces [F,3] int32, piece of every vertex [V] in position order mapped to indices)"""
    pos = np.arange(n_verts, dtype=np.int64)
    if order == 'ascending':
        index = pos
    elif order == 'descending':
        index = pos[::-1].copy()
    else:
        index = np.random.default_rng(SEED).permutation(n_verts)
    piece_of_pos = np.searchsorted(np.asarray(sorted(cuts), np.int64), pos, side='right')
    i = np.arange(n_verts - 2)
    whole = (piece_of_pos[i] == piece_of_pos[i + 2])
    i = i[whole]
    faces = np.stack([index[i], index[i + 1], index[i + 2]], 1).astype(np.int32)
    piece = np.empty(n_verts, np.int64)
    piece[index] = piece_of_pos
    return faces, piece


def strip_cuts(n_verts):
    """two seeded cut positions, each leaving pieces of at least three vertices"""
    rng = np.random.default_rng(SEED + 1)
    a = int(rng.integers(3, n_verts // 2 - 3))
    b = int(rng.integers(n_verts // 2 + 3, n_verts - 3))
    return (a, b)


def expected_labels_of_pieces(piece, referenced=None):
    """C3 for vertices whose component is known (piece [V]): ids in ascending order of the pieces' smallest vertex"""
    piece = np.asarray(piece, np.int64)
    first = np.full(int(piece.max()) + 1, piece.shape[0], np.int64)
    np.minimum.at(first, piece, np.arange(piece.shape[0]))
    ident = np.argsort(np.argsort(first))
    return ident[piece].astype(np.int32)


def fan(n_faces, hub_last):
    """n_faces triangles (hub, r_i, r_i+1) around one hub: V = n_faces + 2, the hub vertex 0 or vertex V - 1"""
    V = n_faces + 2
    rim = np.arange(n_faces + 1, dtype=np.int64) + (0 if hub_last else 1)
    hub = V - 1 if hub_last else 0
    faces = np.stack([np.full(n_faces, hub), rim[:-1], rim[1:]], 1).astype(np.int32)
    return faces, V


def disjoint_triangles(n_verts):
    """(3t, 3t+1, 3t+2) for every whole triple below n_verts: C = n_verts // 3, vertices past the last triple unreferenced"""
    t = np.arange(n_verts // 3, dtype=np.int64)
    return np.stack([3 * t, 3 * t + 1, 3 * t + 2], 1).astype(np.int32)


# ---- the hand-written mesh: 12 vertices, 0 and 11 in no face; a repeated face, (a,a,b) and (a,a,a) ---------------------------------------
HAND_VERTS = 12
HAND_FACES = np.array([[5, 3, 7], [1, 1, 4], [10, 2, 6], [8, 8, 8], [7, 9, 5], [10, 2, 6]], np.int32)
HAND_VERT_LABEL = np.array([-1, 0, 1, 2, 0, 2, 1, 2, 3, 2, 1, -1], np.int32)      # representatives 1, 2, 3, 8
HAND_FACE_LABEL = np.array([2, 0, 1, 3, 2, 1], np.int32)
HAND_COMP_VERTS = np.array([2, 3, 4, 1], np.int32)
HAND_COMP_FACES = np.array([1, 2, 2, 1], np.int32)

# ---- the three-blob isosurface ------------------------------------------------------------------------------------------------------------
BLOB_BOX = (-1.0, -1.0, -1.0, 1.0, 1.0, 1.0)
BLOB_DIMS = (25, 25, 25)
_S = 0.013
BLOBS = (((0.45 + _S, _S, _S), 0.3), ((-0.45 + _S, _S, _S), 0.38), ((_S, 0.7 + _S, -0.6 + _S), 0.12))
BLOB_EXPECTED = dict(n_verts=2002, n_faces=3992, representatives=(0, 110, 200), comp_verts=(110, 1170, 722), comp_faces=(216, 2336, 1440),
                     label_changes=113)


def blob_field():
    """[25,25,25] float32: the maximum of the three spheres' signed distances (positive inside); the level is 0"""
    import isosurface_ref as IR
    f = None
    for centre, r0 in BLOBS:
        g = IR.sphere_field(BLOB_DIMS, BLOB_BOX, centre, r0)
        f = g if f is None else np.maximum(f, g)
    return f


def two_equal_spheres_field():
    """two spheres of one radius, twelve whole grid steps (1.0) apart along x: the same crossed edges, so the same face count (the Kuhn
    split is not mirror symmetric: a mirror image would not do)"""
    import isosurface_ref as IR
    return np.maximum(IR.sphere_field(BLOB_DIMS, BLOB_BOX, (0.513, 0.02, 0.03), 0.3), IR.sphere_field(BLOB_DIMS, BLOB_BOX, (-0.487, 0.02, 0.03), 0.3))
