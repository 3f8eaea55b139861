"""The inputs of tests/test_hip_smpl_edges.py are fair: on every body model and pose of tests/helpers/body_edges.py the skinning chain evaluated on the
host in FLOAT32 (SMPLDiff.vertex_forward_torch under torch's autograd, and oracle/smpl.py's numpy restatement of the reference) stays within ONE
QUARTER of the tolerance at which the HIP kernels are then compared with the float64 chain.  A condition on the inputs, not a measurement of the
kernels: a case whose float32 evaluation wanders by itself (a near-singular blend of the da pose, a gradient that cancels to nothing) would make the
device test a test of luck.  Runs without a GPU."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "helpers"))
import body_edges as BE  # noqa: E402
from oracle import smpl as OS  # noqa: E402


def test_model_recipe():
    """the helper builds what it says: sparse normalised weights and regressor, an earlier-joint tree, SMPL's root marker"""
    for V, J, NB in BE.SHAPE_CASES:
        m = BE.model(V, J, NB)
        assert m['v_template'].shape == (V, 3) and m['shapedirs'].shape == (V, 3, NB) and m['J_regressor'].shape == (J, V) and m['weights'].shape == (V, J)
        np.testing.assert_allclose(m['weights'].sum(1), 1.0, atol=1e-12)
        np.testing.assert_allclose(m['J_regressor'].sum(1), 1.0, atol=1e-12)
        assert ((m['weights'] != 0).sum(1) <= 4).all() and ((m['J_regressor'] != 0).sum(1) <= 8).all()
        if J > 4:
            assert (m['weights'] == 0).any()                                        # the sparse skips have something to skip
        par = m['kintree_table'][0]
        assert par[0] == 2 ** 32 - 1 and all(max(0, j - 3) <= par[j] < j for j in range(1, J))
        assert int(m['f'].max()) < V
    rng = np.random.default_rng(0)
    assert not BE.edge_pose(24, "zero", rng).any()
    assert 0 < np.abs(BE.edge_pose(24, "tiny", rng)).max() < 1e-5
    mixed = BE.edge_pose(24, "mixed", rng).reshape(24, 3)
    assert not mixed[::2].any() and mixed[1::2].all()
    pi = BE.edge_pose(24, "pi", rng).reshape(24, 3)
    assert pi[0, 0] == np.float32(np.pi) and pi[23, 1] == np.float32(2 * np.pi + 0.3) and tuple(pi[1]) == (0, 0, 1)


@pytest.mark.parametrize("case", BE.CASES, ids=BE.case_id)
def test_float32_references_stay_within_a_quarter_of_the_tolerances(case):
    V, J, NB, kind = case
    x = BE.inputs(V, J, NB, kind)
    ow, oT = OS.vertex_forward(OS.Model(BE.model(V, J, NB)), x['pose'][0], x['beta'][0], x['align'], BE.SCALE)
    line = []
    for through in ("both", "world", "T"):                           # the loss of the device test's three variants
        f64 = BE.reference(V, J, NB, kind, through, True)
        f32 = BE.reference(V, J, NB, kind, through, False)
        for name in ("world", "T", "g_pose", "g_beta", "g_align") if through == "both" else ("g_pose", "g_beta", "g_align"):
            assert np.isfinite(f64[name]).all() and np.isfinite(f32[name]).all(), name
            e = BE.rel_err(f32[name], f64[name], BE.grad_scale(V, J, NB, kind, through, name))
            line.append(f"{name}{'' if through == 'both' else ' through ' + through} {e:.1e}")
            assert e <= BE.tol(name) / 4, (name, through, e)
    f64 = BE.reference(V, J, NB, kind, "both", True)
    for name, got in (("world", ow), ("T", oT)):
        e = BE.rel_err(got, f64[name][0])
        line.append(f"oracle {name} {e:.1e}")
        assert np.isfinite(got).all() and e <= BE.tol(name) / 4, ("oracle", name, e)
    print(f"[body-edges host] {BE.case_id(case)}: float32 vs float64, fraction of the largest entry: " + ", ".join(line))
