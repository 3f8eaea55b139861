"""The drop-in boundary: neuman_hip.install() and neuman_hip's modules against what the REFERENCE's own modules present there,
recorded from the reference unmodified by tests/golden/make_golden_dropin.py (tests/golden/dropin.npz): the signatures of the
functions install() rebinds, the state_dict layout of the reference's HumanNeRF(opt) built on the rebound modules, of its Joiner
and of HumanNeRF(opt, poses, betas, alignments, scale), and that module's vertex_forward."""
import argparse
import inspect
import json
import os
import pickle
import tempfile
import types

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "dropin.npz")
HOT_PATH = {"utils.ray_utils": ["shot_ray", "shot_rays", "shot_all_rays", "to_homogeneous", "ray_to_samples", "ray_to_importance_samples",
                                "sample_pdf", "geometry_guided_near_far", "geometry_guided_near_far_torch", "geometry_guided_near_far_np",
                                "warp_samples_to_canonical", "warp_samples_to_canonical_diff"],
            "utils.render_utils": ["raw2outputs", "render_vanilla", "render_smpl_nerf", "render_hybrid_nerf", "render_hybrid_nerf_multi_persons"]}
MODEL_CALLABLES = ["build_nerf", "build_offset_net"]


def signature_ok(recorded, fn):
    """equal to the reference's, or the reference's plus trailing keyword arguments with defaults"""
    op = list(inspect.signature(fn).parameters.values())
    same_prefix = len(op) >= len(recorded) and all(
        name == p.name and kind == p.kind.name and default == (None if p.default is inspect.Parameter.empty else repr(p.default))
        for (name, kind, default), p in zip(recorded, op))
    extras_ok = all(p.default is not inspect.Parameter.empty for p in op[len(recorded):])
    return bool(same_prefix and extras_ok)


def layout(sd):
    return [[k, list(v.shape), str(v.dtype)] for k, v in sd.items()]


def strict_load(net, recorded, seed):
    """load_state_dict(strict=True) of a state_dict with the recorded keys, shapes and dtypes (seeded values); True when every value
    reads back unchanged"""
    g = torch.Generator().manual_seed(seed)
    sd = {k: torch.randn(shape, generator=g).to(getattr(torch, dtype.split(".")[1])) for k, shape, dtype in recorded}
    net.load_state_dict(sd, strict=True)
    mine = net.state_dict()
    return all(torch.equal(mine[k], v) for k, v in sd.items())


@pytest.fixture(scope="module")
def report():
    import neuman_hip
    from neuman_hip import human_nerf as our_hn, synthetic
    g = np.load(GOLDEN)
    meta = json.loads(str(g["meta"]))
    opt = argparse.Namespace(**meta["opt"])

    # install() over stand-ins for the reference's three modules: every hot-path name must be rebound
    placeholder = object()
    mods = {name: types.ModuleType(name) for name in ("utils.ray_utils", "utils.render_utils", "models.vanilla")}
    for name, fns in HOT_PATH.items():
        for n in fns:
            setattr(mods[name], n, placeholder)
    neuman_hip.install(mods["utils.ray_utils"], mods["utils.render_utils"], mods["models.vanilla"])
    out = {"signatures": {}, "rebound": 0}
    for name, fns in HOT_PATH.items():
        for n in fns:
            ours = getattr(mods[name], n)
            out["rebound"] += int(ours is not placeholder)
            out["signatures"][f"{name}.{n}"] = {"ok": signature_ok(meta["signatures"][f"{name}.{n}"], ours),
                                                "reference": meta["signatures"][f"{name}.{n}"], "ours": str(inspect.signature(ours))}
    out["model_signatures"] = {k: signature_ok(v, getattr(mods["models.vanilla"], k.rsplit(".", 1)[1])) for k, v in meta["model_signatures"].items()}

    # HumanNeRF(opt) on the rebound models.vanilla: the reference's module tree against ours
    net = our_hn.HumanNeRF(opt)
    ref = meta["human_nerf"]
    out["human_nerf"] = {"state_dict_tensors": len(ref["state_dict"]), "parameters": ref["parameters"],
                         "layout_equal": layout(net.state_dict()) == ref["state_dict"],
                         "our_parameters": int(sum(p.numel() for p in net.parameters())),
                         "bkg_is_ours": ref["bkg_class_module"].startswith("neuman_hip") and type(net.coarse_bkg_net).__module__ == ref["bkg_class_module"],
                         "human_mapping": ref["human_mapping"], "our_human_mapping": net.coarse_human_net.pos_pe.mapping}

    # checkpoint compatibility, both directions: our state_dict has the reference Joiner's layout, and loads the reference's
    o_coarse, _ = neuman_hip.vanilla.build_nerf(opt)
    rj = meta["joiner"]["state_dict"]
    mine = layout(o_coarse.state_dict())
    out["state_dict"] = {"keys_equal": [k for k, _, _ in mine] == [k for k, _, _ in rj],
                         "shapes_equal": all(a[1:] == b[1:] for a, b in zip(mine, rj)),
                         "reference_class": meta["joiner"]["reference_class"],
                         "values_round_trip": strict_load(o_coarse, rj, 0)}

    # HumanNeRF with per-frame body parameters (train.py:103) on the synthetic body model in SMPL's file layout
    pose, betas, align = synthetic.smpl_like_frames(3, 0)
    al = np.stack([np.concatenate([align[f'{i:05d}.png'], np.array([[0.], [0.], [0.], [1.]])], 1) for i in range(3)]).astype(np.float32)
    with tempfile.TemporaryDirectory() as tmp:
        with open(os.path.join(tmp, 'SMPL_NEUTRAL.pkl'), 'wb') as f:
            pickle.dump(synthetic.smpl_like_model(0), f, protocol=2)
        o_net = our_hn.HumanNeRF(opt, pose.copy(), betas.copy(), al.copy(), scale=1.3, smpl_dir=tmp)
    with torch.no_grad():
        ov, oT = o_net.vertex_forward(1)
    rs = {k: (shape, dtype) for k, shape, dtype in meta["human_nerf_with_body"]["state_dict"]}
    os_ = {k: (shape, dtype) for k, shape, dtype in layout(o_net.state_dict())}
    reloaded = strict_load(our_hn.HumanNeRF(opt, pose.copy(), betas.copy(), al.copy(), scale=1.3, smpl_dir=synthetic.smpl_like_model(0)),
                           meta["human_nerf_with_body"]["state_dict"], 1)
    out["human_nerf_with_body"] = {"keys_equal": sorted(rs) == sorted(os_) and reloaded, "n_keys": len(rs),
                                   "shapes_equal": all(rs[k] == os_[k] for k in rs if k in os_),
                                   "only_reference": sorted(set(rs) - set(os_)), "only_ours": sorted(set(os_) - set(rs)),
                                   "reference_class_module": meta["human_nerf_with_body"]["reference_class_module"],
                                   "vertex_forward_linf": [float(np.abs(ov.numpy() - g["vertex_forward_verts"]).max()),
                                                           float(np.abs(oT.numpy() - g["vertex_forward_T"]).max())]}
    return out


def test_every_hot_path_name_is_rebound_with_the_reference_signature(report):
    sigs = report["signatures"]
    assert len(sigs) == 17 and report["rebound"] == 17
    bad = {k: v for k, v in sigs.items() if not v["ok"]}
    assert not bad, bad
    assert all(report["model_signatures"].values()), report["model_signatures"]


def test_reference_human_nerf_builds_on_the_rebound_modules(report):
    h = report["human_nerf"]
    assert h["state_dict_tensors"] == 90 and h["parameters"] == 2292111          # SURVEY 8c [probe]
    assert h["bkg_is_ours"] and h["human_mapping"] == "rotate"
    assert h["layout_equal"] and h["our_parameters"] == h["parameters"] and h["our_human_mapping"] == h["human_mapping"]


def test_checkpoints_load_strictly_both_ways(report):
    s = report["state_dict"]
    assert s["keys_equal"] and s["shapes_equal"] and s["values_round_trip"]
    assert s["reference_class"] == "models.vanilla.Joiner"


def test_human_nerf_module_has_the_references_state_dict(report):
    """neuman_hip.human_nerf.HumanNeRF(opt, poses, betas, alignments, scale) against models/human_nerf.py's (its hard-coded SMPL asset
    path redirected to a synthetic model; train.py:103's constructor call): the 101 `hybrid_model_state_dict` keys -- networks, offset
    nets, poses / betas / alignments / da_smpl, body_model.* buffers -- equal in name, shape and dtype, strict loads in both directions,
    vertex_forward equal to float32 round-off"""
    h = report["human_nerf_with_body"]
    assert h["keys_equal"] and h["shapes_equal"] and h["n_keys"] == 101 and not h["only_reference"] and not h["only_ours"], h
    assert h["reference_class_module"] == "models.vanilla"
    assert max(h["vertex_forward_linf"]) < 5e-6, h["vertex_forward_linf"]
