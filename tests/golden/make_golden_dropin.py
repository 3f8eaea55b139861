"""What the REFERENCE's own modules present at the drop-in boundary (tests/golden/dropin.npz), recorded so that
tests/test_install_dropin.py checks neuman_hip against it without the reference.  Needs a checkout of the reference:

    python tests/golden/make_golden_dropin.py /path/to/ml-neuman

The reference is imported unmodified with its absent wheels stubbed (as make_golden.py does), and recorded:

  * the options the networks are built with (the defaults of options/options.py, on the CPU);
  * the signature of every hot-path function install() rebinds (utils/ray_utils.py, utils/render_utils.py) and of the
    model callables of models/vanilla.py: parameter names, kinds and default values;
  * HumanNeRF(opt) (models/human_nerf.py:21-31) built on the rebound models.vanilla: its state_dict layout and parameter count,
    which classes its networks are and the mapping of its canonical net;
  * the state_dict layout of the reference's own build_nerf(opt) Joiner and its class;
  * HumanNeRF(opt, poses, betas, alignments, scale) on the reference's ORIGINAL models.vanilla (train.py:103; its hard-coded SMPL
    asset directory redirected to the synthetic model of neuman_hip.synthetic in SMPL's file layout): its state_dict layout and
    vertex_forward(1).
"""
import argparse
import contextlib
import importlib
import inspect
import io
import json
import os
import pickle
import sys
import tempfile
from unittest import mock

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, "..", ".."))
ap = argparse.ArgumentParser()
ap.add_argument("reference", help="the reference checkout (the directory holding utils/, models/, options/)")
REF = os.path.abspath(ap.parse_args().reference)
for m in ["igl", "open3d", "pytorch3d", "pytorch3d.structures", "pytorch3d.renderer", "imageio", "lpips", "tensorboardX",
          "skimage", "skimage.metrics", "torchvision", "torchvision.utils", "cv2"]:
    sys.modules[m] = mock.MagicMock(name=m)
sys.path.insert(0, REF)
sys.path.insert(0, os.path.join(ROOT, "ml-neuman_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402
from utils import ray_utils, render_utils  # noqa: E402  (reference)
from models import vanilla  # noqa: E402
from options import options  # noqa: E402
from test_install_dropin import HOT_PATH, MODEL_CALLABLES  # noqa: E402


def parse_opt():
    parser = argparse.ArgumentParser()
    for f in (options.set_general_option, options.set_nerf_option, options.set_pe_option, options.set_render_option):
        f(parser)
    parser.add_argument('--offset_scale', type=float, default=1.0)
    parser.add_argument('--num_offset_nets', type=int, default=1)
    parser.add_argument('--offset_scale_type', type=str, default='linear')
    parser.add_argument('--out_dir', type=str, default='./out')
    parser.add_argument('--load_background', type=str, default='none')
    parser.add_argument('--load_can', type=str, default='none')
    parser.add_argument('--posenc', type=str, default='posenc')
    return parser.parse_args(['--use_cuda', 'no'])


def signature(fn):
    return [[p.name, p.kind.name, None if p.default is inspect.Parameter.empty else repr(p.default)]
            for p in inspect.signature(fn).parameters.values()]


def layout(sd):
    return [[k, list(v.shape), str(v.dtype)] for k, v in sd.items()]


opt = parse_opt()
meta = {"opt": vars(opt), "signatures": {}, "model_signatures": {}}
for modname, names in HOT_PATH.items():
    mod = importlib.import_module(modname)
    for n in names:
        meta["signatures"][f"{modname}.{n}"] = signature(getattr(mod, n))
for n in MODEL_CALLABLES:
    meta["model_signatures"][f"models.vanilla.{n}"] = signature(getattr(vanilla, n))

torch.manual_seed(0)
r_coarse, _ = vanilla.build_nerf(opt)                     # the reference's own classes (models.vanilla is rebound below)
meta["joiner"] = {"reference_class": f"{type(r_coarse).__module__}.{type(r_coarse).__name__}", "state_dict": layout(r_coarse.state_dict())}

import neuman_hip  # noqa: E402

neuman_hip.install(ray_utils, render_utils, vanilla)
from models import human_nerf  # noqa: E402  (imports models.vanilla -> ours now)
with contextlib.redirect_stdout(io.StringIO()):
    net = human_nerf.HumanNeRF(opt)
meta["human_nerf"] = {"state_dict": layout(net.state_dict()), "parameters": int(sum(p.numel() for p in net.parameters())),
                      "bkg_class_module": type(net.coarse_bkg_net).__module__, "human_mapping": net.coarse_human_net.pos_pe.mapping}

from neuman_hip import synthetic  # noqa: E402
for name in ("models.vanilla", "models.human_nerf"):
    sys.modules.pop(name, None)
importlib.import_module("models.vanilla")                    # a fresh, un-rebound copy
ref_hn = importlib.import_module("models.human_nerf")
from models import smpl as ref_smpl  # noqa: E402
pose, betas, al = synthetic.smpl_like_frames(3, 0)
al = np.stack([np.concatenate([al[f'{i:05d}.png'], np.array([[0.], [0.], [0.], [1.]])], 1) for i in range(3)]).astype(np.float32)
with tempfile.TemporaryDirectory() as tmp:
    with open(os.path.join(tmp, 'SMPL_NEUTRAL.pkl'), 'wb') as f:
        pickle.dump(synthetic.smpl_like_model(0), f, protocol=2)
    real_smpl = ref_smpl.SMPL
    ref_hn.SMPL = lambda path, gender='neutral', device=None: real_smpl(tmp, gender=gender, device=device)
    with contextlib.redirect_stdout(io.StringIO()):
        r_net = ref_hn.HumanNeRF(opt, pose.copy(), betas.copy(), al.copy(), scale=1.3)
with torch.no_grad():
    rv, rT = r_net.vertex_forward(1)
meta["human_nerf_with_body"] = {"state_dict": layout(r_net.state_dict()), "reference_class_module": type(r_net.coarse_bkg_net).__module__}

out = os.path.join(HERE, "dropin.npz")
np.savez_compressed(out, meta=np.array(json.dumps(meta)), vertex_forward_verts=rv.numpy(), vertex_forward_T=rT.numpy())
print(out, {k: len(v) for k, v in meta["signatures"].items()}, rv.shape, rT.shape)
