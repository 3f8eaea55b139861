"""What the REFERENCE's small pure functions of preprocess/optimize_smpl.py return (tests/golden/optimize_smpl.npz).  Build container only:
    python tests/golden/make_golden_optimize_smpl.py
coco_to_smpl, densepose_name_to_idx, turn_smpl_gradient_on and clip_smpl_vals, imported unmodified (absent wheels stubbed), on seeded inputs."""
import json
import os
import sys
from unittest import mock

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
for m in ["igl", "open3d", "pytorch3d", "pytorch3d.structures", "pytorch3d.renderer", "imageio", "lpips", "tensorboardX", "skimage", "skimage.metrics",
          "torchvision", "torchvision.utils", "cv2", "matplotlib", "matplotlib.pyplot", "tqdm", "joblib", "trimesh", "scipy.spatial.transform", "PIL"]:
    try:
        __import__(m)
    except Exception:
        sys.modules[m] = mock.MagicMock(name=m)
sys.path.insert(0, "/root/reference")
sys.path.insert(0, "/root/reference/preprocess")
from preprocess import optimize_smpl as R  # noqa: E402

rng = np.random.default_rng(0)
coco = rng.uniform(0, 500, size=(5, 17, 2))
smpl2d = np.stack([R.coco_to_smpl(c) for c in coco])
label_sets = [rng.choice(25, size=rng.integers(1, 25), replace=False) for _ in range(100)] + [np.arange(25), np.array([0]), np.array([15, 17]), np.array([5, 6])]
maps = np.stack([rng.choice(s, size=(9, 7)) for s in label_sets])
masks = np.stack([R.turn_smpl_gradient_on(m) for m in maps])
np.savez_compressed(os.path.join(HERE, 'optimize_smpl.npz'), coco=coco, smpl2d=smpl2d, maps=maps, masks=masks, limits=R.clip_smpl_vals(),
                    name_to_idx=np.array(json.dumps(R.densepose_name_to_idx())))
print(smpl2d.shape, maps.shape, masks.shape, masks.mean())
