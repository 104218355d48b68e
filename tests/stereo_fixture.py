"""A stereo dataset in the KITTI layout for the drop-in reader with estimateDepth: image_2/ (left), image_3/ (right), semantics/,
calibration.txt, times.txt, pose.txt -- and no PSMNet/, the depth is what the library estimates."""
import os

import numpy as np

import kitti_fixture as kf


def write_stereo_dataset(root, cam, frames, poses, with_right=True):
    """frames: [(rgb_left, rgb_right, sem)], poses: 4x4 camera->world matrices BEFORE the reader's T20 offset"""
    for d in ("image_2", "semantics") + (("image_3",) if with_right else ()):
        os.makedirs(os.path.join(root, d), exist_ok=True)
    with open(os.path.join(root, "calibration.txt"), "w") as f:
        f.write(f"{cam['fx']} {cam['fy']} {cam['cx']} {cam['cy']}\n{cam['width']} {cam['height']}\n")
    with open(os.path.join(root, "times.txt"), "w") as f:
        for k in range(len(frames)):
            f.write(f"{0.1 * k:.6f}\n")
    with open(os.path.join(root, "pose.txt"), "w") as f:
        for p in poses:
            f.write(" ".join(f"{v:.9g}" for v in np.asarray(p, np.float32)[:3, :].reshape(-1)) + "\n")
    for k, (left, right, sem) in enumerate(frames):
        kf.write_png(os.path.join(root, "image_2", f"{k:06d}.png"), left)
        if with_right:
            kf.write_png(os.path.join(root, "image_3", f"{k:06d}.png"), right)
        kf.write_png(os.path.join(root, "semantics", f"{k:06d}.png"), sem)
