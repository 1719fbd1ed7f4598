"""KITTI raw calibration and Velodyne files (host only), as far as the LiDAR depth ground truth needs them
(core/evaluation.py::generate_depth_map; the chain of mono/datasets/kitti_utils.py:50-66):

    read_calib_file(path)              'key: value' lines -> dict; a value made of numbers only becomes a float64 array
    velo_to_image(calib_dir, cam=2)    (P (3,4) float64 velodyne -> image plane of camera `cam`, (H, W) of the rectified image)
    load_velodyne_points(path)         the scan as (N, 4) float32: x forward, y left, z up, reflectance

File formats (KITTI raw data development kit, readme of the calibration files): calib_cam_to_cam.txt holds, per camera c,
S_rect_0c (width height of the rectified image), R_rect_0c (3x3 rectifying rotation) and P_rect_0c (3x4 projection after
rectification); calib_velo_to_cam.txt holds R (3x3) and T (3) of the rigid velodyne -> camera 0 transform.  A velodyne .bin file is
a flat array of little-endian float32, four per point."""
from __future__ import annotations

import os

import numpy as np


def read_calib_file(path) -> dict:
    out = {}
    with open(path, "r") as f:
        for line in f:
            if ":" not in line:
                continue
            key, value = line.split(":", 1)
            value = value.strip()
            try:
                out[key] = np.array([float(tok) for tok in value.split()], dtype=np.float64) if value else value
            except ValueError:
                out[key] = value                      # e.g. calib_time: 09-Jan-2012 13:57:47
    return out


def velo_to_image(calib_dir, cam=2):
    """P = P_rect_0cam @ R_rect_00 (as 4x4) @ [R | T; 0 0 0 1], multiplied in that order, and the (H, W) of S_rect_0cam."""
    cam2cam = read_calib_file(os.path.join(calib_dir, "calib_cam_to_cam.txt"))
    velo2cam = read_calib_file(os.path.join(calib_dir, "calib_velo_to_cam.txt"))
    rigid = np.identity(4)
    rigid[:3, :3] = velo2cam["R"].reshape(3, 3)
    rigid[:3, 3] = velo2cam["T"]
    rect = np.identity(4)
    rect[:3, :3] = cam2cam["R_rect_00"].reshape(3, 3)
    proj = cam2cam[f"P_rect_0{int(cam)}"].reshape(3, 4)
    width, height = cam2cam[f"S_rect_0{int(cam)}"].astype(np.int32)
    return (proj @ rect) @ rigid, (int(height), int(width))


def load_velodyne_points(path) -> np.ndarray:
    pts = np.fromfile(path, dtype="<f4")
    if pts.size % 4:
        raise ValueError(f"{path}: {pts.size} floats is not a whole number of (x, y, z, reflectance) points")
    return pts.reshape(-1, 4)
