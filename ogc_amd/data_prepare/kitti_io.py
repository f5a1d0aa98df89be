"""Readers of the raw KITTI files the preparation drivers take, and the box rows ogc_box_segm labels with.

Plain-float restatements of data_prepare/kittidet/kittidet_util.py (`read_calib_file` :174-192, `Object3d` :50-82, `roty`
:347-351, `read_label` :378-381) and of the box arithmetic of process_kittidet.py:33-65 / process_waymo.py:48-84.  The image
size comes from the PNG header (PIL); no image is decoded.
"""
import math

import numpy as np


def read_calib_file(path):
    """key -> float64 array of the numbers after `key:`; lines whose values are not numbers are passed over."""
    data = {}
    with open(path, "r") as f:
        for line in f.readlines():
            line = line.rstrip()
            if len(line) == 0:
                continue
            key, value = line.split(":", 1)
            try:
                data[key] = np.array([float(x) for x in value.split()])
            except ValueError:
                pass
    return data


def read_kittidet_calib(path):
    """KITTI-Det calib/%06d.txt -> {"P" (3, 4) from P2, "V2C" (3, 4) from Tr_velo_to_cam, "R0" (3, 3) from R0_rect}."""
    c = read_calib_file(path)
    return {"P": c["P2"].reshape(3, 4), "V2C": c["Tr_velo_to_cam"].reshape(3, 4), "R0": c["R0_rect"].reshape(3, 3)}


def read_semantickitti_calib(path):
    """SemanticKITTI sequences/%02d/calib.txt -> {"P" (3, 4) from P2, "V2C" (3, 4) from Tr}; there is no R0."""
    c = read_calib_file(path)
    return {"P": c["P2"].reshape(3, 4), "V2C": c["Tr"].reshape(3, 4)}


def read_kittisf_calib(path):
    """KITTI Scene Flow calib_cam_to_cam/%06d.txt -> P_rect_02 as a (3, 4) float32 array (process_kittisf.py:32-40): exactly one
    such line, and equal focal lengths on both axes."""
    with open(path) as f:
        lines = [line for line in f.readlines() if line.startswith("P_rect_02")]
    if len(lines) != 1:
        raise ValueError("%s: %d lines start with P_rect_02, expected one" % (path, len(lines)))
    P = np.array([float(item) for item in lines[0].split()[1:]], dtype=np.float32).reshape(3, 4)
    if P[0, 0] != P[1, 1]:
        raise ValueError("%s: P_rect_02 has different focal lengths, %r and %r" % (path, P[0, 0], P[1, 1]))
    return P


def image_size(path):
    """(width, height) from the image's header."""
    from PIL import Image
    with Image.open(path) as img:
        return img.size


class Object3d(object):
    """One line of a KITTI label_2 file."""

    def __init__(self, line):
        data = line.split(" ")
        data[1:] = [float(x) for x in data[1:]]
        self.type = data[0]
        self.truncation = data[1]
        self.occlusion = int(data[2])
        self.alpha = data[3]
        self.xmin, self.ymin, self.xmax, self.ymax = data[4], data[5], data[6], data[7]
        self.h, self.w, self.l = data[8], data[9], data[10]
        self.t = (data[11], data[12], data[13])      # location in camera coordinates
        self.ry = data[14]                           # yaw about the camera's y axis


def read_label(path):
    with open(path) as f:
        return [Object3d(line.rstrip()) for line in f if line.rstrip()]


def roty(t):
    c, s = math.cos(t), math.sin(t)
    return np.array([[c, 0.0, s], [0.0, 1.0, 0.0], [-s, 0.0, c]])


KITTIDET_SIGN = (-1, -1, 1)     # the saved cloud is the rect camera frame with x and y flipped; the boxes live in the rect frame


def kittidet_boxes(objects, relax=0.01):
    """Box rows of the `Car` objects of a label file (process_kittidet.py:46-64): rot = roty(-ry), centre = obj.t, bounds
    x +-(l/2 + relax), y (-h - relax, relax) — t is the bottom centre and y points down —, z +-(w/2 + relax); the object id is the
    line index + 1 counting every line.  -> boxes (K, 18) float64, ids (K, 2) int32 [id, 1]."""
    boxes, ids = [], []
    for sid, obj in enumerate(objects):
        if obj.type != "Car":
            continue
        l, w, h = obj.l, obj.w, obj.h
        lo = [-l / 2 - relax, -h - relax, -w / 2 - relax]
        hi = [l / 2 + relax, relax, w / 2 + relax]
        boxes.append(np.concatenate([roty(-obj.ry).reshape(9), np.asarray(obj.t, dtype=np.float64), lo, hi]))
        ids.append([sid + 1, 1])
    return (np.asarray(boxes, dtype=np.float64).reshape(-1, 18), np.asarray(ids, dtype=np.int32).reshape(-1, 2))


def waymo_boxes(gt_boxes, object_ids, class_ids, relax=0.01):
    """Box rows of Waymo boxes (K, 7) [x, y, z, l, w, h, heading] (process_waymo.py:63-79): rot = the rotation about z by
    -heading — Rotation.from_euler('zyx', [-heading, 0, 0]) in closed form —, centre = box[0:3], bounds x +-(l/2 + relax),
    y +-(h/2 + relax), z +-(w/2 + relax): the reference pairs h with the lidar's y axis and w with z, and so does this.
    The boxes are taken to float64 first.  -> boxes (K, 18) float64, ids (K, 2) int32."""
    gt = np.asarray(gt_boxes, dtype=np.float64).reshape(-1, 7)
    rows = np.zeros((gt.shape[0], 18), dtype=np.float64)
    c, s = np.cos(-gt[:, 6]), np.sin(-gt[:, 6])
    rows[:, 0], rows[:, 1], rows[:, 3], rows[:, 4], rows[:, 8] = c, -s, s, c, 1.0
    rows[:, 9:12] = gt[:, 0:3]
    l, w, h = gt[:, 3], gt[:, 4], gt[:, 5]
    rows[:, 15], rows[:, 16], rows[:, 17] = l / 2 + relax, h / 2 + relax, w / 2 + relax
    rows[:, 12], rows[:, 13], rows[:, 14] = -l / 2 - relax, -h / 2 - relax, -w / 2 - relax
    ids = np.stack([np.asarray(object_ids, dtype=np.int32).reshape(-1), np.asarray(class_ids, dtype=np.int32).reshape(-1)], 1)
    return rows, np.ascontiguousarray(ids)
