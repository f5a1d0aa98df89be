"""OGC-DR preparation, the scene composition (reference: data_prepare/ogcdr/build_ogcdr.py): ShapeNet meshes set into rooms of four
frames -> <data_root>/mesh/<NN_id>/ and <data_root>/data/<NN_id>/, what sample_pointcloud, build_ogcdrsv, collect_segm and
OGCDynamicRoomDataset read.

    python -m ogc_amd.data_prepare.build_ogcdr DATA_ROOT --split_root DIR [--types 8,7,6,5,4] [--dataset_size 1000]
                                               [--keep_background] [--seed 0] [--n_sample_point 100000]
                                               [--n_sample_point_fps 2048] [--batch 64] [--synthetic N]

DATA_ROOT/ShapeNet_mesh/<class>/<model>/model.obj are read with mesh_io.read_obj, DIR/<class>/{train,val,test}.lst name the models of
a split (the reference's data_prepare/ogcdr/raw_splits).  As in the reference the k-th entry of --types takes the k-th scale
interval, rooms are numbered per type through the three splits, and a split holds int(p * dataset_size) rooms, p = 75 / 5 / 20 %.

Per (type, split) trials j = 0, 1, 2, ... are composed in batches of --batch.  The host draws a trial's models, scales, room range and
wall height from np.random.RandomState([seed & 0xffffffff, type_id, split_id, j]) in the reference's order, scales and centres the
meshes as load_meshes does — the centre is that of the bounding box BEFORE scaling, a quirk that decides where objects stand and is
kept — and uploads the batch once.  The device places the objects of all frames (mesh_ops.compose_rooms: DESIGN §4p) under the seed
trial_seed(seed, type_id, split_id, j) and moves the vertices (mesh_ops.apply_poses); poses, status and frame vertices come back in
one copy each.  Scene i of a split is the i-th trial that composed, in trial order, so the output does not depend on --batch.

Per scene: mesh/<NN_id>/object_FF_OO.obj, ground.obj, wall_00..03.obj, meta.pkl with the reference's keys; data/<NN_id>/pose_FF.npy,
the map from the canonical mesh to the frame's mesh (the reference's saved pose disagrees with its mesh in y: DESIGN §4p), and
pc_FF.npy, segm_FF.npy by sample_pointcloud.sample_frame under frame_seed(seed, scene_index, frame) with the scene's position among
the sorted names of mesh/, so that sample_pointcloud over the same root writes the same files; data/{train,val,test}.lst at the end.
The placement is this package's own definition (include/ogc_ops.h: ogc_room_compose): np.random's stream, which the reference shares
with trimesh, cannot be reproduced.  `--synthetic N` first writes a root of N models per class and split
(ogc_amd/utils/synthetic.py::write_shapenet_root) and lets --types and --dataset_size default to 3,2 and 4.
"""
import argparse
import functools
import os
import pickle

import numpy as np
import torch

from .mesh_io import read_obj, write_obj
from .mesh_ops import apply_poses, compose_rooms
from .sample_pointcloud import N_FRAME, frame_seed, sample_frame

CLASSES = ("02828884", "02933112", "03001627", "03211117", "03636649", "04256520", "04379243")      # build_ogcdr.py:36-49
N_OBJECTS = (8, 7, 6, 5, 4)
SCALE_INTERVALS = ((0.2, 0.3), (0.2, 0.35), (0.25, 0.35), (0.25, 0.40), (0.25, 0.45))
SPLIT_PERCENTAGES = (.75, .05, .2)
SPLIT_NAMES = ("train", "val", "test")
XZ_GROUND_RANGE = (0.6, 1.)                                                                         # :54-59
WALL_HEIGHT_RANGE = (0.2, 0.4)
MAX_TRIALS_PER_ROOM = 1000      # a split whose trials keep failing is given up after this many per room it still needs


def split_sizes(dataset_size):
    """build_ogcdr.py:50."""
    return [int(p * dataset_size) for p in SPLIT_PERCENTAGES]


def trial_rng(seed, type_id, split_id, j):
    """The host stream of trial j of a (type, split): numpy's frozen legacy generator, seeded by the four numbers."""
    return np.random.RandomState([int(seed) & 0xffffffff, int(type_id), int(split_id), int(j)])


def trial_seed(seed, type_id, split_id, j):
    """The 64-bit device seed of that trial: the low 32 bits of `seed` above type_id << 28 | split_id << 26 | j."""
    if not (0 <= type_id < 16 and 0 <= split_id < 4 and 0 <= j < 1 << 26):
        raise ValueError("type_id must be below 16, split_id below 4 and the trial number below 2**26")
    return ((int(seed) & 0xffffffff) << 32) | (int(type_id) << 28 | int(split_id) << 26 | int(j))


def draw_trial(rs, model_files, n_object, type_id):
    """What the reference draws for a scene before it places anything, in its order (build_ogcdr.py:428-436, with sample_models'
    two choices per object taken from `rs` too) -> the scene's meta entries."""
    classes = sorted(model_files)
    obj_list, cl_list = [], []
    for _ in range(n_object):
        cl = classes[rs.randint(len(classes))]
        cl_list.append(cl)
        obj_list.append("%s/%s" % (cl, model_files[cl][rs.randint(len(model_files[cl]))]))
    lo, hi = SCALE_INTERVALS[type_id]
    scales = [lo + rs.rand() * (hi - lo) for _ in range(n_object)]
    short_is_z = rs.rand() > 0.5                    # which of x and z is the shorter side of the room; the other is 1
    short = rs.rand() * (XZ_GROUND_RANGE[1] - XZ_GROUND_RANGE[0]) + XZ_GROUND_RANGE[0]
    xz = np.array([1.0, short] if short_is_z else [short, 1.0])
    wall_height = WALL_HEIGHT_RANGE[0] + rs.rand() * (WALL_HEIGHT_RANGE[1] - WALL_HEIGHT_RANGE[0])
    return {"objects": obj_list, "classes": cl_list, "scales": scales, "xz_ground_range": xz, "wall_height": wall_height}


def canonical_vertices(vertices, scale):
    """load_meshes (build_ogcdr.py:119-125): the longest edge of the bounding box becomes `scale`; then HALF THE SUM OF THE UNSCALED
    BOX'S CORNERS is taken off, as the reference does."""
    corner_lo, corner_hi = vertices.min(0), vertices.max(0)
    longest = (corner_hi - corner_lo).max()
    return vertices / longest * scale - (corner_lo + corner_hi) / 2


def read_split_list(split_root, cl, split_name):
    """The model names of <split_root>/<class>/<split>.lst, one per line."""
    with open(os.path.join(split_root, cl, split_name + ".lst"), "r") as f:
        return [line for line in f.read().split("\n") if line]


def compose_batch(trials, load, device="cuda"):
    """trials: [(meta entries, device seed)] -> per trial None, or (poses (n, N_FRAME, 4, 4), frames (N_FRAME, V_t, 3), faces [..]),
    numpy.  One upload, one launch each of compose_rooms and apply_poses, one copy back of status, poses and frame vertices."""
    meshes = [[load(name) for name in meta["objects"]] for meta, _ in trials]
    verts = [canonical_vertices(v, s) for t, (meta, _) in enumerate(trials) for (v, _), s in zip(meshes[t], meta["scales"])]
    vert_offsets = np.cumsum([0] + [len(v) for v in verts])
    obj_offsets = np.cumsum([0] + [len(m) for m in meshes])
    up = lambda a, dtype: torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(device)      # noqa: E731
    vertices, vo = up(np.concatenate(verts, 0), np.float64), up(vert_offsets, np.int32)
    composed = compose_rooms(vertices, vo, up(obj_offsets, np.int32), up(np.stack([meta["xz_ground_range"] for meta, _ in trials]), np.float64),
                             up(np.array([seed - (1 << 64) if seed >= 1 << 63 else seed for _, seed in trials], dtype=np.int64), np.int64),
                             n_frame=N_FRAME)
    frames = apply_poses(vertices, vo, composed.poses).cpu().numpy()
    status, poses = composed.status.cpu().numpy(), composed.poses.cpu().numpy()
    out = []
    for t in range(len(trials)):
        if status[t, 0] != 0:
            out.append(None)
            continue
        o0, o1 = obj_offsets[t], obj_offsets[t + 1]
        out.append((poses[o0:o1], [frames[:, vert_offsets[o]:vert_offsets[o + 1]] for o in range(o0, o1)], [f for _, f in meshes[t]]))
    return out


def write_scene(data_root, name, meta, poses, frames, faces, keep_background, sizes, seed, scene_index):
    from ..utils.synthetic import ogcdr_background_meshes
    mesh_path, save_path = os.path.join(data_root, "mesh", name), os.path.join(data_root, "data", name)
    os.makedirs(mesh_path, exist_ok=True)
    os.makedirs(save_path, exist_ok=True)
    with open(os.path.join(mesh_path, "meta.pkl"), "wb") as f:
        pickle.dump(meta, f, protocol=pickle.HIGHEST_PROTOCOL)
    ground, walls = ogcdr_background_meshes(meta["xz_ground_range"], meta["wall_height"])
    for w, wall in enumerate(walls):
        write_obj(os.path.join(mesh_path, "wall_%02d.obj" % w), *wall)
    write_obj(os.path.join(mesh_path, "ground.obj"), *ground)
    background = [(v, np.asarray(f, dtype=np.int32)) for v, f in [ground] + walls] if keep_background else []
    for frame_id in range(N_FRAME):
        objects = [(np.ascontiguousarray(frames[k][frame_id]), faces[k]) for k in range(len(faces))]
        for k, (vertices, f) in enumerate(objects):
            write_obj(os.path.join(mesh_path, "object_%02d_%02d.obj" % (frame_id, k)), vertices, f)
        points, segms = sample_frame(objects + background, len(objects), meta["xz_ground_range"], sizes[0], sizes[1],
                                     frame_seed(seed, scene_index, frame_id), where="scene %s, frame %d" % (name, frame_id))
        np.save(os.path.join(save_path, "pc_%02d.npy" % frame_id), points)
        np.save(os.path.join(save_path, "segm_%02d.npy" % frame_id), segms)
        np.save(os.path.join(save_path, "pose_%02d.npy" % frame_id), np.ascontiguousarray(poses[:, frame_id]))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("data_root", type=str, help="Root path for the dataset: ShapeNet_mesh/ below it; mesh/ and data/ are written")
    ap.add_argument("--split_root", type=str, required=True, help="<class>/{train,val,test}.lst, the reference's raw_splits")
    ap.add_argument("--types", type=str, default=None, help="objects per room of every type, at most %d types (default 8,7,6,5,4)" % len(N_OBJECTS))
    ap.add_argument("--dataset_size", type=int, default=None, help="rooms per type (default 1000)")
    ap.add_argument("--keep_background", dest="keep_background", default=False, action="store_true",
                    help="sample ground and walls too (label 0)")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--n_sample_point", type=int, default=100000, help="surface points drawn per frame before the sampling")
    ap.add_argument("--n_sample_point_fps", type=int, default=2048, help="points kept per frame by furthest point sampling")
    ap.add_argument("--batch", type=int, default=64, help="trial scenes composed per launch")
    ap.add_argument("--synthetic", type=int, default=0, help="write a synthetic root of this many models per class and split first")
    args = ap.parse_args(argv)
    if args.synthetic < 0:
        raise ValueError("--synthetic must not be negative")
    types = [int(x) for x in (args.types or ("3,2" if args.synthetic else ",".join(str(n) for n in N_OBJECTS))).split(",")]
    dataset_size = args.dataset_size if args.dataset_size is not None else (4 if args.synthetic else 1000)
    if not 1 <= len(types) <= len(SCALE_INTERVALS) or not all(1 <= n <= 32 for n in types) or len(set(types)) != len(types):
        raise ValueError("--types must be 1 to %d different numbers in 1..32, got %s" % (len(SCALE_INTERVALS), types))
    if dataset_size < 0 or args.batch < 1 or args.n_sample_point < 1 or args.n_sample_point_fps < 1:
        raise ValueError("--dataset_size must not be negative; --batch, --n_sample_point and --n_sample_point_fps must be at least 1")
    if not torch.cuda.is_available():
        raise RuntimeError("build_ogcdr needs a HIP device; ogc_amd has no CPU path")
    if args.synthetic > 0:
        from ..utils.synthetic import write_shapenet_root
        write_shapenet_root(args.data_root, args.split_root, args.synthetic)
    src_dir = os.path.join(args.data_root, "ShapeNet_mesh")
    if not os.path.isdir(src_dir):
        raise FileNotFoundError("%s is no directory: data_root must hold ShapeNet_mesh/<class>/<model>/model.obj" % src_dir)
    classes = [cl for cl in CLASSES if os.path.isdir(os.path.join(args.split_root, cl))]
    if not classes:
        raise FileNotFoundError("%s holds none of the classes %s" % (args.split_root, ", ".join(CLASSES)))
    mesh_root, save_root = os.path.join(args.data_root, "mesh"), os.path.join(args.data_root, "data")
    os.makedirs(mesh_root, exist_ok=True)
    os.makedirs(save_root, exist_ok=True)
    n_rooms = split_sizes(dataset_size)
    planned = ["%02d_%06d" % (n, r) for n in types for r in range(sum(n_rooms))]
    names = sorted(set(os.listdir(mesh_root)) | set(planned))      # what sorted(os.listdir(mesh)) will be when all are written
    scene_index = {name: i for i, name in enumerate(names)}

    @functools.lru_cache(maxsize=512)
    def load(model):
        cl, m = model.split("/")
        vertices, faces = read_obj(os.path.join(src_dir, cl, m, "model.obj"))
        if len(vertices) == 0 or not np.isfinite(vertices).all() or not (vertices.max(0) - vertices.min(0)).max() > 0:
            raise ValueError("%s holds no extent of finite vertices" % os.path.join(src_dir, cl, m, "model.obj"))
        return vertices, faces

    split_lsts = {name: [] for name in SPLIT_NAMES}
    n_trials = 0
    for type_id, n_object in enumerate(types):
        room_id = 0
        for split_id, split_name in enumerate(SPLIT_NAMES):
            if n_rooms[split_id] == 0:
                continue
            model_files = {cl: read_split_list(args.split_root, cl, split_name) for cl in classes}
            model_files = {cl: models for cl, models in model_files.items() if models}
            if not model_files:
                raise ValueError("%s names no model of split %s" % (args.split_root, split_name))
            split_item_id, j = 0, 0
            while split_item_id < n_rooms[split_id]:
                if j >= MAX_TRIALS_PER_ROOM * n_rooms[split_id]:
                    raise RuntimeError("type %d (%d objects), split %s: %d trials composed %d of %d rooms"
                                       % (type_id, n_object, split_name, j, split_item_id, n_rooms[split_id]))
                trials = [(draw_trial(trial_rng(args.seed, type_id, split_id, jj), model_files, n_object, type_id),
                           trial_seed(args.seed, type_id, split_id, jj)) for jj in range(j, j + args.batch)]
                j += args.batch
                n_trials += args.batch
                for (meta, _), result in zip(trials, compose_batch(trials, load)):
                    if result is None or split_item_id == n_rooms[split_id]:
                        continue
                    name = "%02d_%06d" % (n_object, room_id)
                    item_dict = dict({"room_id": room_id, "split": split_name, "n_object": n_object}, **meta)
                    write_scene(args.data_root, name, item_dict, *result, args.keep_background,
                                (args.n_sample_point, args.n_sample_point_fps), args.seed, scene_index[name])
                    split_lsts[split_name].append(name)
                    room_id += 1
                    split_item_id += 1
    for split_name in SPLIT_NAMES:
        with open(os.path.join(save_root, split_name + ".lst"), "w") as f:
            f.write("\n".join(split_lsts[split_name]))
    n_scene = sum(len(v) for v in split_lsts.values())
    print("build_ogcdr: %d scenes of %d frames written to %s (%d trials composed; train / val / test: %s)"
          % (n_scene, N_FRAME, args.data_root, n_trials, " / ".join(str(len(split_lsts[s])) for s in SPLIT_NAMES)))
    return {"scenes": [n for s in SPLIT_NAMES for n in split_lsts[s]], "lists": {s: list(split_lsts[s]) for s in SPLIT_NAMES}, "trials": n_trials}


if __name__ == "__main__":
    main()
