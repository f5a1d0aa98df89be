"""Seeded synthetic scenes with the reference datasets' sample contract (no datasets travel with the repo).

A sample is the 4-tuple the reference loaders yield (datasets/dataset_kittisf.py:119-122):
``pcs (t, N, 3)``, ``segms (t, N)``, ``flows (t, N, 3)``, ``valids`` — here batched as (B, t, N, ...).
Frame 2 is frame 1 moved by per-object rigid motions (+ noise), re-ordered by a random permutation, so the
flows are exact rigid flows per object, which is what the OGC losses assume.  With ``aug=True`` two more views
are appended: the same two frames under a random similarity transform (the role of ``augment_transform``,
utils/data_util.py:140-195), giving t = 4 as in training with ``aug_transform_epoch`` reached.

Scales: outdoor clouds ``(rand - 0.5) * [60, 4, 80]`` m; object-scale clouds in the unit cube.
"""
import math

import torch


def _rot_y(angle):
    c, s = torch.cos(angle), torch.sin(angle)
    R = torch.zeros(*angle.shape, 3, 3)
    R[..., 0, 0], R[..., 0, 2], R[..., 1, 1], R[..., 2, 0], R[..., 2, 2] = c, s, 1.0, -s, c
    return R


def make_scene_batch(B, N, K, seed=1234, outdoor=True, aug=False, device="cpu", flows=None):
    """`flows` (B, 2, N, 3), when given, replaces the ground-truth flows of the two frames BEFORE the augmented views
    are derived — predicted flows are loaded first and then augmented, as datasets/dataset_kittisf.py:91-117 does."""
    g = torch.Generator().manual_seed(seed)
    scale = torch.tensor([60.0, 4.0, 80.0]) if outdoor else torch.ones(3)
    max_shift, noise = (0.5, 0.01) if outdoor else (0.05, 0.002)
    pc1 = (torch.rand(B, N, 3, generator=g) - 0.5) * scale
    centres = pc1[:, torch.randperm(N, generator=g)[:K]]                              # (B, K, 3)
    segm1 = torch.cdist(pc1, centres).argmin(-1)                                      # (B, N)
    ang = (torch.rand(B, K, generator=g) - 0.5) * 2 * math.radians(5.0)
    R = _rot_y(ang)                                                                   # (B, K, 3, 3)
    shift = (torch.rand(B, K, 3, generator=g) - 0.5) * 2 * max_shift
    Rn = R.gather(1, segm1[:, :, None, None].expand(-1, -1, 3, 3))
    tn = shift.gather(1, segm1[:, :, None].expand(-1, -1, 3))
    cn = centres.gather(1, segm1[:, :, None].expand(-1, -1, 3))
    moved = torch.einsum("bnij,bnj->bni", Rn, pc1 - cn) + cn + tn
    flow1 = moved - pc1
    perm = torch.stack([torch.randperm(N, generator=g) for _ in range(B)])
    pc2 = (moved + torch.randn(B, N, 3, generator=g) * noise).gather(1, perm[:, :, None].expand(-1, -1, 3))
    segm2 = segm1.gather(1, perm)
    flow2 = (-flow1).gather(1, perm[:, :, None].expand(-1, -1, 3))                    # backward flow of frame 2

    if flows is not None:
        flow1, flow2 = flows[:, 0].to(pc1), flows[:, 1].to(pc1)
    pcs, segms, flows = [pc1, pc2], [segm1, segm2], [flow1, flow2]
    if aug:
        s = 0.95 + 0.1 * torch.rand(B, 1, 1, generator=g)
        Ra = _rot_y((torch.rand(B, generator=g) - 0.5) * 2 * math.pi)
        ta = (torch.rand(B, 1, 3, generator=g) - 0.5) * 2 * torch.tensor([1.0, 0.1, 1.0]) * (1.0 if outdoor else 0.05)
        for pc, fl, sg in [(pc1, flow1, segm1), (pc2, flow2, segm2)]:
            pcs.append(s * torch.einsum("bij,bnj->bni", Ra, pc) + ta)
            flows.append(s * torch.einsum("bij,bnj->bni", Ra, fl))
            segms.append(sg)
    pcs = torch.stack(pcs, 1).contiguous().to(device)
    flows = torch.stack(flows, 1).contiguous().to(device)
    segms = torch.stack(segms, 1).contiguous().to(device)
    valids = torch.ones_like(segms, dtype=torch.bool)
    return pcs, segms, flows, valids


def make_sequence(T, N, K, seed=1234, outdoor=True, device="cpu"):
    """One scene observed over T frames — the unit multi-frame voting works on (vote.py:95-131).
    Returns pc (T, N, 3), segm (T, N), flows (T-1, 2, N, 3): flows[t, 0] is the forward flow of frame t (to t+1),
    flows[t, 1] the backward flow of frame t+1 (to t); every step moves each object rigidly, adds noise and re-orders
    the points, as make_scene_batch does for a pair."""
    g = torch.Generator().manual_seed(seed)
    scale = torch.tensor([60.0, 4.0, 80.0]) if outdoor else torch.ones(3)
    max_shift, noise = (0.5, 0.01) if outdoor else (0.05, 0.002)
    pc = (torch.rand(N, 3, generator=g) - 0.5) * scale
    centres = pc[torch.randperm(N, generator=g)[:K]]
    segm = torch.cdist(pc, centres).argmin(-1)
    pcs, segms, flows = [pc], [segm], []
    for _ in range(T - 1):
        R = _rot_y((torch.rand(K, generator=g) - 0.5) * 2 * math.radians(5.0))
        shift = (torch.rand(K, 3, generator=g) - 0.5) * 2 * max_shift
        moved = torch.einsum("nij,nj->ni", R[segm], pc - centres[segm]) + centres[segm] + shift[segm]
        fwd = moved - pc
        perm = torch.randperm(N, generator=g)
        nxt = (moved + torch.randn(N, 3, generator=g) * noise)[perm]
        flows.append(torch.stack([fwd, (-fwd)[perm]]))
        centres = centres + shift
        pc, segm = nxt, segm[perm]
        pcs.append(pc)
        segms.append(segm)
    return torch.stack(pcs).to(device), torch.stack(segms).to(device), torch.stack(flows).to(device)


def make_kitti_raw_scene(N, seed=1234, ground_frac=0.3, n_cluster=48):
    """One full-resolution KITTI-SF style pair as the "processed" layout stores it (datasets/dataset_kittisf.py:73-76): pc1,
    pc2 (N, 3) with points in correspondence, one labelling segm (N,).  A static world — clusters of points above a ground
    sheet at y = -1.65 +- 0.05, i.e. below the -1.4 m the flow-prediction driver cuts at — seen under a small ego-motion
    (rotation about y, translation mostly along z), so the flow pc2 - pc1 is one exact rigid flow.  Also returns the 4x4
    motion, float64."""
    g = torch.Generator().manual_seed(seed)
    n_ground = int(N * ground_frac)
    n_obj = N - n_ground
    centres = (torch.rand(n_cluster, 3, generator=g) - 0.5) * torch.tensor([50.0, 0.0, 50.0]) + torch.tensor([0.0, 0.5, 0.0])
    which = torch.randint(n_cluster, (n_obj,), generator=g)
    obj = centres[which] + torch.randn(n_obj, 3, generator=g) * torch.tensor([0.6, 0.5, 0.6])
    obj[:, 1] = obj[:, 1].clamp(min=-1.2)
    ground = (torch.rand(n_ground, 3, generator=g) - 0.5) * torch.tensor([60.0, 0.1, 60.0]) + torch.tensor([0.0, -1.65, 0.0])
    pc1 = torch.cat([obj, ground])[torch.randperm(N, generator=g)]
    sign = 1.0 if torch.rand(1, generator=g).item() < 0.5 else -1.0
    angle = sign * (0.02 + 0.02 * torch.rand(1, generator=g))
    shift = torch.tensor([0.3, 0.02, 0.4]) * (torch.rand(3, generator=g) - 0.5) * 2 + torch.tensor([0.0, 0.0, 0.8])
    T = torch.eye(4, dtype=torch.float64)
    T[:3, :3], T[:3, 3] = _rot_y(angle)[0].double(), shift.double()
    pc2 = (pc1.double() @ T[:3, :3].T + T[:3, 3]).float()
    return pc1.contiguous(), pc2.contiguous(), torch.zeros(N, dtype=torch.int64), T


def write_kitti_processed_root(root, n_scenes, n_points, seed=1000, split="val"):
    """`n_scenes` scenes of make_kitti_raw_scene under <root>/processed/%06d/{pc1,pc2,segm}.npy and the split file
    <root>/<split>.txt listing their ids — what KITTISceneFlowDataset(root, mapping, downsampled=False) reads.
    Returns (path of the split file, [4x4 motions])."""
    import os

    import numpy as np
    ids, motions = [], []
    for i in range(n_scenes):
        pc1, pc2, segm, T = make_kitti_raw_scene(n_points, seed=seed + i)
        d = os.path.join(root, "processed", "%06d" % i)
        os.makedirs(d, exist_ok=True)
        np.save(os.path.join(d, "pc1.npy"), pc1.numpy())
        np.save(os.path.join(d, "pc2.npy"), pc2.numpy())
        np.save(os.path.join(d, "segm.npy"), segm.numpy())
        ids.append("%06d" % i)
        motions.append(T.numpy())
    mapping = os.path.join(root, split + ".txt")
    with open(mapping, "w") as f:
        f.write("\n".join(ids) + "\n")
    return mapping, motions


def _rot_y_np(angle):
    import numpy as np
    c, s = np.cos(angle), np.sin(angle)
    return np.array([[c, 0.0, s], [0.0, 1.0, 0.0], [-s, 0.0, c]])


WAYMO_SHEET = (0.03, 0.02, -0.2)     # the ground of the synthetic Waymo world: y = 0.03 x + 0.02 z - 0.2 (metres)


def make_waymo_sequence(n_frames, n_points, seed=2000, ground_frac=0.6, n_boxes=8):
    """One synthetic Waymo-style sequence: a static world — boxes standing on a TILTED ground sheet (3 cm / m in x, 2 cm / m in
    z, so that a height threshold alone mislabels part of the ground) — in front of and beside a sensor that drives along +z under known
    poses (yaw and translation in the ground plane; y is up and the sensor stays at y = 0).  Guaranteed gaps: every ground point
    lies within 0.1 m of the sheet, every other point at least 0.6 m above it (and above y = 0.35).  Every frame samples the
    world anew with its own number of points (n_points +- 5 %), so frames are not in correspondence.
    Returns a list of frames {pc (N, 3) f32 in sensor coordinates, segm (N,) i32 instance ids (0: ground), semantic_segm (N,)
    i32 class ids (0: ground, 1 / 2: boxes), ground (N,) bool, pose (4, 4) f64 sensor-to-world}."""
    import numpy as np
    rs = np.random.RandomState(seed)
    a, b, c0 = WAYMO_SHEET
    centres = np.stack([(rs.rand(n_boxes) - 0.5) * 40.0, np.zeros(n_boxes), 6.0 + rs.rand(n_boxes) * 22.0], 1)
    sizes = np.stack([1.5 + 2.0 * rs.rand(n_boxes), 1.2 + 1.5 * rs.rand(n_boxes), 1.5 + 2.5 * rs.rand(n_boxes)], 1)
    classes = 1 + (np.arange(n_boxes) % 4 == 3).astype(np.int32)
    frames, yaw, position = [], 0.0, np.zeros(3)
    for t in range(n_frames):
        pose = np.eye(4)
        pose[:3, :3], pose[:3, 3] = _rot_y_np(yaw), position
        n = n_points + int(rs.randint(-(n_points // 20), n_points // 20 + 1))
        n_ground = int(n * ground_frac)
        # ground: uniform around the sensor, within 0.08 m of the sheet
        gx = position[0] + (rs.rand(n_ground) - 0.5) * 60.0
        gz = position[2] + (rs.rand(n_ground) - 0.5) * 60.0
        ground = np.stack([gx, a * gx + b * gz + c0 + (rs.rand(n_ground) - 0.5) * 0.16, gz], 1)
        # boxes: points inside their footprint, from 0.6 m above the sheet (and y = 0.35) upwards
        which = rs.randint(n_boxes, size=n - n_ground)
        bx = centres[which, 0] + (rs.rand(n - n_ground) - 0.5) * sizes[which, 0]
        bz = centres[which, 2] + (rs.rand(n - n_ground) - 0.5) * sizes[which, 2]
        by = np.maximum(a * bx + b * bz + c0 + 0.6, 0.35) + rs.rand(n - n_ground) * sizes[which, 1]
        world = np.concatenate([ground, np.stack([bx, by, bz], 1)])
        segm = np.concatenate([np.zeros(n_ground, np.int32), (which + 1).astype(np.int32)])
        perm = rs.permutation(n)
        world, segm = world[perm], segm[perm]
        pc = ((world - position) @ pose[:3, :3]).astype(np.float32)         # R^T (w - t), row-wise
        frames.append({"pc": pc, "segm": segm, "semantic_segm": np.where(segm > 0, classes[np.maximum(segm, 1) - 1], 0).astype(np.int32),
                       "ground": segm == 0, "pose": pose})
        yaw += (rs.rand() - 0.5) * 0.04
        position = position + np.array([(rs.rand() - 0.5) * 0.2, 0.0, 0.6 + 0.4 * rs.rand()])
    return frames


def write_waymo_root(root, n_sequences, n_frames, n_points, seed=2000, split="val"):
    """`n_sequences` sequences of make_waymo_sequence under <root>/data/seq_%04d/{pc,segm,semantic_segm,ground,pose}_%04d.npy
    with the backward flows flow_%04d_%04d.npy (t, t - 1) — the rigid flow of frame t towards frame t - 1, the world being
    static — and the split file <root>/<split>.txt: what WaymoOpenDataset(root, mapping) reads.
    Returns (path of the split file, {sequence name: [4x4 poses]})."""
    import os

    import numpy as np
    names, poses = [], {}
    for k in range(n_sequences):
        name = "seq_%04d" % k
        frames = make_waymo_sequence(n_frames, n_points, seed=seed + k)
        d = os.path.join(root, "data", name)
        os.makedirs(d, exist_ok=True)
        for t, frame in enumerate(frames):
            for what in ("pc", "segm", "semantic_segm", "ground", "pose"):
                np.save(os.path.join(d, "%s_%04d.npy" % (what, t)), frame[what])
            if t >= 1:
                p1, p2 = frame["pose"], frames[t - 1]["pose"]
                rot, transl = p2[:3, :3].T @ p1[:3, :3], p2[:3, :3].T @ (p1[:3, 3] - p2[:3, 3])
                pc = frame["pc"].astype(np.float64)
                np.save(os.path.join(d, "flow_%04d_%04d.npy" % (t, t - 1)), (pc @ rot.T + transl - pc).astype(np.float32))
        names.append(name)
        poses[name] = [f["pose"] for f in frames]
    mapping = os.path.join(root, split + ".txt")
    with open(mapping, "w") as f:
        f.write("\n".join(names) + "\n")
    return mapping, poses


def write_waymo_singleframe_roots(root, n_train, n_val, n_frames, n_points, seed=8000, small_object=20):
    """Single-frame Waymo data for the supervised Waymo trainer and the Waymo evaluation (WaymoSingleFrameDataset with
    downsampled=True): sequences of make_waymo_sequence under <root>/data/<split>_%04d/{pc,segm,semantic_segm}_%04d.npy, every
    frame cut to exactly `n_points` points so that frames batch, with what makes the reader's ignore mask non-empty whatever the
    threshold: box 4 is of class 2 (make_waymo_sequence's), box 2 becomes class 3, and `small_object` points of box 1 in every
    frame become an object of their own (id n_boxes + 1, class 1) that a threshold above `small_object` drops.
    Writes <root>/train.txt and <root>/val.txt (one name listed in each is not on disk: the readers pass over it) and
    <root>/train_select.json / val_select.json with every second frame as [sequence, t].
    Returns {"train": {"mapping", "select_frame", "names"}, "val": {...}}."""
    import json
    import os

    import numpy as np
    out, k = {}, 0
    os.makedirs(root, exist_ok=True)
    for split, n_sequences in (("train", n_train), ("val", n_val)):
        names = []
        for _ in range(n_sequences):
            name = "%s_%04d" % (split, len(names))
            frames = make_waymo_sequence(n_frames, n_points + n_points // 19 + 2, seed=seed + k)   # n - 5 % >= n_points
            k += 1
            d = os.path.join(root, "data", name)
            os.makedirs(d, exist_ok=True)
            for t, frame in enumerate(frames):
                pc, segm, semantic = (frame[what][:n_points].copy() for what in ("pc", "segm", "semantic_segm"))
                assert pc.shape[0] == n_points
                semantic[segm == 2] = 3
                fragment = np.nonzero(segm == 1)[0][:small_object]
                segm[fragment] = int(frame["segm"].max()) + 1
                for what, value in (("pc", pc), ("segm", segm), ("semantic_segm", semantic)):
                    np.save(os.path.join(d, "%s_%04d.npy" % (what, t)), value)
            names.append(name)
        mapping, select = os.path.join(root, split + ".txt"), os.path.join(root, split + "_select.json")
        with open(mapping, "w") as f:
            f.write("\n".join(["%s.tfrecord" % n for n in names] + ["%s_absent.tfrecord" % split]) + "\n")
        with open(select, "w") as f:
            json.dump([[n, t] for n in names for t in range(0, n_frames, 2)], f)
        out[split] = {"mapping": mapping, "select_frame": select, "names": names}
    return out


def write_waymo_moving_root(root, n_sequences, n_frames, n_points, n_sample_point, seed=9400, split="train", n_boxes=4, n_moving=3, ground_frac=0.2,
                            small_object=12, short_frame=("seq_0000", 2)):
    """A full-resolution Waymo root for the preparation chain filter_empty -> downsample_waymo -> select_mov, in the layout of
    write_waymo_root with the poses and float64 flows process_waymo writes.  Sequences of make_waymo_sequence with `n_boxes` boxes
    and `ground_frac` of the points on the ground (few, so that furthest point sampling, which spreads over the 60 m of ground,
    still leaves the compact boxes some tens of points each);
    in the sequences of EVEN number the boxes 1 .. n_moving drive through the static world, box k by velocity[k] per frame, 0.5 to
    0.9 m in the ground plane: their points of frame t are displaced by t * velocity (seen from the sensor), and the stored
    backward flow is the rigid flow of the displaced point minus the velocity seen from frame t - 1 — where the point was one
    frame earlier.  The sequences of odd number stay static: their flows are the rigid flows of write_waymo_root.
    In every frame `small_object` points of the last box become an object of their own (id n_boxes + 1, class 1), and frame
    `short_frame` = (sequence, t) is cut to n_sample_point - n_sample_point // 8 points, fewer than the sample count.  Every other
    frame has at least n_sample_point points (n_points - 5 % must reach it).
    Returns {"mapping": the split file, "names", "moving": names of the moving sequences, "short_frame", "velocity": {name: (n_boxes + 2, 3)}}."""
    import os

    import numpy as np
    assert n_points - n_points // 20 >= n_sample_point and 0 < n_moving <= n_boxes
    names, moving, velocities = [], [], {}
    for k in range(n_sequences):
        name = "seq_%04d" % k
        frames = make_waymo_sequence(n_frames, n_points, seed=seed + k, ground_frac=ground_frac, n_boxes=n_boxes)
        rs = np.random.RandomState(seed + 1000 + k)
        velocity = np.zeros((n_boxes + 2, 3))
        if k % 2 == 0:
            angle, speed = rs.rand(n_moving) * 2.0 * np.pi, 0.5 + 0.4 * rs.rand(n_moving)
            velocity[1:n_moving + 1] = np.stack([speed * np.cos(angle), np.zeros(n_moving), speed * np.sin(angle)], 1)
            moving.append(name)
        velocities[name] = velocity
        d = os.path.join(root, "data", name)
        os.makedirs(d, exist_ok=True)
        for t, frame in enumerate(frames):
            pc, segm, semantic = frame["pc"].copy(), frame["segm"].copy(), frame["semantic_segm"].copy()
            if (name, t) == tuple(short_frame):
                cut = n_sample_point - n_sample_point // 8
                pc, segm, semantic = pc[:cut], segm[:cut], semantic[:cut]
            rot_t = frame["pose"][:3, :3]
            pc = (pc.astype(np.float64) + t * (velocity[segm] @ rot_t)).astype(np.float32)      # R^T v, row-wise
            fragment = np.nonzero(segm == n_boxes)[0][:small_object]
            stored_segm = segm.copy()
            stored_segm[fragment], semantic[fragment] = n_boxes + 1, 1
            for what, value in (("pc", pc), ("segm", stored_segm), ("semantic_segm", semantic), ("pose", frame["pose"])):
                np.save(os.path.join(d, "%s_%04d.npy" % (what, t)), value)
            if t >= 1:
                p1, p2 = frame["pose"], frames[t - 1]["pose"]
                rot, transl = p2[:3, :3].T @ p1[:3, :3], p2[:3, :3].T @ (p1[:3, 3] - p2[:3, 3])
                p = pc.astype(np.float64)
                np.save(os.path.join(d, "flow_%04d_%04d.npy" % (t, t - 1)), p @ rot.T + transl - p - velocity[segm] @ p2[:3, :3])
        names.append(name)
    mapping = os.path.join(root, split + ".txt")
    with open(mapping, "w") as f:
        f.write("\n".join(names) + "\n")
    return {"mapping": mapping, "names": names, "moving": moving, "short_frame": tuple(short_frame), "velocity": velocities}


LABELLED_LAYOUTS = ("kittisf", "kittidet", "semantickitti")
SYNTHETIC_SEQUENCES = (0, 8, 12)   # synthetic frames cycle through these; test_seg evaluates sequences 0..10


def write_labelled_root(root, layout, n_scenes, n_points, n_objects, seed=3000, split="val"):
    """`n_scenes` outdoor scenes of make_scene_batch (objects = Voronoi cells of random centres, rigid motion per object) with
    their labels, in the layout a segmentation data set of ogc_amd/datasets.py reads:
      kittisf         <root>/data/%06d/{pc,segm,flow}{1,2}.npy, <root>/<split>.txt    (KITTISceneFlowDataset, downsampled=True)
      kittidet        <root>/downsampled/%06d/{pc,segm}.npy, <root>/<split>.txt       (KITTIDetectionDataset; frame 1 only)
      semantickitti   <root>/downsampled/<ss>_%06d/{pc,segm}.npy, ss cycling through SYNTHETIC_SEQUENCES, no split file
    Labels are written as 2 * object + 1, with gaps, so that a reader has something to compress.
    Returns (path of the split file or None, [ids])."""
    import os

    import numpy as np
    if layout not in LABELLED_LAYOUTS:
        raise KeyError("write_labelled_root covers %s, got %r" % (", ".join(LABELLED_LAYOUTS), layout))
    ids = []
    for i in range(n_scenes):
        pcs, segms, flows, _ = make_scene_batch(1, n_points, n_objects, seed=seed + i, outdoor=True)
        pcs, segms, flows = pcs[0].numpy(), (2 * segms[0] + 1).numpy().astype(np.int32), flows[0].numpy()
        if layout == "kittisf":
            name = "%06d" % i
            d = os.path.join(root, "data", name)
            os.makedirs(d, exist_ok=True)
            for v in (0, 1):
                np.save(os.path.join(d, "pc%d.npy" % (v + 1)), pcs[v])
                np.save(os.path.join(d, "segm%d.npy" % (v + 1)), segms[v])
                np.save(os.path.join(d, "flow%d.npy" % (v + 1)), flows[v])
        else:
            sequence = SYNTHETIC_SEQUENCES[i % len(SYNTHETIC_SEQUENCES)]
            name = "%06d" % i if layout == "kittidet" else "%02d_%06d" % (sequence, i)
            d = os.path.join(root, "downsampled", name)
            os.makedirs(d, exist_ok=True)
            np.save(os.path.join(d, "pc.npy"), pcs[0])
            np.save(os.path.join(d, "segm.npy"), segms[0])
        ids.append(name)
    if layout == "semantickitti":
        return None, ids
    mapping = os.path.join(root, split + ".txt")
    with open(mapping, "w") as f:
        f.write("\n".join(ids) + "\n")
    return mapping, ids


def _sequence_scene(n_frames, n_points, n_objects, seed):
    """An object-scale scene for the two four-frame layouts: `n_objects` blobs in the unit cube (labels 1..n_objects) in front of
    a static background (label 0, about a quarter of the points), every object under its own 4x4 object-to-world motion per
    frame (a rotation of a few degrees about y and a shift of a few centimetres from frame to frame).  Every frame holds the
    SAME canonical points in its own order.  Returns canon (N, 3) f64, label (N,) i32, motions (n_frames, n_objects, 4, 4) f64,
    perms (n_frames, N)."""
    import numpy as np
    rs = np.random.RandomState(seed)
    label = rs.randint(0, n_objects + 1, size=n_points).astype(np.int32)
    label[rs.rand(n_points) < 0.1] = 0
    centres = (rs.rand(n_objects + 1, 3) - 0.5) * 0.8
    canon = centres[label] + rs.randn(n_points, 3) * 0.06
    canon[label == 0] = (rs.rand(int((label == 0).sum()), 3) - 0.5) * np.array([1.0, 0.05, 1.0]) - np.array([0.0, 0.5, 0.0])
    motions = np.zeros((n_frames, n_objects, 4, 4))
    yaw, shift = np.zeros(n_objects), centres[1:].copy()
    for t in range(n_frames):
        for k in range(n_objects):
            motions[t, k] = np.eye(4)
            motions[t, k, :3, :3], motions[t, k, :3, 3] = _rot_y_np(yaw[k]), shift[k]
        yaw = yaw + (rs.rand(n_objects) - 0.5) * 2 * math.radians(8.0)
        shift = shift + (rs.rand(n_objects, 3) - 0.5) * 0.1
    perms = np.stack([rs.permutation(n_points) for _ in range(n_frames)])
    return canon - np.where(label[:, None] > 0, centres[label], 0.0), label, motions, perms


def _apply_4x4(m, pc):
    return pc @ m[:3, :3].T + m[:3, 3]


def write_ogcdr_root(root, n_scenes, n_points, n_objects=3, n_frames=4, seed=4000, split="val"):
    """`n_scenes` scenes of `n_frames` frames in the OGC-DR layout: <root>/data/<id>/{pc,segm,pose}_%02d.npy — pc (N, 3) f32,
    segm (N,) i32 (0: background), pose (n_objects, 4, 4) f64 object-to-world — and <root>/data/<split>.lst, exactly what
    OGCDynamicRoomDataset(root, split) reads; the flow it computes from the poses moves every object rigidly onto its place in
    the other frame.  Returns [ids]."""
    import os

    import numpy as np
    ids = []
    for i in range(n_scenes):
        canon, label, motions, perms = _sequence_scene(n_frames, n_points, n_objects, seed + i)
        name = "%08d" % i
        d = os.path.join(root, "data", name)
        os.makedirs(d, exist_ok=True)
        for t in range(n_frames):
            pc = canon.copy()
            for k in range(n_objects):
                pc[label == k + 1] = _apply_4x4(motions[t, k], canon[label == k + 1])
            np.save(os.path.join(d, "pc_%02d.npy" % t), pc[perms[t]].astype(np.float32))
            np.save(os.path.join(d, "segm_%02d.npy" % t), label[perms[t]])
            np.save(os.path.join(d, "pose_%02d.npy" % t), motions[t])
        ids.append(name)
    with open(os.path.join(root, "data", split + ".lst"), "w") as f:
        f.write("\n".join(ids) + "\n")
    return ids


def write_sapien_root(root, n_scenes, n_points, n_parts=3, n_frames=4, seed=5000, split="val"):
    """`n_scenes` articulated objects of `n_parts` parts seen in `n_frames` frames in the SAPIEN layout: <root>/meta.json
    {split: [integer ids]} and <root>/data/%06d.npz with pc (V, N, 3) f32 in each frame's CAMERA coordinates, segm (V, N) i32
    (0: no part) and trans {"cam": (V, 4, 4), part id: (V, 4, 4)} (camera-to-world, part-to-world) — exactly what
    SapienDataset(root, split) reads; its flow is cam_b^-1 . M_b . M_a^-1 . cam_a applied per part.  Points of no part are given
    to part 1 here: the reader leaves their flow at zero, which would not be a motion of the moving camera's frame.
    Returns [ids]."""
    import json
    import os

    import numpy as np
    ids = []
    os.makedirs(os.path.join(root, "data"), exist_ok=True)
    for i in range(n_scenes):
        canon, label, motions, perms = _sequence_scene(n_frames, n_points, n_parts, seed + i)
        label = np.where(label == 0, 1, label).astype(np.int32)
        rs = np.random.RandomState(seed + 7919 * (i + 1))
        cams = np.zeros((n_frames, 4, 4))
        for t in range(n_frames):
            cams[t] = np.eye(4)
            cams[t, :3, :3] = _rot_y_np((rs.rand() - 0.5) * 2 * math.radians(10.0))
            cams[t, :3, 3] = (rs.rand(3) - 0.5) * 0.1
        pcs = np.zeros((n_frames, n_points, 3))
        for t in range(n_frames):
            inv = np.linalg.inv(cams[t])
            for k in range(n_parts):
                sel = label == k + 1
                pcs[t, sel] = _apply_4x4(inv, _apply_4x4(motions[t, k], canon[sel]))
        # one order for all frames: the npz holds (V, N) arrays and the reader indexes them by frame
        trans = {k + 1: motions[:, k].copy() for k in range(n_parts)}
        trans["cam"] = cams
        np.savez(os.path.join(root, "data", "%06d.npz" % i), pc=pcs[:, perms[0]].astype(np.float32),
                 segm=np.stack([label[perms[0]]] * n_frames), trans=np.array(trans, dtype=object))
        ids.append(i)
    with open(os.path.join(root, "meta.json"), "w") as f:
        json.dump({split: ids}, f)
    return ids


def write_kitti_downsampled_root(full_root, down_root, n_points, predflow=None, seed=6000, split="val"):
    """The down-sampled twin of a root written by write_kitti_processed_root, in the layout KITTISceneFlowDataset(down_root,
    mapping, downsampled=True) reads: per scene `n_points` random points of each frame (their own subset per frame) as
    <down_root>/data/<id>/{pc,segm,flow}{1,2}.npy, the flows being the scan's own pc2 - pc1 and pc1 - pc2 at those points, and
    <down_root>/<split>.txt.  With `predflow` the same flows are stored once more as predictions,
    <down_root>/flow_preds/<predflow>/<id>/flow{1,2}.npy.  Returns (path of the split file, [ids])."""
    import os

    import numpy as np

    from . import flow_store
    with open(os.path.join(full_root, split + ".txt")) as f:
        ids = f.read().strip().split("\n")
    rs = np.random.RandomState(seed)
    for name in ids:
        src = os.path.join(full_root, "processed", name)
        pc1, pc2, segm = (np.load(os.path.join(src, what + ".npy")) for what in ("pc1", "pc2", "segm"))
        d = os.path.join(down_root, "data", name)
        os.makedirs(d, exist_ok=True)
        flows = []
        for v, (pc, other) in enumerate(((pc1, pc2), (pc2, pc1))):
            sel = rs.choice(pc.shape[0], size=min(n_points, pc.shape[0]), replace=False)
            np.save(os.path.join(d, "pc%d.npy" % (v + 1)), pc[sel])
            np.save(os.path.join(d, "segm%d.npy" % (v + 1)), segm[sel])
            np.save(os.path.join(d, "flow%d.npy" % (v + 1)), other[sel] - pc[sel])
            flows.append(other[sel] - pc[sel])
        if predflow is not None:
            flow_store.save_pair(os.path.join(down_root, "flow_preds", predflow), name, flows[0], flows[1])
    mapping = os.path.join(down_root, split + ".txt")
    with open(mapping, "w") as f:
        f.write("\n".join(ids) + "\n")
    return mapping, ids


SUPERVISED_LAYOUTS = ("sapien", "ogcdr", "kittisf", "kittidet")


def write_supervised_roots(root, dataset, n_train, n_val, n_points, n_objects, seed=7000):
    """A labelled training and a validation set for the supervised trainer (train_seg_sup.py), each under its own directory
    (the writers number their scenes from 0): <root>/train and <root>/val in the layout `dataset`'s reader takes — kittisf and
    kittidet by write_labelled_root, ogcdr by write_ogcdr_root, sapien by write_sapien_root.  n_objects counts the moving
    objects; the four-frame layouts add a background.  Returns {split: (data root, path of the split file or None)}."""
    import os
    if dataset not in SUPERVISED_LAYOUTS:
        raise KeyError("write_supervised_roots covers %s, got %r" % (", ".join(SUPERVISED_LAYOUTS), dataset))
    out = {}
    for split, n_scenes, s in (("train", n_train, seed), ("val", n_val, seed + 100003)):
        sub = os.path.join(root, split)
        os.makedirs(sub, exist_ok=True)
        mapping = None
        if dataset in ("kittisf", "kittidet"):
            mapping, _ = write_labelled_root(sub, dataset, n_scenes, n_points, n_objects, seed=s, split=split)
        elif dataset == "ogcdr":
            write_ogcdr_root(sub, n_scenes, n_points, n_objects=n_objects, seed=s, split=split)
        else:
            write_sapien_root(sub, n_scenes, n_points, n_parts=n_objects, seed=s, split=split)
        out[split] = (sub, mapping)
    return out


# ---- raw roots for the preparation drivers (ogc_amd/data_prepare) ----------------------------------------------------------
RAW_MARGIN = 0.05            # object points lie this far inside their box, all others this far outside every relaxed box
RAW_RELAX = 0.01             # the `relax` of the reference's box tests
KITTI_IMAGE_SIZE = (1242, 375)


def _rot_x_np(angle):
    import numpy as np
    c, s = np.cos(angle), np.sin(angle)
    return np.array([[1.0, 0.0, 0.0], [0.0, c, -s], [0.0, s, c]])


def _rot_z_np(angle):
    import numpy as np
    c, s = np.cos(angle), np.sin(angle)
    return np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])


def _written(values):
    """What a reader gets back from numbers written with %.12e."""
    import numpy as np
    return np.array([float("%.12e" % v) for v in np.asarray(values, dtype=np.float64).reshape(-1)])


def make_kitti_calibration(seed, with_r0=True):
    """A KITTI-like calibration as the numbers a calib file holds: P2 (3, 4) a 721-px pinhole with a baseline term, V2C (3, 4)
    the velodyne frame (x forward, y left, z up) turned into the camera's (x right, y down, z forward) under a tilt of a degree
    or so and a lever arm, R0 (3, 3) a rectifying rotation of a few milliradians (None without)."""
    import numpy as np
    rs = np.random.RandomState(seed)
    axes = np.array([[0.0, -1.0, 0.0], [0.0, 0.0, -1.0], [1.0, 0.0, 0.0]])
    tilt = _rot_x_np((rs.rand() - 0.5) * 0.03) @ _rot_y_np((rs.rand() - 0.5) * 0.03) @ _rot_z_np((rs.rand() - 0.5) * 0.03)
    V2C = np.concatenate([tilt @ axes, np.array([[-0.004], [-0.076], [-0.272]]) + (rs.rand(3, 1) - 0.5) * 0.01], 1)
    P = np.array([[721.5377, 0.0, 609.5593, 44.85728], [0.0, 721.5377, 172.854, 0.2163791], [0.0, 0.0, 1.0, 0.002745884]])
    calib = {"P": _written(P).reshape(3, 4), "V2C": _written(V2C).reshape(3, 4)}
    if with_r0:
        R0 = _rot_x_np((rs.rand() - 0.5) * 0.02) @ _rot_y_np((rs.rand() - 0.5) * 0.02) @ _rot_z_np((rs.rand() - 0.5) * 0.02)
        calib["R0"] = _written(R0).reshape(3, 3)
    return calib


def _rect_to_velo(rect, calib):
    """Camera (rect) coordinates -> velodyne coordinates, float64."""
    import numpy as np
    ref = rect @ np.linalg.inv(calib["R0"]).T if calib.get("R0") is not None else rect
    return (ref - calib["V2C"][:, 3]) @ np.linalg.inv(calib["V2C"][:, :3]).T


def _camera_scene(n_points, rs, objects):
    """Points of one camera frame in RECT coordinates (x right, y down, z forward; the camera 1.65 m above the ground) and their
    object index (0: none).  `objects` is a list of (l, w, h, (tx, ty, tz), ry) — t the bottom centre, as a KITTI label — whose
    boxes do not come within 2 * RAW_MARGIN + 2 * RAW_RELAX of one another.  A third of the points lies RAW_MARGIN inside the
    objects, the rest on the ground and in clutter over a region wider than the crop on every side, RAW_MARGIN outside every
    relaxed box."""
    import numpy as np
    n_obj = n_points // 3
    which = rs.randint(len(objects), size=n_obj)
    pts, labels = [], []
    for k, (l, w, h, t, ry) in enumerate(objects):
        m = int((which == k).sum())
        half = np.array([l / 2 - RAW_MARGIN, 0.0, w / 2 - RAW_MARGIN])
        local = (rs.rand(m, 3) - 0.5) * 2 * half
        local[:, 1] = -RAW_MARGIN - rs.rand(m) * (h - 2 * RAW_MARGIN)
        pts.append(local @ _rot_y_np(ry).T + np.asarray(t))
        labels.append(np.full(m, k + 1, dtype=np.int32))
    n_bg = n_points - n_obj
    z = -5.0 + 50.0 * rs.rand(n_bg)
    x = np.where(rs.rand(n_bg) < 0.8, z * (rs.rand(n_bg) - 0.5) * 1.9, (rs.rand(n_bg) - 0.5) * 60.0)
    y = np.where(rs.rand(n_bg) < 0.6, 1.65 + (rs.rand(n_bg) - 0.5) * 0.06, 1.6 - 2.6 * rs.rand(n_bg))
    bg = np.stack([x, y, z], 1)
    free = np.ones(n_bg, dtype=bool)
    grow = RAW_RELAX + RAW_MARGIN + 0.01
    for l, w, h, t, ry in objects:
        q = (bg - np.asarray(t)) @ _rot_y_np(-ry).T
        free &= ~((np.abs(q[:, 0]) < l / 2 + grow) & (q[:, 1] > -h - grow) & (q[:, 1] < grow) & (np.abs(q[:, 2]) < w / 2 + grow))
    pts.append(bg[free])
    labels.append(np.zeros(int(free.sum()), dtype=np.int32))
    pts, labels = np.concatenate(pts), np.concatenate(labels)
    perm = rs.permutation(pts.shape[0])
    return pts[perm], labels[perm]


def _camera_objects(rs, n):
    """n upright boxes (l, w, h, t, ry) on the ground in front of the camera, one per 7-m slot, so that none comes near another;
    every number has the two decimals a label file keeps."""
    import numpy as np
    slots = [(x, z) for z in (10.0, 17.0, 24.0, 31.0) for x in (-7.0, 0.0, 7.0) if abs(x) < 0.55 * z]
    order = rs.permutation(len(slots))[:n]

    def r2(v):
        return float("%.2f" % v)
    return [(r2(3.2 + 1.2 * rs.rand()), r2(1.5 + 0.4 * rs.rand()), r2(1.4 + 0.4 * rs.rand()),
             (r2(slots[i][0] + rs.rand() - 0.5), 1.65, r2(slots[i][1] + rs.rand() - 0.5)), r2((rs.rand() - 0.5) * 2 * np.pi))
            for i in order]


def _calib_lines(entries):
    import numpy as np
    return "".join("%s: %s\n" % (key, " ".join("%.12e" % v for v in np.asarray(value, dtype=np.float64).reshape(-1)))
                   for key, value in entries)


def write_kittidet_raw_root(root, n_frames, n_points, seed=9000):
    """`n_frames` raw KITTI-Det frames under <root>/training: velodyne/%06d.bin (N, 4) f32, calib/%06d.txt (P0 .. P3, R0_rect,
    Tr_velo_to_cam, Tr_imu_to_velo), label_2/%06d.txt (a Pedestrian, three Cars and a DontCare line, in an order that gives the
    Cars the ids 2, 4, 5) and image_2/%06d.png, a blank 1242 x 375 — what process_kittidet reads.  Returns a list of frames
    {"calib": the matrices as the file holds them, "labels": (N,) i32 the label-line id of the Car a point lies in, else 0
    (the Pedestrian's points included), "objects": per label line (type, h, w, l, tx, ty, tz, ry) as the line holds them}."""
    import os

    import numpy as np
    from PIL import Image
    base = os.path.join(root, "training")
    for sub in ("velodyne", "calib", "label_2", "image_2"):
        os.makedirs(os.path.join(base, sub), exist_ok=True)
    frames = []
    for i in range(n_frames):
        rs = np.random.RandomState(seed + i)
        calib = make_kitti_calibration(seed + i)
        boxes = _camera_objects(rs, 4)
        types = ["Pedestrian", "Car", "DontCare", "Car", "Car"]
        rect, which = _camera_scene(n_points, rs, boxes)
        line_of_box = [0, 1, 3, 4]                                      # the label line of box k
        labels = np.zeros(rect.shape[0], dtype=np.int32)
        for k in (1, 2, 3):
            labels[which == k + 1] = line_of_box[k] + 1
        velo = _rect_to_velo(rect, calib)
        scan = np.concatenate([velo, rs.rand(velo.shape[0], 1)], 1).astype(np.float32)
        scan.tofile(os.path.join(base, "velodyne", "%06d.bin" % i))
        with open(os.path.join(base, "calib", "%06d.txt" % i), "w") as f:
            f.write(_calib_lines([("P0", calib["P"]), ("P1", calib["P"]), ("P2", calib["P"]), ("P3", calib["P"]),
                                  ("R0_rect", calib["R0"]), ("Tr_velo_to_cam", calib["V2C"]), ("Tr_imu_to_velo", np.eye(3, 4))]))
        lines, objects, b = [], [], 0
        for kind in types:
            if kind == "DontCare":
                lines.append("DontCare -1 -1 -10 503.89 169.71 590.61 190.13 -1 -1 -1 -1000 -1000 -1000 -10")
                objects.append(("DontCare", -1.0, -1.0, -1.0, -1000.0, -1000.0, -1000.0, -10.0))
                continue
            l, w, h, t, ry = boxes[b]
            b += 1
            text = "%s 0.00 0 -1.57 100.00 120.00 300.00 220.00 %.2f %.2f %.2f %.2f %.2f %.2f %.2f" % (kind, h, w, l, t[0], t[1], t[2], ry)
            lines.append(text)
            objects.append((kind,) + tuple(float(v) for v in text.split(" ")[8:15]))
        with open(os.path.join(base, "label_2", "%06d.txt" % i), "w") as f:
            f.write("\n".join(lines) + "\n")
        Image.new("RGB", KITTI_IMAGE_SIZE).save(os.path.join(base, "image_2", "%06d.png" % i))
        frames.append({"calib": calib, "labels": labels, "objects": objects})
    return frames


SEMANTICKITTI_OBJECTS = ((10, 1), (252, 2), (18, 1), (30, 1))   # (class, instance) of the four objects: car, moving-car, truck, person
SEMANTICKITTI_GROUND = 40                                       # road, instance 0


def write_semantickitti_raw_root(root, n_frames, n_points, sequences=(0,), seed=9100):
    """Raw SemanticKITTI sequences under <root>/sequences/%02d: velodyne/%06d.bin (N, 4) f32, labels/%06d.label (N,) 32-bit words
    — the class in the low half, the instance id in the high half: four objects of SEMANTICKITTI_OBJECTS, of which the person is
    not among the classes the preparation keeps, and road — and one calib.txt (P0 .. P3, Tr; no R0) — what process_semantickitti
    reads.  Returns {sequence: {"calib": the matrices as the file holds them, "labels": [per frame the (N,) i32 label words]}}."""
    import os

    import numpy as np
    out = {}
    for s, sequence in enumerate(sequences):
        base = os.path.join(root, "sequences", "%02d" % sequence)
        for sub in ("velodyne", "labels"):
            os.makedirs(os.path.join(base, sub), exist_ok=True)
        calib = make_kitti_calibration(seed + 1000 * s, with_r0=False)
        with open(os.path.join(base, "calib.txt"), "w") as f:
            f.write(_calib_lines([("P0", calib["P"]), ("P1", calib["P"]), ("P2", calib["P"]), ("P3", calib["P"]), ("Tr", calib["V2C"])]))
        words = np.array([SEMANTICKITTI_GROUND] + [c | (i << 16) for c, i in SEMANTICKITTI_OBJECTS], dtype=np.int32)
        labels = []
        for i in range(n_frames):
            rs = np.random.RandomState(seed + 1000 * s + i + 1)
            rect, which = _camera_scene(n_points, rs, _camera_objects(rs, len(SEMANTICKITTI_OBJECTS)))
            scan = np.concatenate([_rect_to_velo(rect, calib), rs.rand(rect.shape[0], 1)], 1).astype(np.float32)
            scan.tofile(os.path.join(base, "velodyne", "%06d.bin" % i))
            words[which].tofile(os.path.join(base, "labels", "%06d.label" % i))
            labels.append(words[which])
        out[sequence] = {"calib": calib, "labels": labels}
    return out


WAYMO_CLASSES = ("Vehicle", "Pedestrian", "Cyclist")
# the boxes of a synthetic raw Waymo sequence, in this order: (name, counted points; 0 = annotated as empty).  Labelled are the
# first five; `unknown`, the box annotated as empty and the Sign hold points too, which must come out unlabelled.
WAYMO_RAW_BOXES = (("Vehicle", 1), ("Vehicle", 1), ("Pedestrian", 1), ("Cyclist", 1), ("Vehicle", 1), ("unknown", 1), ("Vehicle", 0),
                   ("Sign", 1))


def write_waymo_raw_root(root, n_sequences, n_frames, n_points, seed=9200, data_tag="waymo_processed_data", flow_tag="scene_flow",
                         split="train", box_dtype="float64"):
    """Raw Waymo sequences as the info-file pipeline leaves them: <root>/<data_tag>/<seq>/<seq>.pkl, a list of frame infos
    {point_cloud: {lidar_sequence, sample_idx}, pose (4, 4) f64 sensor-to-world, annos: {name, gt_boxes_lidar (K, 7) [x, y, z, l, w,
    h, heading], obj_ids, num_points_in_gt}}, <root>/<data_tag>/<seq>/%04d.npy (N, 6) f32 [x, y, z, intensity, elongation, NLZ
    flag] in lidar coordinates (x forward, y left, z up) and <root>/<flow_tag>/<seq>/%04d.npy (N, 4) f32 velocities in m/s, plus
    <root>/<split>.txt with the names as `<seq>.tfrecord` and one name that is not on disk — what process_waymo reads.
    The world is static but for box 4, which drives along x; the sensor moves under known poses (yaw about z, shift in the
    plane).  Every frame samples the world anew: a ground sheet at z = -1.8 wider than every range test, the boxes of
    WAYMO_RAW_BOXES filled RAW_MARGIN inside the extents the reference tests (l on x, h on y, w on z), in a per-frame order of the
    annotations, and about a tenth of the points flagged out through column 5.
    Returns {seq: [per frame {"box": (N,) i32 index + 1 into WAYMO_RAW_BOXES of the box a point was drawn in (0: ground),
    "static": (N,) bool, "pose": (4, 4)}]}."""
    import os
    import pickle

    import numpy as np
    names, out = [], {}
    n_box = len(WAYMO_RAW_BOXES)
    for s in range(n_sequences):
        seq = "segment-%04d_with_camera_labels" % s
        rs = np.random.RandomState(seed + s)
        d_data, d_flow = os.path.join(root, data_tag, seq), os.path.join(root, flow_tag, seq)
        os.makedirs(d_data, exist_ok=True)
        os.makedirs(d_flow, exist_ok=True)
        # world boxes, one per 7-m slot in front of the start: centre, (l, w, h), heading; the reference's extents are (l, h, w)
        slots = [(x, y) for x in (9.0, 16.0, 23.0) for y in (-7.0, 0.0, 7.0)]
        order = rs.permutation(len(slots))[:n_box]
        dims = np.stack([2.0 + 2.5 * rs.rand(n_box), 1.2 + 0.8 * rs.rand(n_box), 1.2 + 0.8 * rs.rand(n_box)], 1)
        centres = np.stack([np.array([slots[i][0] for i in order]) + rs.rand(n_box) - 0.5,
                            np.array([slots[i][1] for i in order]) + rs.rand(n_box) - 0.5, -1.8 + 0.2 + dims[:, 1] / 2 + 0.3 * rs.rand(n_box)], 1)
        headings = (rs.rand(n_box) - 0.5) * 2 * np.pi
        velocity = np.zeros((n_box, 3))
        velocity[4] = [3.0, 0.0, 0.0]                      # m/s in the world; a frame is 0.1 s
        tracks = ["%s_trk%02d" % (seq[:12], k) for k in range(n_box)]
        infos, frames, yaw, position = [], [], 0.0, np.zeros(3)
        for t in range(n_frames):
            pose = np.eye(4)
            pose[:3, :3], pose[:3, 3] = _rot_z_np(yaw), position
            n = n_points + int(rs.randint(-(n_points // 20), n_points // 20 + 1))
            n_obj = n // 3
            which = rs.randint(n_box, size=n_obj)
            now = centres + 0.1 * t * velocity
            half = dims[:, [0, 2, 1]] / 2 - RAW_MARGIN                  # x: l, y: h, z: w
            local = (rs.rand(n_obj, 3) - 0.5) * 2 * half[which]
            c, sn = np.cos(headings[which]), np.sin(headings[which])
            world = np.stack([c * local[:, 0] - sn * local[:, 1], sn * local[:, 0] + c * local[:, 1], local[:, 2]], 1) + now[which]
            ground = np.stack([position[0] - 20.0 + 95.0 * rs.rand(n - n_obj), position[1] + (rs.rand(n - n_obj) - 0.5) * 130.0,
                               -1.8 + (rs.rand(n - n_obj) - 0.5) * 0.06], 1)
            world = np.concatenate([world, ground])
            box = np.concatenate([which + 1, np.zeros(n - n_obj, dtype=np.int64)]).astype(np.int32)
            vel = np.concatenate([velocity[which], np.zeros((n - n_obj, 3))])
            perm = rs.permutation(n)
            world, box, vel = world[perm], box[perm], vel[perm]
            pc = (world - position) @ pose[:3, :3]                      # R^T (w - t), row-wise
            flag = np.where(rs.rand(n) < 0.1, rs.randint(0, 2, size=n), -1).astype(np.float64)
            np.save(os.path.join(d_data, "%04d.npy" % t), np.concatenate([pc, rs.rand(n, 2), flag[:, None]], 1).astype(np.float32))
            np.save(os.path.join(d_flow, "%04d.npy" % t), np.concatenate([vel @ pose[:3, :3], box[:, None] > 0], 1).astype(np.float32))
            listed = rs.permutation(n_box)
            gt = np.concatenate([(now - position) @ pose[:3, :3], dims, (headings - yaw)[:, None]], 1)[listed]
            infos.append({"point_cloud": {"lidar_sequence": seq, "sample_idx": t}, "pose": pose.copy(),
                          "annos": {"name": np.array([WAYMO_RAW_BOXES[k][0] for k in listed]),
                                    "gt_boxes_lidar": gt.astype(box_dtype),
                                    "obj_ids": np.array([tracks[k] for k in listed]),
                                    "num_points_in_gt": np.array([WAYMO_RAW_BOXES[k][1] * int((box == k + 1).sum()) for k in listed])}})
            frames.append({"box": box, "static": box != 5, "pose": pose.copy()})
            yaw += (rs.rand() - 0.5) * 0.04
            position = position + np.array([0.6 + 0.4 * rs.rand(), (rs.rand() - 0.5) * 0.2, 0.0])
        with open(os.path.join(d_data, seq + ".pkl"), "wb") as f:
            pickle.dump(infos, f)
        names.append(seq)
        out[seq] = frames
    with open(os.path.join(root, split + ".txt"), "w") as f:
        f.write("\n".join(["%s.tfrecord" % n for n in names] + ["segment-absent_with_camera_labels.tfrecord"]) + "\n")
    return out


# P_rect_02 of a KITTI Scene Flow calib_cam_to_cam file, as the numbers the file holds
KITTISF_P_RECT = ((721.5377, 0.0, 609.5593, 44.85728), (0.0, 721.5377, 172.854, 0.2163791), (0.0, 0.0, 1.0, 0.002745884))
# raw instance ids (semantic * 256 + instance) of the synthetic instance maps: background, two cars (26), a truck (28) — the
# semantics process_kittisf keeps — and a person (24), a bus (27) and a bicycle (33), which it does not
KITTISF_INSTANCE_IDS = (0, 26 * 256 + 1, 26 * 256 + 2, 28 * 256 + 1, 24 * 256 + 1, 27 * 256 + 3, 33 * 256)


def make_kittisf_maps(height, width, rs):
    """The four 16-bit maps of one KITTI Scene Flow frame, drawn from the RandomState `rs`: disp1, disp2, inst (H, W) and flow
    (H, W, 3) uint16.  Disparities between 1500 and 12000 raw (5.9 .. 46.9 px: depths of 66 .. 8.3 m, on both sides of the 35-m
    threshold) with about 20 % zeros (no ground truth) in each map; flows of up to +-20 px with about 80 % of the validity flags
    1; the instance map constant on blocks of 8 x 16 pixels with ids of KITTISF_INSTANCE_IDS, half of the blocks background."""
    import numpy as np
    disp1 = rs.randint(1500, 12001, size=(height, width))
    disp2 = np.clip(disp1 + rs.randint(-400, 401, size=(height, width)), 1500, 12000)
    disp1[rs.rand(height, width) < 0.2] = 0
    disp2[rs.rand(height, width) < 0.2] = 0
    flow = np.stack([32768 + rs.randint(-1280, 1281, size=(height, width)), 32768 + rs.randint(-1280, 1281, size=(height, width)),
                     (rs.rand(height, width) < 0.8).astype(np.int64)], 2)
    blocks = rs.randint(1, len(KITTISF_INSTANCE_IDS), size=((height + 7) // 8, (width + 15) // 16))
    blocks[rs.rand(*blocks.shape) < 0.5] = 0
    inst = np.asarray(KITTISF_INSTANCE_IDS)[np.repeat(np.repeat(blocks, 8, 0), 16, 1)[:height, :width]]
    return disp1.astype(np.uint16), disp2.astype(np.uint16), flow.astype(np.uint16), inst.astype(np.uint16)


def write_kittisf_raw_root(root, n_frames, height=48, width=160, seed=9300):
    """`n_frames` raw KITTI Scene Flow frames under <root>/training, in the layout of the download: disp_occ_0/%06d_10.png,
    disp_occ_1/%06d_10.png, instance/%06d_10.png (16-bit grey), flow_occ/%06d_10.png (16-bit RGB) — the maps of
    make_kittisf_maps, written by data_prepare/png16.py with mixed row filters — and calib_cam_to_cam/%06d.txt — what
    process_kittisf reads.  Returns a list of frames {"disp1", "disp2", "flow", "inst": the arrays, "P_rect": (3, 4) float32}."""
    import os

    import numpy as np

    from ..data_prepare.png16 import write_png
    base = os.path.join(root, "training")
    for sub in ("disp_occ_0", "disp_occ_1", "flow_occ", "instance", "calib_cam_to_cam"):
        os.makedirs(os.path.join(base, sub), exist_ok=True)
    frames = []
    for i in range(n_frames):
        rs = np.random.RandomState(seed + i)
        disp1, disp2, flow, inst = make_kittisf_maps(height, width, rs)
        for sub, array in (("disp_occ_0", disp1), ("disp_occ_1", disp2), ("flow_occ", flow), ("instance", inst)):
            write_png(os.path.join(base, sub, "%06d_10.png" % i), array, filters=rs.randint(0, 5, size=height))
        P = np.asarray(KITTISF_P_RECT, dtype=np.float64)
        with open(os.path.join(base, "calib_cam_to_cam", "%06d.txt" % i), "w") as f:
            f.write("calib_time: 09-Jan-2012 13:57:47\ncorner_dist: 9.950000e-02\n")
            f.write("".join("%s: %s\n" % (key, " ".join("%.6e" % v for v in value.reshape(-1)))
                            for key, value in (("S_rect_02", np.array([float(width), float(height)])), ("R_rect_02", np.eye(3)),
                                               ("P_rect_02", P), ("P_rect_03", P))))
        frames.append({"disp1": disp1, "disp2": disp2, "flow": flow, "inst": inst,
                       "P_rect": np.array([float("%.6e" % v) for v in P.reshape(-1)], dtype=np.float32).reshape(3, 4)})
    return frames


OGCDR_GROUND_THICKNESS, OGCDR_GROUND_HEIGHT, OGCDR_WALL_THICKNESS = 0.01, -0.5, 0.01      # build_ogcdr.py:55-58
OGCDR_GROUND_LEVEL = OGCDR_GROUND_HEIGHT + OGCDR_GROUND_THICKNESS


def _grid_box(size, k):
    """A closed box of 12 k^2 triangles around the origin, every side a k x k grid of its own vertices."""
    import numpy as np
    size = np.asarray(size, dtype=np.float64)
    vertices, faces = [], []
    t = np.linspace(-0.5, 0.5, k + 1)
    for axis in range(3):
        for sign in (-0.5, 0.5):
            a, b = (axis + 1) % 3, (axis + 2) % 3
            base = len(vertices)
            for i in range(k + 1):
                for j in range(k + 1):
                    p = np.zeros(3)
                    p[axis], p[a], p[b] = sign, t[i], t[j]
                    vertices.append(p * size)
            for i in range(k):
                for j in range(k):
                    q = [base + i * (k + 1) + j, base + (i + 1) * (k + 1) + j, base + (i + 1) * (k + 1) + j + 1, base + i * (k + 1) + j + 1]
                    if sign < 0:
                        q = q[::-1]
                    faces += [[q[0], q[1], q[2]], [q[0], q[2], q[3]]]
    return np.asarray(vertices), faces


def _ellipsoid(size, n_around=8, n_rings=6):
    """A closed ellipsoid of 2 n_around (n_rings - 1) triangles around the origin."""
    import numpy as np
    size = np.asarray(size, dtype=np.float64)
    vertices = [[0.0, 0.5, 0.0]]
    for r in range(1, n_rings):
        polar = math.pi * r / n_rings
        vertices += [[0.5 * math.sin(polar) * math.cos(2 * math.pi * s / n_around), 0.5 * math.cos(polar),
                      0.5 * math.sin(polar) * math.sin(2 * math.pi * s / n_around)] for s in range(n_around)]
    vertices.append([0.0, -0.5, 0.0])
    last = len(vertices) - 1
    faces = []
    for s in range(n_around):
        t = (s + 1) % n_around
        faces.append([0, 1 + t, 1 + s])
        for r in range(n_rings - 2):
            u, v = 1 + r * n_around, 1 + (r + 1) * n_around
            faces += [[u + s, u + t, v + t], [u + s, v + t, v + s]]
        faces.append([last, last - n_around + s, last - n_around + t])
    return np.asarray(vertices) * size, faces


def ogcdr_object_mesh(kind, rs):
    """The canonical mesh of a synthetic OGC-DR object -> (vertices (V, 3) float64, faces: a list of index lists).  kind % 3 == 0: a
    grid box of 48 triangles with zero-area faces in front, inside and at the end of the list; 1: an ellipsoid of 80 triangles;
    2: a grid box of 108 triangles, two of them written as one quad."""
    size = 0.05 + 0.03 * rs.rand(3)
    if kind % 3 == 0:
        vertices, faces = _grid_box(size, 2)
        faces = [[0, 0, 1], [2, 2, 2]] + faces[:20] + [[5, 7, 5]] + faces[20:] + [[3, 4, 4]]
    elif kind % 3 == 1:
        vertices, faces = _ellipsoid(size)
    else:
        vertices, faces = _grid_box(size, 3)
        faces = [[faces[0][0], faces[0][1], faces[0][2], faces[1][2]]] + faces[2:]
    return vertices, faces


def box_mesh_between(lo, hi):
    """The axis-aligned box between two corners as 12 triangles: (vertices (24, 3) float64, faces)."""
    import numpy as np
    lo, hi = np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64)
    vertices, faces = _grid_box(hi - lo, 1)
    return vertices + (lo + hi) / 2, faces


def ogcdr_background_meshes(xz_range, wall_height):
    """Ground and the four walls of a room as get_ground / get_walls lay them out around `xz_range` (build_ogcdr.py:370-405)
    -> ((vertices, faces) of the ground, [(vertices, faces)] of wall 0 .. 3)."""
    xr = xz_range
    gl, wt = OGCDR_GROUND_LEVEL, OGCDR_WALL_THICKNESS
    ground = box_mesh_between([-xr[0] / 2, OGCDR_GROUND_HEIGHT, -xr[1] / 2], [xr[0] / 2, gl, xr[1] / 2])
    walls = (([-xr[0] / 2, gl, -xr[1] / 2], [xr[0] / 2, gl + wall_height, -xr[1] / 2 + wt]),
             ([-xr[0] / 2, gl, -xr[1] / 2], [-xr[0] / 2 + wt, gl + wall_height, xr[1] / 2]),
             ([-xr[0] / 2, gl, xr[1] / 2 - wt], [xr[0] / 2, gl + wall_height, xr[1] / 2]),
             ([xr[0] / 2 - wt, gl, -xr[1] / 2], [xr[0] / 2, gl + wall_height, xr[1] / 2]))
    return ground, [box_mesh_between(lo, hi) for lo, hi in walls]


def write_shapenet_root(data_root, split_root, n_models, classes=("02828884", "03001627", "04379243"), seed=9700):
    """A small root in the layout build_ogcdr reads: <data_root>/ShapeNet_mesh/<class>/<model>/model.obj, `n_models` models of
    ogcdr_object_mesh per class and split, away from the origin and of differing sizes so that scaling and centring have work to
    do, and <split_root>/<class>/{train,val,test}.lst naming them.  Returns {class: {split: [model]}}."""
    import os

    import numpy as np

    from ..data_prepare.mesh_io import write_obj
    rs = np.random.RandomState(seed)
    out = {}
    for c, cl in enumerate(classes):
        os.makedirs(os.path.join(split_root, cl), exist_ok=True)
        out[cl] = {}
        for s, split in enumerate(("train", "val", "test")):
            models = ["%s%04d" % (split, m) for m in range(n_models)]
            for m, model in enumerate(models):
                vertices, faces = ogcdr_object_mesh(c + s + m, rs)
                os.makedirs(os.path.join(data_root, "ShapeNet_mesh", cl, model), exist_ok=True)
                write_obj(os.path.join(data_root, "ShapeNet_mesh", cl, model, "model.obj"),
                          vertices * (1.0 + 9.0 * rs.rand()) + (rs.rand(3) - 0.5), faces)
            with open(os.path.join(split_root, cl, split + ".lst"), "w") as f:
                f.write("\n".join(models) + "\n")
            out[cl][split] = models
    return out


def write_ogcdr_mesh_root(root, n_scenes, n_objects=3, n_frames=4, seed=9500, split="val", xz_range=(0.4, 0.3), wall_height=0.08,
                          meta_key="xz_ground_range"):
    """`n_scenes` scenes in the layout build_ogcdr.py leaves and sample_pointcloud reads: <root>/mesh/<NN_id>/object_FF_OO.obj — the
    meshes of ogcdr_object_mesh under a rigid object-to-world pose per frame (a turn about y and a shift of a few millimetres from
    frame to frame) —, ground.obj and wall_00..03.obj as get_ground / get_walls lay them out around `xz_range` (build_ogcdr.py:370-405)
    and meta.pkl with the range under `meta_key`; <root>/data/<NN_id>/pose_FF.npy (n_objects, 4, 4) float64 and
    <root>/data/{train,val,test}.lst, the scenes listed in `split`.  NN is the number of objects.  The room is small, so that at a few
    thousand sampled points the thinning radius stays below the thickness of ground and walls.  Returns the scene ids."""
    import os
    import pickle

    import numpy as np

    from ..data_prepare.mesh_io import write_obj
    xr = np.asarray(xz_range, dtype=np.float64)
    ids = []
    for i in range(n_scenes):
        rs = np.random.RandomState(seed + i)
        name = "%02d_%06d" % (n_objects, i)
        mesh_dir, data_dir = os.path.join(root, "mesh", name), os.path.join(root, "data", name)
        os.makedirs(mesh_dir, exist_ok=True)
        os.makedirs(data_dir, exist_ok=True)
        with open(os.path.join(mesh_dir, "meta.pkl"), "wb") as f:
            pickle.dump({"room_id": i, "split": split, "n_object": n_objects, meta_key: xr.copy(), "wall_height": float(wall_height)}, f,
                        protocol=pickle.HIGHEST_PROTOCOL)
        gl = OGCDR_GROUND_LEVEL
        ground, walls = ogcdr_background_meshes(xr, wall_height)
        write_obj(os.path.join(mesh_dir, "ground.obj"), *ground)
        for w, wall in enumerate(walls):
            write_obj(os.path.join(mesh_dir, "wall_%02d.obj" % w), *wall)
        objects = [ogcdr_object_mesh(k, rs) for k in range(n_objects)]
        yaw = rs.rand(n_objects) * 2 * math.pi
        shift = (rs.rand(n_objects, 3) - 0.5) * np.array([xr[0] * 0.4, 0.1, xr[1] * 0.4]) + np.array([0.0, gl + 0.12, 0.0])
        for t in range(n_frames):
            poses = np.zeros((n_objects, 4, 4))
            for k, (vertices, faces) in enumerate(objects):
                poses[k] = np.eye(4)
                poses[k, :3, :3], poses[k, :3, 3] = _rot_y_np(yaw[k]), shift[k]
                write_obj(os.path.join(mesh_dir, "object_%02d_%02d.obj" % (t, k)), _apply_4x4(poses[k], vertices), faces)
            np.save(os.path.join(data_dir, "pose_%02d.npy" % t), poses)
            yaw = yaw + (rs.rand(n_objects) - 0.5) * 2 * math.radians(8.0)
            shift = shift + (rs.rand(n_objects, 3) - 0.5) * np.array([0.016, 0.01, 0.016])
        ids.append(name)
    for which in ("train", "val", "test"):
        with open(os.path.join(root, "data", which + ".lst"), "w") as f:
            f.write("\n".join(ids) + "\n" if which == split else "")
    return ids


def write_ogcdr_singleview_root(sv_root, complete_root, n_frames=4, seed=9600, jitter=5e-4):
    """A single-view root for collect_segm from complete clouds: for every scene under <complete_root>/data the file
    <sv_root>/pcd/<id>/pc_FF.pcd with those points of pc_FF.npy that face +z — at or above the cloud's median z —, each moved by a
    jitter of `jitter` per coordinate and shuffled, as binary PCD.  Returns {id: [points per frame]}."""
    import os

    import numpy as np

    from ..data_prepare.mesh_io import write_pcd
    rs = np.random.RandomState(seed)
    counts = {}
    for name in sorted(os.listdir(os.path.join(complete_root, "data"))):
        src = os.path.join(complete_root, "data", name)
        if not os.path.isdir(src):
            continue
        os.makedirs(os.path.join(sv_root, "pcd", name), exist_ok=True)
        counts[name] = []
        for t in range(n_frames):
            pc = np.load(os.path.join(src, "pc_%02d.npy" % t)).astype(np.float32)
            view = pc[pc[:, 2] >= np.median(pc[:, 2])]
            view = (view + (rs.rand(*view.shape).astype(np.float32) - np.float32(0.5)) * np.float32(2 * jitter))[rs.permutation(len(view))]
            write_pcd(os.path.join(sv_root, "pcd", name, "pc_%02d.pcd" % t), view)
            counts[name].append(len(view))
    return counts
