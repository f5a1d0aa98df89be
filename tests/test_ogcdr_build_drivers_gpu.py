"""The scene-composition driver (ogc_amd/data_prepare/build_ogcdr.py) on a synthetic ShapeNet-like root
(ogc_amd/utils/synthetic.py::write_shapenet_root): two types of 2 and 3 objects, 4 rooms each asked for, 4000 surface points sampled
to 256.  The written tree, meshes against poses bit for bit, independence of --batch, the seed, and the rest of the OGC-DR chain on
the result: sample_pointcloud reproduces the clouds, the reader loads a sample, build_ogcdrsv and collect_segm run."""
import os
import pickle
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ogcdr_compose_cases as cc  # noqa: E402

from ogc_amd.data_prepare import build_ogcdr, build_ogcdrsv, collect_segm, mesh_io, sample_pointcloud  # noqa: E402
from ogc_amd.datasets import OGCDynamicRoomDataset  # noqa: E402

N_FPS, DATASET_SIZE, TYPES = 256, 4, (2, 3)
SIZES = ["--n_sample_point", "4000", "--n_sample_point_fps", str(N_FPS)]
COMMON = ["--types", ",".join(str(n) for n in TYPES), "--dataset_size", str(DATASET_SIZE)] + SIZES


@pytest.fixture(scope="module")
def roots(tmp_path_factory):
    base = tmp_path_factory.mktemp("ogcdr_build")
    out = {k: str(base / k) for k in ("batch4", "batch1", "seed1", "splits", "resampled", "single")}
    out["result"] = build_ogcdr.main([out["batch4"], "--split_root", out["splits"], "--synthetic", "2", "--batch", "4"] + COMMON)
    for name, extra in (("batch1", ["--batch", "1"]), ("seed1", ["--batch", "4", "--seed", "1"])):
        os.makedirs(out[name])
        os.symlink(os.path.join(out["batch4"], "ShapeNet_mesh"), os.path.join(out[name], "ShapeNet_mesh"))
        build_ogcdr.main([out[name], "--split_root", out["splits"]] + extra + COMMON)
    return out


def tree(root):
    """{relative path: bytes} of mesh/ and data/ below root."""
    out = {}
    for top in ("mesh", "data"):
        for d, _, files in os.walk(os.path.join(root, top)):
            for name in files:
                path = os.path.join(d, name)
                out[os.path.relpath(path, root)] = open(path, "rb").read()
    return out


def test_file_tree_meta_and_lists(roots):
    n_rooms = [int(p * DATASET_SIZE) for p in (.75, .05, .2)]
    assert n_rooms == build_ogcdr.split_sizes(DATASET_SIZE) == [3, 0, 0]
    names = ["%02d_%06d" % (n, r) for n in sorted(TYPES) for r in range(sum(n_rooms))]
    root = roots["batch4"]
    assert sorted(os.listdir(os.path.join(root, "mesh"))) == names == sorted(roots["result"]["scenes"])
    assert sorted(os.listdir(os.path.join(root, "data"))) == names + ["test.lst", "train.lst", "val.lst"]
    for split, size in zip(("train", "val", "test"), n_rooms):
        listed = open(os.path.join(root, "data", split + ".lst")).read().split()
        assert len(listed) == size * len(TYPES) and listed == roots["result"]["lists"][split]
    assert open(os.path.join(root, "data", "train.lst")).read().split() == ["%02d_%06d" % (n, r) for n in TYPES for r in range(3)]
    models = {cl: open(os.path.join(roots["splits"], cl, "train.lst")).read().split() for cl in os.listdir(roots["splits"])}
    for name in names:
        n = int(name[:2])
        files = sorted(os.listdir(os.path.join(root, "mesh", name)))
        assert files == sorted(["ground.obj", "meta.pkl"] + ["wall_%02d.obj" % w for w in range(4)]
                               + ["object_%02d_%02d.obj" % (f, k) for f in range(4) for k in range(n)])
        assert sorted(os.listdir(os.path.join(root, "data", name))) == sorted("%s_%02d.npy" % (w, f) for w in ("pc", "segm", "pose") for f in range(4))
        with open(os.path.join(root, "mesh", name, "meta.pkl"), "rb") as f:
            meta = pickle.load(f)
        assert list(meta) == ["room_id", "split", "n_object", "objects", "classes", "scales", "xz_ground_range", "wall_height"]
        assert meta["room_id"] == int(name[3:]) and meta["split"] == "train" and meta["n_object"] == n == len(meta["objects"]) == len(meta["scales"])
        lo, hi = build_ogcdr.SCALE_INTERVALS[TYPES.index(n)]
        assert all(lo <= s <= hi for s in meta["scales"]) and 0.2 <= meta["wall_height"] <= 0.4
        assert all(o.split("/")[1] in models[o.split("/")[0]] and o.split("/")[0] == c for o, c in zip(meta["objects"], meta["classes"]))
        xr = meta["xz_ground_range"]
        assert xr.dtype == np.float64 and xr.max() == 1.0 and 0.6 <= xr.min() <= 1.0
        ground = mesh_io.read_obj(os.path.join(root, "mesh", name, "ground.obj"))[0]
        assert np.allclose(ground.min(0), [-xr[0] / 2, -0.5, -xr[1] / 2]) and np.allclose(ground.max(0), [xr[0] / 2, -0.49, xr[1] / 2])


def test_written_meshes_are_the_posed_canonical_meshes_in_every_bit(roots):
    root = roots["batch4"]
    for name in roots["result"]["scenes"]:
        with open(os.path.join(root, "mesh", name, "meta.pkl"), "rb") as f:
            meta = pickle.load(f)
        inner = meta["xz_ground_range"] / 2.0 - 0.01
        canonical = []
        for model, scale in zip(meta["objects"], meta["scales"]):
            vertices, faces = mesh_io.read_obj(os.path.join(root, "ShapeNet_mesh", model, "model.obj"))
            canonical.append((build_ogcdr.canonical_vertices(vertices, scale), faces))
            assert abs((canonical[-1][0].max(0) - canonical[-1][0].min(0)).max() - scale) < 1e-12
        offsets = np.cumsum([0] + [len(v) for v, _ in canonical])
        for f in range(4):
            poses = np.load(os.path.join(root, "data", name, "pose_%02d.npy" % f))
            assert poses.shape == (len(canonical), 4, 4) and poses.dtype == np.float64
            want = cc.apply_poses_mirror(np.concatenate([v for v, _ in canonical]), offsets, poses[:, None])[0]
            boxes = []
            for k, (_, faces) in enumerate(canonical):
                got_v, got_f = mesh_io.read_obj(os.path.join(root, "mesh", name, "object_%02d_%02d.obj" % (f, k)))
                assert np.array_equal(got_f, faces)
                assert np.array_equal(got_v.view(np.uint64), want[offsets[k]:offsets[k + 1]].view(np.uint64)), (name, f, k)
                assert abs(got_v[:, 1].min() + 0.49) <= 1e-12
                lo, hi = got_v[:, [0, 2]].min(0), got_v[:, [0, 2]].max(0)
                assert (lo >= -inner - 1e-12).all() and (hi <= inner + 1e-12).all()
                assert all(((lo >= b - 1e-12) | (a >= hi - 1e-12)).any() for a, b in boxes)
                boxes.append((lo, hi))


def test_batch_size_does_not_matter_and_the_seed_does(roots):
    a, b, c = tree(roots["batch4"]), tree(roots["batch1"]), tree(roots["seed1"])
    assert sorted(a) == sorted(b) == sorted(c) and len(a) > 100
    assert all(a[k] == b[k] for k in a)
    differ = [k for k in a if a[k] != c[k]]
    assert any("pose_00.npy" in k for k in differ) and any("object_00_00.obj" in k for k in differ) and any("pc_00.npy" in k for k in differ)


def test_sample_pointcloud_reproduces_the_clouds(roots):
    sample_pointcloud.main([roots["batch4"], "--save_root", roots["resampled"]] + SIZES)
    a, b = tree(roots["batch4"]), tree(roots["resampled"])
    for name in roots["result"]["scenes"]:
        for f in range(4):
            for what in ("pc", "segm", "pose"):
                key = os.path.join("data", name, "%s_%02d.npy" % (what, f))
                assert a[key] == b[key], key
    pc, segm = (np.load(os.path.join(roots["batch4"], "data", "03_000000", "%s_00.npy" % w)) for w in ("pc", "segm"))
    assert pc.shape == (N_FPS, 3) and pc.dtype == np.float32 and segm.dtype == np.int16 and set(np.unique(segm)) == {1, 2, 3}


def test_reader_loads_a_sample(roots):
    dataset = OGCDynamicRoomDataset(roots["batch4"], "train", view_sels=[[0, 1], [2, 3]])
    assert len(dataset) == 2 * 6
    pcs, segms, flows, valids = dataset[7]
    assert pcs.shape == (2, N_FPS, 3) and flows.shape == (2, N_FPS, 3) and segms.shape == (2, N_FPS) and valids.all()
    # every object moves 0.02 .. 0.04 per axis between frames, plus its turn
    assert 0.02 < np.abs(flows[0]).max() < 0.2


def test_single_view_chain_runs_on_the_tree(roots):
    out = build_ogcdrsv.main(["--src_root", roots["batch4"], "--dest_root", roots["single"], "--width", "320", "--height", "180"])
    assert out["scenes"] == sorted(roots["result"]["scenes"]) and out["points"] > 0
    collect_segm.main(["--src_root", roots["batch4"], "--dest_root", roots["single"], "--n_sample_point", "64"])
    for name in roots["result"]["scenes"]:
        segm = np.load(os.path.join(roots["single"], "data", name, "segm_03.npy"))
        assert segm.shape == (64,) and segm.min() >= 1 and segm.max() <= int(name[:2])
    assert open(os.path.join(roots["single"], "data", "train.lst")).read() == open(os.path.join(roots["batch4"], "data", "train.lst")).read()
