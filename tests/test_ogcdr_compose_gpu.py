"""ogc_room_compose and ogc_mesh_apply_poses (csrc/room_compose.hip) against the float64 mirror of
tests/ogcdr_compose_cases.py, bit for bit: poses, attempt, fails and status of the composition, and the moved vertices.  The two
large batches are checked to contain every path of the rule — the three codes, a frame accepted after a failed try, accepted attempts
in the first, the second and a later group of 64 — on the MIRROR's result, so that no path is silently missed."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ogcdr_compose_cases as cc  # noqa: E402

from ogc_amd import _lib  # noqa: E402
from ogc_amd import pointnet2_cuda as native  # noqa: E402
from ogc_amd.data_prepare import mesh_ops  # noqa: E402

KEYS = ("vertices", "vert_offsets", "obj_offsets", "room", "seeds")
BIG = {"three": (dict(n_trial=300, n_object=3, scale_lo=0.25, scale_hi=0.45, seed=11), dict(max_iter=1000, max_retry=20)),
       "two": (dict(n_trial=300, n_object=2, scale_lo=0.2, scale_hi=0.3, seed=12), dict(max_iter=2, max_retry=1))}


def upload(batch):
    return [torch.from_numpy(np.ascontiguousarray(batch[k])).cuda() for k in KEYS]


def launch(batch, **constants):
    """The library called directly -> its four outputs as numpy, whatever the codes."""
    c = dict(cc.DEFAULTS, **constants)
    dev = upload(batch)
    n_object, n_trial, n_frame = len(batch["vert_offsets"]) - 1, len(batch["obj_offsets"]) - 1, c["n_frame"]
    poses = torch.zeros(n_object, n_frame, 4, 4, dtype=torch.float64, device="cuda")
    attempt = torch.zeros(n_object, n_frame, dtype=torch.int32, device="cuda")
    fails = torch.zeros(n_trial, n_frame, dtype=torch.int32, device="cuda")
    status = torch.full((n_trial, 2), -1, dtype=torch.int32, device="cuda")
    native.room_compose_wrapper(n_trial, n_object, len(batch["vertices"]), *dev, [c[k] for k in mesh_ops.COMPOSE_DOUBLES],
                                [c[k] for k in mesh_ops.COMPOSE_INTS], poses, attempt, fails, status)
    return dict(poses=poses.cpu().numpy(), attempt=attempt.cpu().numpy(), fails=fails.cpu().numpy(), status=status.cpu().numpy())


def mirror(batch, **constants):
    want = cc.compose_mirror(*[batch[k] for k in KEYS], **constants)
    want["obj_offsets"] = batch["obj_offsets"]
    return want


def check(batch, **constants):
    """compose_rooms and apply_poses on a batch against the mirror -> the mirror's result."""
    want = mirror(batch, **constants)
    dev = upload(batch)
    out = mesh_ops.compose_rooms(*dev, **constants)
    got = {k: getattr(out, k).cpu().numpy() for k in out._fields}
    assert got["poses"].dtype == np.float64 and got["attempt"].dtype == np.int32 and got["status"].shape == (len(batch["room"]), 2)
    cc.compare_composed(got, want)
    moved = mesh_ops.apply_poses(dev[0], dev[1], out.poses).cpu().numpy()
    want_moved = cc.apply_poses_mirror(batch["vertices"], batch["vert_offsets"], want["poses"])
    assert moved.shape == want_moved.shape == (want["poses"].shape[1], len(batch["vertices"]), 3)
    for t in np.nonzero(want["status"][:, 0] == 0)[0]:
        v0, v1 = (int(batch["vert_offsets"][batch["obj_offsets"][e]]) for e in (t, t + 1))
        assert np.array_equal(moved[:, v0:v1].view(np.uint64), want_moved[:, v0:v1].view(np.uint64)), t
    return want


@pytest.fixture(scope="module")
def big():
    """The two large batches and the mirror's result for each, computed once."""
    out = {}
    for name, (shape, constants) in BIG.items():
        batch = cc.box_batch(shape["n_trial"], shape["n_object"], shape["scale_lo"], shape["scale_hi"], shape["seed"])
        out[name] = (batch, constants, mirror(batch, **constants))
    return out


def test_the_large_batches_reach_every_path(big):
    codes, after_failure, attempts = set(), 0, []
    for batch, _, want in big.values():
        codes |= set(want["status"][:, 0].tolist())
        good = np.nonzero(want["status"][:, 0] == 0)[0]
        after_failure += int((want["fails"][good].max(1) >= 1).sum())
        attempts += [want["attempt"][batch["obj_offsets"][t]:batch["obj_offsets"][t + 1]].ravel() for t in good]
        assert (want["status"][want["status"][:, 0] == 2, 1] >= 1).all() and (want["status"][want["status"][:, 0] != 2, 1] == 0).all()
    attempts = np.concatenate(attempts)
    print("codes %s, composed after a failed try: %d, accepted attempts: %d at 0, %d in [64, 128), %d from 128, largest %d"
          % (sorted(codes), after_failure, (attempts == 0).sum(), ((attempts >= 64) & (attempts < 128)).sum(), (attempts >= 128).sum(),
             attempts.max()))
    assert codes == {0, 1, 2} and after_failure >= 1
    assert (attempts == 0).any() and ((attempts >= 64) & (attempts < 128)).any() and (attempts >= 128).any()


@pytest.mark.parametrize("name", sorted(BIG))
def test_large_batch_equals_the_mirror(big, name):
    batch, constants, want = big[name]
    dev = upload(batch)
    out = mesh_ops.compose_rooms(*dev, **constants)
    cc.compare_composed({k: getattr(out, k).cpu().numpy() for k in out._fields}, want)
    moved = mesh_ops.apply_poses(dev[0], dev[1], out.poses).cpu().numpy()
    want_moved = cc.apply_poses_mirror(batch["vertices"], batch["vert_offsets"], want["poses"])
    n = batch["obj_offsets"][1] * 8                                           # every trial: the same number of boxes of 8 vertices
    for t in np.nonzero(want["status"][:, 0] == 0)[0]:
        assert np.array_equal(moved[:, n * t:n * (t + 1)].view(np.uint64), want_moved[:, n * t:n * (t + 1)].view(np.uint64)), t


def test_one_trial_and_one_object():
    rs = np.random.RandomState(31)
    want = check(cc.pack([([cc.box_object(rs, 0.25, 0.45) for _ in range(3)], [1.0, 0.9])], 3100))
    assert want["status"].tolist() == [[0, 0]]
    # one object: no overlap test, every frame-0 attempt is accepted at once
    want = check(cc.pack([([cc.box_object(rs, 0.2, 0.3)], cc.draw_room(rs)) for _ in range(5)], 3200))
    assert (want["status"][:, 0] == 0).all() and (want["attempt"][:, 0] == 0).all()


def test_thirty_two_objects_in_a_large_room():
    rs = np.random.RandomState(32)
    want = check(cc.pack([([cc.box_object(rs, 0.2, 0.3) for _ in range(32)], [3.0, 3.0]) for _ in range(2)], 3300))
    assert (want["status"][:, 0] == 0).any() and want["attempt"].max() >= 1


def test_trials_of_differing_object_counts_and_reduction_edges():
    rs = np.random.RandomState(33)
    trials = [([cc.box_object(rs, 0.2, 0.3) for _ in range(n)], cc.draw_room(rs)) for n in (4, 0, 1, 7, 2, 0, 5)]
    # meshes of 1, 257 and 1000 vertices: one lane, one vertex past a full round of the workgroup, several rounds with a ragged end
    trials += [([cc.cloud_object(rs, n, 0.3) for n in (1, 257, 1000)], [1.0, 0.8]), ([cc.cloud_object(rs, n, 0.25) for n in (1000, 1, 257, 8)], [0.9, 1.0])]
    want = check(cc.pack(trials, 3400))
    assert (want["status"][[1, 5]] == 0).all() and (want["status"][-2:, 0] == 0).all()
    # other constants than the reference's: more frames, every range moved
    want = check(cc.pack(trials, 3500), n_frame=8, y_angle_lo=-30.0, y_angle_hi=400.0, mot_y_angle_lo=-3.0, mot_y_angle_hi=7.0, mot_xz_angle_lo=-5.0,
                 mot_xz_angle_hi=2.0, prob_rotation_y=0.3, mot_transl_lo=0.01, mot_transl_hi=0.03, ground_level=0.125, wall_thickness=0.02)
    assert (want["status"][:, 0] == 0).sum() >= 4
    want = check(cc.pack(trials[:1], 3600), n_frame=1)
    assert want["poses"].shape[1] == 1


def test_a_value_that_is_not_finite_is_code_3_in_its_trial_alone():
    batch = cc.box_batch(4, 2, 0.2, 0.3, 34)
    clean = mirror(batch)
    for key, index, trial in (("vertices", (17, 2), 1), ("vertices", (63, 0), 3), ("room", (2, 1), 2)):
        bad = dict(batch, **{key: batch[key].copy()})
        bad[key][index] = (np.nan, np.inf, -np.inf)[trial - 1]
        got, want = launch(bad), mirror(bad)
        assert want["status"][trial].tolist() == [3, 0] and np.array_equal(np.delete(want["status"], trial, 0), np.delete(clean["status"], trial, 0))
        cc.compare_composed(got, want)
        with pytest.raises(ValueError, match="not finite"):
            mesh_ops.compose_rooms(*upload(bad))


def test_offsets_that_are_refused_are_code_4_in_every_trial():
    batch = cc.box_batch(3, 2, 0.2, 0.3, 35)       # vert_offsets 0, 8, .. 48; obj_offsets 0, 2, 4, 6
    cases = [("vert_offsets", [1, 8, 16, 24, 32, 40, 48]), ("vert_offsets", [0, 8, 16, 24, 32, 40, 47]), ("vert_offsets", [0, 8, 8, 24, 32, 40, 48]),
             ("vert_offsets", [0, 8, 24, 16, 32, 40, 48]), ("obj_offsets", [1, 2, 4, 6]), ("obj_offsets", [0, 2, 4, 5]), ("obj_offsets", [0, 4, 2, 6])]
    for key, value in cases:
        bad = dict(batch, **{key: np.array(value, dtype=np.int32)})
        got = launch(bad)
        assert got["status"].tolist() == [[4, 0]] * 3 == mirror(bad)["status"].tolist(), (key, value)
        with pytest.raises(ValueError, match="offsets"):
            mesh_ops.compose_rooms(*upload(bad))
    # the limit on a trial's objects is found on the device, where the offsets are: 32 pass, 33 are code 4
    rs = np.random.RandomState(36)
    for n, code in ((32, None), (33, 4)):
        many = cc.pack([([cc.box_object(rs, 0.05, 0.06) for _ in range(n)], [2.0, 2.0]), ([cc.box_object(rs, 0.2, 0.3)], [1.0, 1.0])], 3700)
        got = launch(many, max_iter=64)
        assert got["status"][:, 0].tolist() == mirror(many, max_iter=64)["status"][:, 0].tolist()
        assert (got["status"][:, 0] == 4).all() if code else (got["status"][:, 0] != 4).all()


def test_argument_errors_launch_nothing_and_no_trials_is_no_work():
    batch = cc.box_batch(2, 2, 0.2, 0.3, 37)
    for constants in (dict(n_frame=9), dict(n_frame=0), dict(max_iter=65537), dict(max_iter=0), dict(max_retry=256), dict(max_retry=-1),
                      dict(ground_level=float("nan")), dict(mot_transl_hi=float("inf"))):
        with pytest.raises(_lib.OgcOpsError, match="status -1"):
            mesh_ops.compose_rooms(*upload(batch), **constants)
    assert (launch(batch, n_frame=8, max_iter=65536, max_retry=255)["status"][:, 0] >= 0).all()      # the limits themselves are taken
    with pytest.raises(TypeError, match="unknown constants"):
        mesh_ops.compose_rooms(*upload(batch), max_tries=3)
    dev = upload(batch)
    with pytest.raises(TypeError):
        mesh_ops.compose_rooms(dev[0].float(), *dev[1:])
    with pytest.raises(RuntimeError, match="CUDA tensor"):
        mesh_ops.compose_rooms(dev[0].cpu(), *dev[1:])
    with pytest.raises(ValueError, match="room must be"):
        mesh_ops.compose_rooms(dev[0], dev[1], dev[2], dev[3][:1], dev[4])
    with pytest.raises(RuntimeError, match="contiguous"):
        mesh_ops.compose_rooms(dev[0], dev[1], dev[2], dev[3].t().contiguous().t(), dev[4])
    with pytest.raises(ValueError, match="poses must be"):
        mesh_ops.apply_poses(dev[0], dev[1], torch.zeros(3, 4, 4, 4, dtype=torch.float64, device="cuda"))
    # T == 0, with and without objects lying about
    empty = dict(vertices=np.zeros((0, 3)), vert_offsets=np.zeros(1, dtype=np.int32), obj_offsets=np.zeros(1, dtype=np.int32),
                 room=np.zeros((0, 2)), seeds=np.zeros(0, dtype=np.int64))
    out = mesh_ops.compose_rooms(*upload(empty))
    assert out.poses.shape == (0, 4, 4, 4) and out.status.shape == (0, 2) and out.fails.shape == (0, 4)
    assert mesh_ops.apply_poses(*upload(empty)[:2], out.poses).shape == (4, 0, 3)
    got = launch(dict(batch, obj_offsets=np.zeros(1, dtype=np.int32), room=np.zeros((0, 2)), seeds=np.zeros(0, dtype=np.int64)))
    assert got["status"].shape == (0, 2) and not got["poses"].any()
