"""ogc_moving_stats (ogc_amd/csrc/moving_stats.hip) through ogc_amd/data_prepare/scan_ops.py::moving_stats / moving_counts and the raw
wrapper, against the numpy mirror of tests/golden/make_waymo_select_golden.py, which its generator pinned to the reference's own
functions.  The outputs are integers, so they must EQUAL the mirror's: no tolerance, no excluded point.  That is decidable because
the inputs are: a static point carries the fp32-rounded rigid flow (residual below 1e-4), a moving one 0.5 m or more on top — the
mirror asserts that no point lies within 1e-6 of the threshold — and the points placed ON the threshold have R = I, t = 0 and one
flow component, where every step of the fp64 sequence is exact."""
import json
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
SIZES = (0, 1, 63, 64, 65, 255, 256, 257, 1000)
FILTERS = (((), 0), ((2, 3), 50), ((2, 3), 0), ((), 50))


@pytest.fixture(scope="module")
def mirror():
    sys.path.insert(0, os.path.join(HERE, "golden"))
    import make_waymo_select_golden
    return make_waymo_select_golden


@pytest.fixture(scope="module")
def golden():
    data = np.load(os.path.join(HERE, "golden", "waymo_select.npz"))
    return data, json.loads(str(data["meta"]))


def cap():
    from ogc_amd import _lib
    from ogc_amd.data_prepare.scan_ops import MOVING_STATS_LABEL_CAP
    c = _lib.load().ogc_moving_stats_label_cap()
    assert c == MOVING_STATS_LABEL_CAP and c >= 4096
    return c


def upload(samples):
    """samples: (pc, flow, segm, semantic_segm, motion) per sample -> the six device tensors of a ragged batch."""
    offsets = np.cumsum([0] + [s[0].shape[0] for s in samples]).astype(np.int32)

    def cat(k, dtype, tail):
        return torch.from_numpy(np.ascontiguousarray(np.concatenate([np.asarray(s[k]).reshape((-1,) + tail) for s in samples], 0), dtype=dtype)).cuda()
    return (cat(0, np.float32, (3,)), cat(1, np.float32, (3,)), cat(2, np.int32, ()), cat(3, np.int32, ()),
            torch.from_numpy(offsets).cuda(), cat(4, np.float64, (12,)))


def run(samples, **kwargs):
    from ogc_amd.data_prepare.scan_ops import moving_stats
    stats = moving_stats(*upload(samples), **kwargs)
    assert stats.dtype == torch.int32 and stats.shape == (len(samples), 4) and stats.is_cuda
    return stats.cpu().numpy()


def expect(mirror, samples, ignore_class_ids=(), ignore_npoint_thresh=0, ground_y=0.3, moving_thresh=0.2):
    return np.array([mirror.moving_mirror(*s[:5], ignore_class_ids, ignore_npoint_thresh, ground_y, moving_thresh) + (0,) for s in samples],
                    dtype=np.int32).reshape(len(samples), 4)


def draw(mirror, n, seed, kind="moving"):
    s = mirror.draw_sample(n, np.random.RandomState(seed), kind)
    mirror.assert_decided(s[0], s[1], s[4], 0.2, margin=1e-6)
    return s


@pytest.mark.parametrize("ignore, thresh", FILTERS)
def test_sizes(mirror, ignore, thresh):
    """Every N around the wave and the workgroup, one sample per launch and all of them in one."""
    samples = [draw(mirror, n, 100 + n) for n in SIZES]
    want = expect(mirror, samples, ignore, thresh)
    assert want[0].tolist() == [0, 0, 0, 0] and want[:, 2].max() > 0 and len(set(want[:, 0].tolist())) >= 3 - (thresh > 0)
    for s, w in zip(samples, want):
        assert np.array_equal(run([s], ignore_class_ids=ignore, ignore_npoint_thresh=thresh), w[None])
    assert np.array_equal(run(samples, ignore_class_ids=ignore, ignore_npoint_thresh=thresh), want)


@pytest.mark.parametrize("batch", (1, 3, 70))
def test_batches(mirror, batch):
    """Ragged batches: an empty sample between two non-empty ones, sample bases at every residue mod 4 points."""
    sizes = {1: [257], 3: [65, 0, 131]}.get(batch) or [(5, 0, 66, 131, 257, 3, 64, 1000, 1, 255)[i % 10] for i in range(batch)]
    samples = [draw(mirror, n, 300 + 7 * i + batch, ("moving", "static", "moving", "background")[i % 4]) for i, n in enumerate(sizes)]
    offsets = np.cumsum([0] + sizes)
    if batch > 1:
        assert sizes[1] == 0 and sizes[0] > 0 and sizes[2] > 0
    if batch == 70:
        assert set((offsets[:-1] % 4).tolist()) == {0, 1, 2, 3} and set((offsets[:-1] * 3 % 4).tolist()) == {0, 1, 2, 3}
    for ignore, thresh in FILTERS[:2]:
        want = expect(mirror, samples, ignore, thresh)
        assert np.array_equal(run(samples, ignore_class_ids=ignore, ignore_npoint_thresh=thresh), want)
    assert want[:, 2].max() > 0 or batch == 1


def test_fixture_cases(mirror, golden):
    data, meta = golden
    names = list(meta["cases"])
    samples = [tuple(data["%s_%s" % (n, k)] for k in ("pc", "flow", "segm", "semantic_segm", "motion")) for n in names]
    for name, s in zip(names, samples):
        case = meta["cases"][name]
        got = run([s], ignore_class_ids=case["ignore_class_ids"], ignore_npoint_thresh=case["ignore_npoint_thresh"],
                  ground_y=meta["ground_y"], moving_thresh=case["moving_thresh"])
        assert got[0].tolist() == data[name + "_stats"].tolist() + [0], name
    # the cases that share their parameters as one batch
    same = [i for i, n in enumerate(names) if meta["cases"][n]["ignore_class_ids"] == [2, 3] and meta["cases"][n]["ignore_npoint_thresh"] == 50]
    assert len(same) >= 2
    got = run([samples[i] for i in same], ignore_class_ids=(2, 3), ignore_npoint_thresh=50)
    assert got[:, :3].tolist() == [data[names[i] + "_stats"].tolist() for i in same] and not got[:, 3].any()


def labelled(mirror, segm, semantic, seed=1):
    """A static sample with the given labels."""
    pc, flow, _, _, motion = mirror.draw_sample(len(segm), np.random.RandomState(seed), "static")
    return pc, flow, np.asarray(segm, dtype=np.int32), np.asarray(semantic, dtype=np.int32), motion


def test_labels(mirror):
    c = cap()
    thresh = 50
    one = labelled(mirror, [7] * 80, [1] * 80)
    class_only = labelled(mirror, [7] * 80, [1] * 79 + [3])                # the only second value, 0, comes from an ignored class
    sizes = labelled(mirror, [0] * 60 + [4] * (thresh - 1) + [9] * thresh, [0] * 60 + [1] * (2 * thresh - 1))
    top = labelled(mirror, [c - 1] * 70 + [0] * 70, [1] * 70 + [0] * 70)
    ignored_whole = labelled(mirror, [5] * 60 + [6] * 60, [2] * 60 + [1] * 60)    # object 5 is all of class 2: it leaves, 0 arrives
    samples = [one, class_only, sizes, top, ignored_whole]
    for ignore, t in FILTERS:
        want = expect(mirror, samples, ignore, t)
        assert np.array_equal(run(samples, ignore_class_ids=ignore, ignore_npoint_thresh=t), want), (ignore, t)
    assert expect(mirror, samples, (), 0)[:, 0].tolist() == [1, 1, 3, 2, 2]
    assert expect(mirror, samples, (2, 3), 0)[:, 0].tolist() == [1, 2, 3, 2, 2]
    assert expect(mirror, samples, (), thresh)[:, 0].tolist() == [1, 1, 2, 2, 2]
    assert expect(mirror, samples, (2, 3), thresh)[:, 0].tolist() == [1, 2, 2, 2, 2]


@pytest.mark.parametrize("bad_label", ("cap", "minus_one"))
def test_label_outside_the_table(mirror, bad_label):
    """status 1 for that sample only, its other fields 0; the neighbours' results intact; nothing behind stats written."""
    from ogc_amd import pointnet2_cuda as nat
    from ogc_amd.data_prepare.scan_ops import moving_counts
    c = cap()
    bad_segm = [0] * 100 + [3] * 99 + [c if bad_label == "cap" else -1]
    samples = [draw(mirror, 130, 41), labelled(mirror, bad_segm, [1] * 200), draw(mirror, 67, 42)]
    want = expect(mirror, [samples[0], samples[2]], (2, 3), 5)
    got = run(samples, ignore_class_ids=(2, 3), ignore_npoint_thresh=5)
    assert got[1].tolist() == [0, 0, 0, 1] and np.array_equal(got[[0, 2]], want)
    with pytest.raises(ValueError, match="sample 1 "):
        moving_counts(*upload(samples), ignore_class_ids=(2, 3), ignore_npoint_thresh=5)
    assert np.array_equal(moving_counts(*upload([samples[0], samples[2]]), ignore_class_ids=(2, 3), ignore_npoint_thresh=5), want[:, :3])
    pc, flow, segm, semantic, offsets, motion = upload(samples)
    stats = torch.full((4, 4), -77, dtype=torch.int32, device="cuda")
    ign = torch.tensor([2, 3, -77, -77], dtype=torch.int32, device="cuda")
    nat.moving_stats_wrapper(3, pc.shape[0], offsets, pc, flow, segm, semantic, motion, ign, 2, 5, 0.3, 0.2, stats)
    assert np.array_equal(stats.cpu().numpy()[:3], got) and stats.cpu().numpy()[3].tolist() == [-77] * 4


def test_offsets_are_checked_on_the_device(mirror):
    """Offsets that descend or leave the arrays: status 2 for that sample, which reads no point; the others as the mirror."""
    from ogc_amd.data_prepare.scan_ops import moving_counts, moving_stats
    samples = [draw(mirror, 40, 51), draw(mirror, 30, 52), draw(mirror, 50, 53)]
    pc, flow, segm, semantic, offsets, motion = upload(samples)
    want = expect(mirror, samples)
    for bad, where in (([0, 40, 30, 120], 1), ([0, 40, 70, 121], 2), ([-1, 40, 70, 120], 0)):
        off = torch.tensor(bad, dtype=torch.int32, device="cuda")
        got = moving_stats(pc, flow, segm, semantic, off, motion).cpu().numpy()
        assert got[where].tolist() == [0, 0, 0, 2]
        keep = [b for b in range(3) if b != where and bad[b] == int(offsets[b]) and bad[b + 1] == int(offsets[b + 1])]
        assert keep and np.array_equal(got[keep], want[keep])
        with pytest.raises(ValueError, match="sample %d " % where):
            moving_counts(pc, flow, segm, semantic, off, motion)


@pytest.mark.parametrize("axis", (0, 1, 2))
@pytest.mark.parametrize("sign", (1.0, -1.0))
def test_exact_edges(mirror, axis, sign):
    """A residual of exactly moving_thresh is not moving, the next float32 above it is."""
    for d in (np.float32(0.2), np.float32(0.7), np.float32(1.5)):
        pc, flow, segm, semantic, motion, thresh = mirror.edge_sample(d, axis, sign)
        r = mirror.residual_norm(pc, flow, motion)
        assert r[2] == thresh and r[3] > thresh and r[3] == float(np.nextafter(d, np.float32(np.inf)))
        got = run([(pc, flow, segm, semantic, motion)], moving_thresh=thresh)
        assert got[0].tolist() == [3, 4, 1, 0] == list(mirror.moving_mirror(pc, flow, segm, semantic, motion, (), 0, 0.3, thresh)) + [0]
        # the same four points with the threshold one float64 lower: the point on the edge moves too
        got = run([(pc, flow, segm, semantic, motion)], moving_thresh=float(np.nextafter(thresh, 0.0)))
        assert got[0].tolist() == [3, 4, 2, 0]


def test_ground_edge(mirror):
    """y exactly float32(0.3) is foreground, the float32 below it is not."""
    edge = np.float32(0.3)
    below, above = np.nextafter(edge, np.float32(0)), np.nextafter(edge, np.float32(1))
    pc, flow, segm, semantic, motion = draw(mirror, 64, 61, "static")
    pc = pc.copy()
    pc[:, 1] = np.where(np.arange(64) % 2 == 0, -1.0, 2.0)
    pc[[3, 4, 5], 1] = [edge, below, above]
    flow = (pc.astype(np.float64) @ motion[:9].reshape(3, 3).T + motion[9:] - pc).astype(np.float32)
    flow[[3, 4, 5], 0] += np.float32(1.0)                                   # all three would move
    s = (pc, flow, segm, semantic, motion)
    want = expect(mirror, [s])
    n_fg = 32 - 2 + 2                      # the odd rows, without rows 3 and 5, plus rows 3 (on the edge) and 5 (above it)
    assert want[0, 1] == n_fg and want[0, 2] == 2
    assert np.array_equal(run([s]), want)


def test_two_calls_give_identical_bytes(mirror):
    samples = [draw(mirror, n, 70 + n) for n in (1000, 0, 257, 63)]
    tensors = upload(samples)
    from ogc_amd.data_prepare.scan_ops import moving_stats
    a = moving_stats(*tensors, ignore_class_ids=(2, 3), ignore_npoint_thresh=20).cpu().numpy().tobytes()
    b = moving_stats(*tensors, ignore_class_ids=(2, 3), ignore_npoint_thresh=20).cpu().numpy().tobytes()
    assert a == b


def test_empty_batch_and_refusals(mirror):
    from ogc_amd import pointnet2_cuda as nat
    from ogc_amd._lib import OgcOpsError
    from ogc_amd.data_prepare.scan_ops import moving_counts, moving_stats
    empty = (torch.zeros(0, 3, device="cuda"), torch.zeros(0, 3, device="cuda"), torch.zeros(0, dtype=torch.int32, device="cuda"),
             torch.zeros(0, dtype=torch.int32, device="cuda"))
    none = moving_stats(*empty, torch.zeros(1, dtype=torch.int32, device="cuda"), torch.zeros(0, 12, dtype=torch.float64, device="cuda"))
    assert none.shape == (0, 4)
    one = moving_counts(*empty, torch.zeros(2, dtype=torch.int32, device="cuda"), torch.zeros(1, 12, dtype=torch.float64, device="cuda"))
    assert one.tolist() == [[0, 0, 0]]
    pc, flow, segm, semantic, offsets, motion = upload([draw(mirror, 40, 81)])
    with pytest.raises(ValueError):
        moving_stats(pc, flow[:-1], segm, semantic, offsets, motion)
    with pytest.raises(ValueError):
        moving_stats(pc, flow, segm, semantic, offsets, motion.reshape(12))
    with pytest.raises(RuntimeError, match="contiguous"):
        moving_stats(torch.zeros(3, 40, device="cuda").t(), flow, segm, semantic, offsets, motion)
    with pytest.raises(ValueError):
        moving_stats(pc, flow, segm, semantic, offsets, motion, ignore_npoint_thresh=-1)
    with pytest.raises(ValueError):
        moving_stats(pc, flow, segm, semantic, offsets, motion, moving_thresh=float("nan"))
    stats = torch.full((1, 4), -77, dtype=torch.int32, device="cuda")
    ign = torch.zeros(1, dtype=torch.int32, device="cuda")
    for n_ignore, thresh, ground_y, moving_thresh in ((-1, 0, 0.3, 0.2), (0, -1, 0.3, 0.2), (0, 0, float("inf"), 0.2), (0, 0, 0.3, float("nan")),
                                                       (0, 0, 0.3, -0.5)):
        with pytest.raises(OgcOpsError, match="ogc_moving_stats"):
            nat.moving_stats_wrapper(1, 40, offsets, pc, flow, segm, semantic, motion, ign, n_ignore, thresh, ground_y, moving_thresh, stats)
    torch.cuda.synchronize()
    assert stats.cpu().numpy().tolist() == [[-77] * 4]
