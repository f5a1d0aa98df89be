"""ogc_slot_confidence (ogc_amd/csrc/seg_conf.hip) and ogc_amd.metrics.seg_conf on the device, against float64 numpy on the same
fp32 inputs.

Truth: per point the arg-max slot (the first maximum; a NaN counts as the maximum and the first NaN wins); the present slots in
ascending order; per present slot math.fsum (the exactly rounded sum) of the widened mask[p, slot] over its own points, divided
by the size in float64 and rounded to float32.

Cases (B, n, k), T = OGC_SLOT_CONF_TILE and P = OGC_SLOT_CONF_MAX_PARTIALS read from the header: (1, 1, 1) the smallest;
(2, 63, 3); (2, 257, 7); (3, T + 1, 5) a second workgroup of one point; (2, 3T + 17, 18) four workgroups, sample 0 with one
column set to 1.0 in every row (exactly one slot present), sample 1 with all 18 present; (1, 2T, 64) whole tiles, all 64 lanes
of the finish and rows read as float4; and (P // 3 - 2, 4T + 5, 2): five tiles per sample, more than P in the batch, so that a
workgroup takes two tiles and three workgroups share a sample.  Masks are the softmax of seeded normal logits.

Bounds: hard, slots, sizes and n_object exactly the truth.  conf within 1 float32 ulp of it: the kernel's fp64 sum of n <= 2**17
non-negative terms is within n * 2**-53, about 1.5e-11 relative, of the exact sum, far below the float32 half-ulp of 2**-25, so
the two float32 roundings can differ by one ulp and no more.
"""
import math
import os
import re

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 16


def _header_constant(name):
    text = open(os.path.join(ROOT, "include", "ogc_ops.h")).read()
    return int(re.search(r"#define %s (\d+)" % name, text).group(1))


T = _header_constant("OGC_SLOT_CONF_TILE")
P = _header_constant("OGC_SLOT_CONF_MAX_PARTIALS")
CASES = {"smallest": (1, 1, 1), "n63": (2, 63, 3), "n257": (2, 257, 7), "tile_plus_1": (3, T + 1, 5),
         "three_tiles_17": (2, 3 * T + 17, 18), "two_tiles_k64": (1, 2 * T, 64), "two_tiles_per_wg": (P // 3 - 2, 4 * T + 5, 2)}
ONE_SLOT_COLUMN = 11   # of sample 0 of three_tiles_17


def draw(B, n, k, seed):
    rng = np.random.default_rng(seed)
    logits = rng.standard_normal((B, n, k)).astype(np.float32)
    e = np.exp(logits - logits.max(axis=2, keepdims=True))
    return (e / e.sum(axis=2, keepdims=True)).astype(np.float32)


def truth(mask):
    """-> hard (B, n) i32, slots / sizes (B, k) i32, conf (B, k) f32, n_object (B,) i32."""
    B, n, k = mask.shape
    nan = np.isnan(mask)
    clean = np.where(nan, -np.inf, mask)
    # the first maximum of a row without NaN, the first NaN of a row with one
    hard = np.where(nan.any(axis=2), nan.argmax(axis=2), clean.argmax(axis=2)).astype(np.int32)
    slots, sizes = np.full((B, k), -1, np.int32), np.zeros((B, k), np.int32)
    conf, n_object = np.zeros((B, k), np.float32), np.zeros(B, np.int32)
    for b in range(B):
        present = np.unique(hard[b])
        n_object[b] = len(present)
        for j, s in enumerate(present):
            own = mask[b, hard[b] == s, s].astype(np.float64)
            slots[b, j], sizes[b, j] = s, own.shape[0]
            conf[b, j] = np.float32(math.fsum(own.tolist()) / own.shape[0])
    return dict(hard=hard, slots=slots, sizes=sizes, conf=conf, n_object=n_object)


def run(d_mask, with_hard=True):
    """The entry point through its wrapper: every output pre-filled with garbage, between guard elements that must survive."""
    from ogc_amd import pointnet2_cuda as nat
    B, n, k = d_mask.shape
    shapes = dict(hard=(B, n), slots=(B, k), sizes=(B, k), conf=(B, k), n_object=(B,))
    flat, out = {}, {}
    for f, shape in shapes.items():
        size = int(np.prod(shape))
        if f == "conf":
            flat[f] = torch.full((size + 2 * GUARD,), float("nan"), dtype=torch.float32, device="cuda")
        else:
            flat[f] = torch.full((size + 2 * GUARD,), -123456789, dtype=torch.int32, device="cuda")
        out[f] = flat[f][GUARD:GUARD + size].view(*shape)
    nat.slot_confidence_wrapper(B, n, k, d_mask, out["hard"] if with_hard else None, out["slots"], out["sizes"], out["conf"],
                                out["n_object"])
    got = {}
    for f, t in flat.items():
        a = t.cpu().numpy()
        edge = np.concatenate([a[:GUARD], a[-GUARD:]])
        assert np.isnan(edge).all() if f == "conf" else (edge == -123456789).all(), "guard elements of %s" % f
        got[f] = a[GUARD:-GUARD].reshape(shapes[f])
    if not with_hard:
        assert (got.pop("hard") == -123456789).all(), "hard was NULL and must not be written"
    return got


def ulps(got, want):
    """Distance in float32 steps between arrays of non-negative finite floats."""
    assert np.isfinite(got).all() and np.isfinite(want).all() and (got >= 0).all() and (want >= 0).all()
    return np.abs(got.view(np.int32).astype(np.int64) - want.view(np.int32).astype(np.int64))


def check(got, want, label):
    for f in ("hard", "slots", "sizes", "n_object"):
        if f in got:
            assert got[f].dtype == np.int32 and np.array_equal(got[f], want[f]), (label, f)
    assert got["conf"].dtype == np.float32
    nan = np.isnan(want["conf"])
    assert np.array_equal(np.isnan(got["conf"]), nan), label
    d = ulps(np.where(nan, 0, got["conf"]).astype(np.float32), np.where(nan, 0, want["conf"]).astype(np.float32))
    print(label, "n_object", want["n_object"][:4].tolist(), "conf: worst distance", int(d.max()), "ulp, bound 1")
    assert d.max() <= 1, label


def same_bits(a, b, fields=("hard", "slots", "sizes", "conf", "n_object")):
    return all(a[f].tobytes() == b[f].tobytes() for f in fields if f in a and f in b)


@pytest.fixture(scope="module")
def cases():
    """name -> dict(mask, d_mask, want = the float64 truth, got = ONE run on the device): shared by the tests, left unchanged."""
    out = {}
    for i, (name, (B, n, k)) in enumerate(CASES.items()):
        mask = draw(B, n, k, 4100 + i)
        if name == "three_tiles_17":
            mask[0, :, ONE_SLOT_COLUMN] = 1.0   # every other entry of a softmax row of 18 is below 1
        d_mask = torch.from_numpy(mask).cuda()
        out[name] = dict(mask=mask, d_mask=d_mask, want=truth(mask), got=run(d_mask))
    return out


@pytest.mark.parametrize("name", list(CASES))
def test_labels_slots_and_sizes_are_exact_and_confidences_within_one_ulp(cases, name):
    c = cases[name]
    B, n, k = CASES[name]
    want = c["want"]
    if name == "three_tiles_17":   # the generator's job, asserted about the truth first
        assert want["n_object"].tolist() == [1, k] and want["slots"][0, 0] == ONE_SLOT_COLUMN and want["sizes"][0, 0] == n
        assert want["conf"][0, 0] == 1.0 and want["slots"][1].tolist() == list(range(k))
    assert (want["sizes"].sum(axis=1) == n).all() and (want["n_object"] >= 1).all()
    check(c["got"], want, name)
    # behind the present slots: -1 / 0 / 0
    for b in range(B):
        m = want["n_object"][b]
        assert (c["got"]["slots"][b, m:] == -1).all() and (c["got"]["sizes"][b, m:] == 0).all()
        assert c["got"]["conf"][b, m:].tobytes() == np.zeros(k - m, np.float32).tobytes()


def test_python_layer_returns_the_kernels_outputs(cases):
    from ogc_amd.metrics.seg_conf import SlotConfidence, pseudo_label_confidences, slot_confidence_batch
    c = cases["three_tiles_17"]
    res = slot_confidence_batch(c["d_mask"])
    assert isinstance(res, SlotConfidence) and res._fields == ("hard", "slots", "sizes", "conf", "n_object")
    assert all(t.is_cuda for t in res)
    assert same_bits({f: getattr(res, f).cpu().numpy() for f in res._fields}, c["got"])
    per_sample = pseudo_label_confidences(c["d_mask"])
    assert isinstance(per_sample, list) and len(per_sample) == 2
    for b, conf in enumerate(per_sample):
        m = int(c["got"]["n_object"][b])
        assert conf.dtype == np.float32 and conf.shape == (m,) and conf.tobytes() == c["got"]["conf"][b, :m].tobytes()
    # a transposed view is made contiguous by the Python layer
    view = c["d_mask"].transpose(1, 2).contiguous().transpose(1, 2)
    assert not view.is_contiguous()
    assert slot_confidence_batch(view).conf.cpu().numpy().tobytes() == c["got"]["conf"].tobytes()


def _with_ties_and_nans(c):
    """The case's masks with, in some rows, the maximum copied to a lower and to a higher column, one NaN before or behind the
    maximum, and two NaNs."""
    mask = c["mask"].copy()
    B, n, k = mask.shape
    hard = c["want"]["hard"]
    rows = np.arange(n)
    for b in range(B):
        top = mask[b, rows, hard[b]]
        for r in range(0, n, 5):            # a tie: the maximum copied to another column
            mask[b, r, (hard[b, r] + 1 + r) % k] = top[r]
        for r in range(3, n, 17):           # one NaN
            mask[b, r, (hard[b, r] + 2 + r) % k] = np.nan
        for r in range(4, n, 29):           # two NaNs: the first wins
            mask[b, r, r % k] = np.nan
            mask[b, r, (r + 3) % k] = np.nan
    return mask


@pytest.mark.parametrize("name", ("n257", "tile_plus_1", "two_tiles_k64"))
def test_ties_and_nans_follow_the_rule_and_agree_with_seg_eval(cases, name):
    from ogc_amd.metrics.seg_eval import seg_eval_batch
    c = cases[name]
    mask = _with_ties_and_nans(c)
    B, n, k = mask.shape
    want = truth(mask)
    # in a row with two equal maxima and no NaN the lower slot wins
    r = 0
    tied = np.flatnonzero(mask[0, r] == np.nanmax(mask[0, r]))
    assert len(tied) >= min(2, k) and not np.isnan(mask[0, r]).any() and want["hard"][0, r] == tied[0]
    assert np.isnan(want["conf"]).any()
    d_mask = torch.from_numpy(mask).cuda()
    got = run(d_mask)
    check(got, want, name + " with ties and NaNs")
    result = seg_eval_batch(torch.zeros(B, n, dtype=torch.int32, device="cuda"), d_mask, 0)
    assert np.array_equal(result.hard.cpu().numpy(), got["hard"])
    assert np.array_equal(seg_eval_batch(torch.zeros(B, n, dtype=torch.int32, device="cuda"), c["d_mask"], 0).hard.cpu().numpy(),
                          c["got"]["hard"])


def test_a_nan_stays_in_the_slot_that_owns_its_point(cases):
    c = cases["tile_plus_1"]               # three samples, two workgroups each; point T is the second workgroup's only one
    B, n, k = CASES["tile_plus_1"]
    # in the point's own arg-max slot: labels and sizes stay, one confidence becomes NaN, nothing else moves a bit
    for p in (7, T):
        mask = c["mask"].copy()
        s = int(c["want"]["hard"][1, p])
        mask[1, p, s] = np.nan
        got = run(torch.from_numpy(mask).cuda())
        j = int(np.flatnonzero(c["got"]["slots"][1] == s)[0])
        assert got["hard"][1, p] == s and np.isnan(got["conf"][1, j])
        assert same_bits(got, c["got"], ("hard", "slots", "sizes", "n_object"))
        others = np.ones((B, k), bool)
        others[1, j] = False
        assert got["conf"][others].tobytes() == c["got"]["conf"][others].tobytes()
    # in another slot: the point moves to the NaN's slot; the other samples do not move a bit
    mask = c["mask"].copy()
    s = (int(c["want"]["hard"][1, T]) + 1) % k
    mask[1, T, s] = np.nan
    got, want = run(torch.from_numpy(mask).cuda()), truth(mask)
    j = int(np.flatnonzero(want["slots"][1] == s)[0])
    assert got["hard"][1, T] == s and np.isnan(got["conf"][1, j]) and np.isnan(got["conf"][1]).sum() == 1
    check(got, want, "a NaN in another slot")
    for f in got:
        assert got[f][[0, 2]].tobytes() == c["got"][f][[0, 2]].tobytes(), f


@pytest.mark.parametrize("name", ("n63", "three_tiles_17", "two_tiles_k64", "two_tiles_per_wg"))
def test_calls_repeat_to_the_bit_with_and_without_hard(cases, name):
    c = cases[name]
    assert same_bits(run(c["d_mask"]), c["got"])
    without = run(c["d_mask"], with_hard=False)
    assert "hard" not in without and same_bits(without, c["got"], ("slots", "sizes", "conf", "n_object"))


def test_a_misaligned_mask_gives_the_same_bits(cases):
    c = cases["two_tiles_k64"]             # k % 4 == 0: float4 rows when the base is 16-byte aligned, scalar loads otherwise
    B, n, k = CASES["two_tiles_k64"]
    flat = torch.empty(B * n * k + 1, dtype=torch.float32, device="cuda")
    flat[1:] = c["d_mask"].reshape(-1)
    shifted = flat[1:].view(B, n, k)
    assert shifted.is_contiguous() and shifted.data_ptr() % 16 == 4 and c["d_mask"].data_ptr() % 16 == 0
    assert same_bits(run(shifted), c["got"])


def test_graph_capture_replays_the_eager_call(cases):
    from ogc_amd.metrics.seg_conf import slot_confidence_batch
    c = cases["three_tiles_17"]
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = slot_confidence_batch(c["d_mask"])   # an allocation by the library or a synchronisation would end the capture
    for t in captured:
        t.fill_(-1)
    graph.replay()
    torch.cuda.synchronize()
    assert same_bits({f: getattr(captured, f).cpu().numpy() for f in captured._fields}, c["got"])


def test_argument_checks(cases):
    from ogc_amd import _lib
    from ogc_amd.metrics.seg_conf import slot_confidence_batch
    OK, INVALID = 0, -1
    c = cases["n63"]
    B, n, k = CASES["n63"]
    fn = _lib.load().ogc_slot_confidence
    fn.argtypes, fn.restype = _lib.SIGNATURES["ogc_slot_confidence"], _lib._int
    i32 = lambda *s: torch.full(s, -5, dtype=torch.int32, device="cuda")  # noqa: E731
    hard, slots, sizes, n_object = i32(B, n), i32(B, 64), i32(B, 64), i32(B)
    conf = torch.full((B, 64), -5.0, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    ptr = lambda t: t.data_ptr()  # noqa: E731

    def call(B_, n_, k_, conf_ptr=ptr(conf), mask_ptr=ptr(c["d_mask"])):
        return fn(B_, n_, k_, mask_ptr, ptr(hard), ptr(slots), ptr(sizes), conf_ptr, ptr(n_object), stream)

    assert call(B, n, 0) == INVALID
    assert call(B, n, 65) == INVALID
    assert call(B, 0, k) == INVALID
    assert call(B, n, k, conf_ptr=None) == INVALID
    assert call(B, n, k, mask_ptr=None) == INVALID
    assert call(-1, n, k) == INVALID
    assert b"ogc_slot_confidence" in _lib.load().ogc_last_error()
    assert call(0, n, k) == OK and call(0, 0, 0, conf_ptr=None) == OK
    torch.cuda.synchronize()
    for t in (hard, slots, sizes, n_object):            # nothing was launched
        assert bool((t == -5).all())
    assert bool((conf == -5.0).all())
    assert call(B, n, k) == OK
    torch.cuda.synchronize()
    assert np.array_equal(hard.cpu().numpy(), c["got"]["hard"]) and np.array_equal(n_object.cpu().numpy(), c["got"]["n_object"])

    d = c["d_mask"]
    with pytest.raises(TypeError):
        slot_confidence_batch(d.double())
    with pytest.raises(TypeError):
        slot_confidence_batch(c["mask"])
    with pytest.raises(ValueError):
        slot_confidence_batch(d[0])
    with pytest.raises(ValueError):
        slot_confidence_batch(torch.zeros(1, 8, 65, device="cuda"))
    with pytest.raises(ValueError):
        slot_confidence_batch(torch.zeros(1, 8, 0, device="cuda"))
    with pytest.raises(RuntimeError) as err:
        slot_confidence_batch(d.cpu())
    assert "no CPU path" in str(err.value)
