"""Writes tests/golden/kittisf_prepare.npz: inputs and expected results for the KITTI Scene Flow preparation
(ogc_amd/csrc/kittisf_prepare.hip, ogc_amd/data_prepare/scan_ops.py::kittisf_unproject, ogc_amd/data_prepare/png16.py).  CPU only.

    python tests/golden/make_kittisf_prepare_golden.py --reference <root of the reference tree>

Unprojection.  The expected clouds and labels are what the reference's own functions give — `load_disp`, `load_op_flow`,
`disp_2_depth`, `pixel2xyz`, `filter_segm` of data_prepare/kittisf/kittisf_util.py, imported with an empty stand-in for the
module `png` (only `load_uint16PNG` needs it; it is replaced by a lookup of the arrays) — under the loop and the masks of
process_kittisf.py:43-87 restated here.  `unproject_mirror` is this repository's own statement of the same per-pixel sequence in
numpy float32, one operation per rounding, in the order include/ogc_ops.h documents; at generation time it must agree with the
reference's functions BIT FOR BIT on every case, every kept value and every label.  The GPU tests apply the mirror to inputs they
draw themselves; they never read the reference.

PNG.  A handful of files as byte strings — grey 8, grey 16 and RGB 16 at 5 x 7, once per filter type and once with mixed filters,
one of them with two IDAT chunks — with the arrays they encode; PIL must read the grey ones back to the same arrays.
"""
import argparse
import io
import json
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
TILE = 1024     # OGC_SCAN_CROP_TILE
SELECT_SEMANTICS = (26, 28)
DEPTH_THRESH = 35.0
CASES = (("a", 25, 41, 11), ("b", 32, 96, 12))       # name, height, width, seed
PNG_KINDS = (("grey8", np.uint8, ()), ("grey16", np.uint16, ()), ("rgb16", np.uint16, (3,)))
PNG_SHAPE = (5, 7)


# ---- the mirror ------------------------------------------------------------------------------------------------------------
def unproject_points(disp1, disp2, flow, P_rect, depth_thresh=DEPTH_THRESH):
    """(keep (H, W) bool, pc1 (H, W, 3) float32, pc2 (H, W, 3) float32): every pixel's two points and whether it is kept."""
    f32 = np.float32
    P = np.asarray(P_rect)
    assert P.dtype == np.float32 and P.shape == (3, 4)
    height, width = disp1.shape
    focal = P[0, 0]
    fb = f32(focal * 0.54)
    p02, p03, p12, p13, p23 = P[0, 2], P[0, 3], P[1, 2], P[1, 3], P[2, 3]
    j = np.tile(np.arange(width, dtype=f32)[None, :], (height, 1))
    i = np.tile(np.arange(height, dtype=f32)[:, None], (1, width))

    def depth(d):
        return fb / (d.astype(f32) / f32(256.0) + f32(1e-5))

    def axis(pix, z, c2, c3):
        return -((pix * (z + p23) - (c2 * z + c3)) / focal)
    z1, z2 = depth(disp1), depth(disp2)
    px2 = j + (flow[..., 0].astype(f32) - f32(32768.0)) / f32(64.0)
    py2 = i + (flow[..., 1].astype(f32) - f32(32768.0)) / f32(64.0)
    pc1 = np.stack([axis(j, z1, p02, p03), axis(i, z1, p12, p13), z1], 2)
    pc2 = np.stack([axis(px2, z2, p02, p03), axis(py2, z2, p12, p13), z2], 2)
    assert pc1.dtype == np.float32 and pc2.dtype == np.float32
    keep = (disp1 > 0) & (disp2 > 0) & (flow[..., 2] == 1) & (z1 < f32(depth_thresh)) & (z2 < f32(depth_thresh))
    return keep, pc1, pc2


def relabel(ids, select_semantics):
    """filter_segm: the ids present whose semantic (id >> 8) is selected -> 1, 2, ... in ascending order, the others -> 0."""
    ids = np.asarray(ids).astype(np.int64)
    present = np.unique(ids)
    chosen = present[np.isin(present >> 8, np.asarray(list(select_semantics), dtype=np.int64))]
    number = np.zeros(65536, dtype=np.int64)                    # the ids are 16-bit samples
    number[chosen] = np.arange(1, chosen.size + 1)
    return number[ids]


def unproject_mirror(disp1, disp2, flow, inst, P_rect, select_semantics=SELECT_SEMANTICS, depth_thresh=DEPTH_THRESH):
    """-> (pc1 (M, 3) float32, pc2 (M, 3) float32, segm (M,) int64, keep_idx (M,) int32), the kept pixels in pixel order."""
    keep, pc1, pc2 = unproject_points(disp1, disp2, flow, P_rect, depth_thresh)
    return pc1[keep], pc2[keep], relabel(inst[keep], select_semantics), np.nonzero(keep.reshape(-1))[0].astype(np.int32)


def p_rect():
    from ogc_amd.utils.synthetic import KITTISF_P_RECT
    return np.asarray(KITTISF_P_RECT, dtype=np.float32)


# ---- the reference ---------------------------------------------------------------------------------------------------------
def load_reference(reference_root):
    sys.modules.setdefault("png", types.ModuleType("png"))      # pypng: only load_uint16PNG uses it, and it is replaced below
    sys.path.insert(0, os.path.join(reference_root, "data_prepare", "kittisf"))
    import kittisf_util
    return kittisf_util


def reference_frame(ref, disp1_raw, disp2_raw, flow_raw, inst_raw, P_rect):
    """process_kittisf.py:41-87 on arrays in place of files."""
    arrays = {"disp1": disp1_raw, "disp2": disp2_raw, "flow": flow_raw}
    ref.load_uint16PNG = lambda key: arrays[key].copy()
    focal_length_pixel = P_rect[0, 0]
    disp1, valid_disp1 = ref.load_disp("disp1")
    depth1 = ref.disp_2_depth(disp1, valid_disp1, focal_length_pixel)
    pc1 = ref.pixel2xyz(depth1, P_rect)
    disp2, valid_disp2 = ref.load_disp("disp2")
    depth2 = ref.disp_2_depth(disp2, valid_disp2, focal_length_pixel)
    valid_disp = np.logical_and(valid_disp1, valid_disp2)
    op_flow, valid_op_flow = ref.load_op_flow("flow")
    vertical, horizontal = op_flow[..., 1], op_flow[..., 0]
    height, width = op_flow.shape[:2]
    px2 = np.zeros((height, width), dtype=np.float32)
    py2 = np.zeros((height, width), dtype=np.float32)
    for i in range(height):
        for j in range(width):
            if valid_op_flow[i, j] and valid_disp[i, j]:
                px2[i, j] = j + horizontal[i, j]
                py2[i, j] = i + vertical[i, j]
    pc2 = ref.pixel2xyz(depth2, P_rect, px=px2, py=py2)
    near_mask = np.logical_and(pc1[..., 2] < 35.0, pc2[..., 2] < 35.0)
    final_mask = np.logical_and(np.logical_and(valid_disp, valid_op_flow), near_mask)
    segm = ref.filter_segm(inst_raw[final_mask].astype(int), select_semantics=list(SELECT_SEMANTICS))
    return pc1[final_mask], pc2[final_mask], segm, final_mask


def build(reference_root):
    sys.path.insert(0, ROOT)
    from PIL import Image

    from ogc_amd.data_prepare import png16
    from ogc_amd.utils.synthetic import make_kittisf_maps
    ref = load_reference(reference_root)
    P = p_rect()
    out, meta = {"P_rect": P}, {"select_semantics": list(SELECT_SEMANTICS), "depth_thresh": DEPTH_THRESH, "tile": TILE, "cases": {},
                                "numpy": np.__version__}
    for name, height, width, seed in CASES:
        disp1, disp2, flow, inst = make_kittisf_maps(height, width, np.random.RandomState(seed))
        want = reference_frame(ref, disp1, disp2, flow, inst, P)
        got = unproject_mirror(disp1, disp2, flow, inst, P)
        assert want[0].dtype == np.float32 and want[1].dtype == np.float32 and want[2].dtype == np.int64
        assert np.array_equal(got[3], np.nonzero(want[3].reshape(-1))[0])
        for k in (0, 1):
            assert np.array_equal(got[k].view(np.int32), want[k].view(np.int32)), "the mirror and the reference differ in bits"
        assert np.array_equal(got[2], want[2])
        valid = int(((disp1 > 0) & (disp2 > 0) & (flow[..., 2] == 1)).sum())
        kept = int(got[3].shape[0])
        assert 0 < kept < valid < height * width and len(set(got[2].tolist())) >= 3
        for key, value in (("disp1", disp1), ("disp2", disp2), ("flow", flow), ("inst", inst), ("pc1", want[0]), ("pc2", want[1]),
                           ("segm", want[2]), ("keep_idx", got[3])):
            out["%s_%s" % (name, key)] = value
        meta["cases"][name] = {"height": height, "width": width, "pixels": height * width, "valid": valid, "kept": kept,
                               "labels": sorted(set(got[2].tolist()))}
        print("case %s: %d x %d = %d pixels, %d valid, %d kept, labels %s: mirror == reference in every bit"
              % (name, height, width, height * width, valid, kept, meta["cases"][name]["labels"]))

    rs = np.random.RandomState(21)
    files = []
    for kind, dtype, tail in PNG_KINDS:
        array = rs.randint(0, np.iinfo(dtype).max + 1, size=PNG_SHAPE + tail).astype(dtype)
        out["png_%s_array" % kind] = array
        variants = [("f%d" % k, [k] * PNG_SHAPE[0], 1) for k in range(5)] + [("mixed", [4, 0, 3, 1, 2], 1)]
        if kind == "rgb16":
            variants.append(("two_idat", [2, 4, 1, 3, 0], 2))
        for tag, filters, idat in variants:
            data = png16.encode_png(array, filters, idat_chunks=idat)
            assert data.count(b"IDAT") == idat
            if not tail:       # PIL reads 8- and 16-bit grey intact
                assert np.array_equal(np.array(Image.open(io.BytesIO(data))), array), (kind, tag)
            out["png_%s_%s" % (kind, tag)] = np.frombuffer(data, dtype=np.uint8)
            files.append("png_%s_%s" % (kind, tag))
    meta["png_files"] = files
    return out, meta


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="root of the reference tree (its data_prepare/kittisf/kittisf_util.py is imported)")
    args = ap.parse_args()
    out, meta = build(args.reference)
    path = os.path.join(HERE, "kittisf_prepare.npz")
    np.savez_compressed(path, meta=json.dumps(meta), **out)
    print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
