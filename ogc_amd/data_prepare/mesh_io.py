"""Readers and writers of the OGC-DR preparation, numpy only: Wavefront .obj triangle meshes (what build_ogcdr.py exports and
sample_pointcloud.py loads with trimesh) and .pcd point clouds (what build_ogcdrsv.py saves and collect_segm.py loads with open3d)."""
import numpy as np


def read_obj(path):
    """A Wavefront .obj as (vertices (V, 3) float64, faces (F, 3) int32).  `v x y z [...]` and `f a b c [...]` lines are read;
    an index may be `a`, `a/b`, `a//c` or `a/b/c` (the vertex index is the first field) and may be negative (relative to the
    vertices read so far); a polygon is triangulated as a fan around its first vertex.  Every other line is ignored.  No vertex
    is merged or dropped and no face removed."""
    vertices, faces = [], []
    with open(path, "r") as f:
        for number, line in enumerate(f, 1):
            fields = line.split()
            if not fields:
                continue
            if fields[0] == "v":
                if len(fields) < 4:
                    raise ValueError("%s:%d: a vertex needs three coordinates" % (path, number))
                vertices.append((float(fields[1]), float(fields[2]), float(fields[3])))
            elif fields[0] == "f":
                if len(fields) < 4:
                    raise ValueError("%s:%d: a face needs three vertices" % (path, number))
                corner = []
                for field in fields[1:]:
                    idx = int(field.split("/")[0])
                    idx = idx - 1 if idx > 0 else len(vertices) + idx
                    if idx < 0 or idx >= len(vertices):     # (an index 0 lands on len(vertices))
                        raise ValueError("%s:%d: vertex index %s outside the %d vertices read so far" % (path, number, field, len(vertices)))
                    corner.append(idx)
                for k in range(1, len(corner) - 1):
                    faces.append((corner[0], corner[k], corner[k + 1]))
    return (np.asarray(vertices, dtype=np.float64).reshape(-1, 3), np.asarray(faces, dtype=np.int32).reshape(-1, 3))


def write_obj(path, vertices, faces):
    """vertices (V, 3) and faces, an (F, K >= 3) array or a list of index sequences of differing lengths -> a Wavefront .obj;
    coordinates as their shortest exact decimal form, so that read_obj returns the float64 values it was given."""
    vertices = np.asarray(vertices, dtype=np.float64)
    with open(path, "w") as f:
        for v in vertices:
            f.write("v %s %s %s\n" % (repr(float(v[0])), repr(float(v[1])), repr(float(v[2]))))
        for face in faces:
            f.write("f " + " ".join(str(int(i) + 1) for i in face) + "\n")


_PCD_TYPES = {("F", 4): "<f4", ("F", 8): "<f8", ("I", 1): "<i1", ("I", 2): "<i2", ("I", 4): "<i4", ("I", 8): "<i8",
              ("U", 1): "<u1", ("U", 2): "<u2", ("U", 4): "<u4", ("U", 8): "<u8"}


def read_pcd(path):
    """The x, y, z fields of a .pcd file as (N, 3) float32.  `DATA ascii` and `DATA binary` are read; x, y and z must be float32
    fields (`SIZE 4`, `TYPE F`, `COUNT 1`), other fields are skipped.  `DATA binary_compressed` is refused by name."""
    with open(path, "rb") as f:
        raw = f.read()
    header, pos = {}, 0
    while True:
        end = raw.find(b"\n", pos)
        if end < 0:
            raise ValueError("%s: no DATA line" % path)
        line = raw[pos:end].decode("ascii", "replace").strip()
        pos = end + 1
        if not line or line.startswith("#"):
            continue
        key, _, value = line.partition(" ")
        header[key.upper()] = value.split()
        if key.upper() == "DATA":
            break
    kind = header["DATA"][0].lower() if header["DATA"] else ""
    if kind == "binary_compressed":
        raise ValueError("%s: DATA binary_compressed is not supported; save the cloud as `binary` or `ascii`" % path)
    if kind not in ("ascii", "binary"):
        raise ValueError("%s: DATA %s is not supported" % (path, kind))
    try:
        names = header["FIELDS"]
        sizes = [int(s) for s in header["SIZE"]]
        types = header["TYPE"]
        counts = [int(c) for c in header.get("COUNT", ["1"] * len(names))]
        n_point = int(header["POINTS"][0]) if "POINTS" in header else int(header["WIDTH"][0]) * int(header["HEIGHT"][0])
    except (KeyError, IndexError, ValueError):
        raise ValueError("%s: incomplete header (FIELDS, SIZE, TYPE and POINTS or WIDTH x HEIGHT are needed)" % path) from None
    if not (len(sizes) == len(types) == len(counts) == len(names)):
        raise ValueError("%s: FIELDS, SIZE, TYPE and COUNT differ in length" % path)
    for axis in "xyz":
        if axis not in names:
            raise ValueError("%s: no field %s" % (path, axis))
        k = names.index(axis)
        if (sizes[k], types[k].upper(), counts[k]) != (4, "F", 1):
            raise ValueError("%s: field %s must be one float32 (SIZE 4, TYPE F, COUNT 1)" % (path, axis))
    if kind == "ascii":
        columns = np.cumsum([0] + counts)
        rows = raw[pos:].decode("ascii", "replace").split()
        if len(rows) < n_point * columns[-1]:
            raise ValueError("%s: %d values, %d points of %d need %d" % (path, len(rows), n_point, columns[-1], n_point * columns[-1]))
        table = np.asarray(rows[:n_point * columns[-1]]).reshape(n_point, columns[-1])
        return np.stack([table[:, columns[names.index(axis)]].astype(np.float32) for axis in "xyz"], 1).reshape(n_point, 3)
    try:
        dtype = np.dtype([("f%d" % k, _PCD_TYPES[(types[k].upper(), sizes[k])], (counts[k],)) for k in range(len(names))])
    except KeyError:
        raise ValueError("%s: a field has a SIZE / TYPE pair that is not supported" % path) from None
    if len(raw) - pos < n_point * dtype.itemsize:
        raise ValueError("%s: %d bytes of data, %d points of %d bytes need %d" % (path, len(raw) - pos, n_point, dtype.itemsize,
                                                                                   n_point * dtype.itemsize))
    table = np.frombuffer(raw, dtype=dtype, count=n_point, offset=pos)
    return np.stack([table["f%d" % names.index(axis)][:, 0] for axis in "xyz"], 1).astype(np.float32).reshape(n_point, 3)


def write_pcd(path, points):
    """points (N, 3) -> a .pcd with the float32 fields x y z, `DATA binary`."""
    points = np.ascontiguousarray(points, dtype="<f4").reshape(-1, 3)
    header = ("# .PCD v0.7 - Point Cloud Data file format\nVERSION 0.7\nFIELDS x y z\nSIZE 4 4 4\nTYPE F F F\nCOUNT 1 1 1\n"
              "WIDTH %d\nHEIGHT 1\nVIEWPOINT 0 0 0 1 0 0 0\nPOINTS %d\nDATA binary\n" % (points.shape[0], points.shape[0]))
    with open(path, "wb") as f:
        f.write(header.encode("ascii"))
        f.write(points.tobytes())
