"""Scene I/O ("next" row N4 of SURVEY §8f): 3DGS-compatible binary PLY import/export and the checkpoint dictionary
keys of the reference.

PLY layout (threedgrut/export/ply_exporter.py:34-84, model/model.py:671-719): per vertex, little-endian float32
    x y z nx ny nz f_dc_0..2 f_rest_0..44 opacity scale_0..2 rot_0..3
with PRE-activation values (density logit, log-scale, un-normalised wxyz quaternion) and the specular SH stored
CHANNEL-major (f_rest = [R coeffs 1..15 | G ... | B ...]) while the tracer's [N,48] tensor is COEFFICIENT-major
(coefficient k, channel c at 3k+c) — the transpose is the only non-trivial part.  Written with numpy only (the
reference depends on the `plyfile` package, which is not available here).
"""
import numpy as np

_N_SPEC = 15


def _attribute_names():
    names = ["x", "y", "z", "nx", "ny", "nz"] + [f"f_dc_{i}" for i in range(3)] + [f"f_rest_{i}" for i in range(3 * _N_SPEC)]
    return names + ["opacity"] + [f"scale_{i}" for i in range(3)] + [f"rot_{i}" for i in range(4)]


def write_ply(path, positions, density_logit, rotation_raw, log_scale, features48):
    """All arrays pre-activation, features48 coefficient-major [N,48]."""
    n = positions.shape[0]
    f = np.asarray(features48, np.float32).reshape(n, 16, 3)
    albedo = f[:, 0, :]
    spec_channel_major = f[:, 1:, :].transpose(0, 2, 1).reshape(n, 3 * _N_SPEC)
    normals = np.tile(np.array([[0, 0, 1]], np.float32), (n, 1))
    table = np.concatenate([np.asarray(positions, np.float32), normals, albedo, spec_channel_major,
                            np.asarray(density_logit, np.float32).reshape(n, 1), np.asarray(log_scale, np.float32),
                            np.asarray(rotation_raw, np.float32)], axis=1).astype("<f4")
    names = _attribute_names()
    assert table.shape[1] == len(names)
    header = "ply\nformat binary_little_endian 1.0\nelement vertex %d\n" % n
    header += "".join(f"property float {a}\n" for a in names) + "end_header\n"
    with open(path, "wb") as fh:
        fh.write(header.encode("ascii"))
        fh.write(np.ascontiguousarray(table).tobytes())


def write_point_cloud(path, xyz, rgb):
    """A plain point cloud, binary little-endian: per vertex float32 x y z and uchar red green blue.  xyz [P,3]; rgb [P,3] in
    [0, 1] (clamped, rounded to the nearest of 255 steps).  read_ply reads it back as dict(positions, rgb uint8)."""
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    rgb = np.asarray(rgb, np.float32).reshape(-1, 3)
    if xyz.shape[0] != rgb.shape[0]:
        raise ValueError(f"{xyz.shape[0]} points and {rgb.shape[0]} colours")
    table = np.zeros(xyz.shape[0], dtype=[("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("red", "u1"), ("green", "u1"), ("blue", "u1")])
    table["x"], table["y"], table["z"] = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    q = np.rint(np.clip(np.nan_to_num(rgb), 0.0, 1.0) * 255.0).astype(np.uint8)
    table["red"], table["green"], table["blue"] = q[:, 0], q[:, 1], q[:, 2]
    header = "ply\nformat binary_little_endian 1.0\nelement vertex %d\n" % xyz.shape[0]
    header += "".join(f"property float {a}\n" for a in "xyz") + "".join(f"property uchar {a}\n" for a in ("red", "green", "blue")) + "end_header\n"
    with open(path, "wb") as fh:
        fh.write(header.encode("ascii"))
        fh.write(table.tobytes())


def write_mesh(path, vertices, colours, faces):
    """A triangle mesh, binary little-endian: per vertex float32 x y z and uchar red green blue (colours [V,3] in [0, 1], clamped and
    rounded as write_point_cloud does), per face `list uchar int vertex_indices` with three indices.  vertices [V,3], faces [F,3]
    integers in [0, V).  read_ply reads it back as dict(positions, rgb uint8, faces int32 [F,3])."""
    xyz = np.asarray(vertices, np.float32).reshape(-1, 3)
    rgb = np.asarray(colours, np.float32).reshape(-1, 3)
    tri = np.asarray(faces).reshape(-1, 3)
    if xyz.shape[0] != rgb.shape[0]:
        raise ValueError(f"{xyz.shape[0]} vertices and {rgb.shape[0]} colours")
    if tri.size and (not np.issubdtype(tri.dtype, np.integer) or int(tri.min()) < 0 or int(tri.max()) >= xyz.shape[0]):
        raise ValueError(f"faces must be integer indices in [0, {xyz.shape[0]})")
    table = np.zeros(xyz.shape[0], dtype=[("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("red", "u1"), ("green", "u1"), ("blue", "u1")])
    table["x"], table["y"], table["z"] = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    q = np.rint(np.clip(np.nan_to_num(rgb), 0.0, 1.0) * 255.0).astype(np.uint8)
    table["red"], table["green"], table["blue"] = q[:, 0], q[:, 1], q[:, 2]
    records = np.zeros(tri.shape[0], dtype=[("n", "u1"), ("v", "<i4", (3,))])
    records["n"], records["v"] = 3, tri
    header = "ply\nformat binary_little_endian 1.0\nelement vertex %d\n" % xyz.shape[0]
    header += "".join(f"property float {a}\n" for a in "xyz") + "".join(f"property uchar {a}\n" for a in ("red", "green", "blue"))
    header += "element face %d\nproperty list uchar int vertex_indices\nend_header\n" % tri.shape[0]
    with open(path, "wb") as fh:
        fh.write(header.encode("ascii"))
        fh.write(table.tobytes())
        fh.write(records.tobytes())


def read_ply(path):
    """Returns dict(positions, density_logit[N,1], rotation_raw[N,4], log_scale[N,3], features48[N,48]) (pre-activation); of a
    plain point cloud (x y z red green blue and no Gaussian attributes, write_point_cloud) dict(positions, rgb uint8 [N,3]), of a
    mesh (write_mesh: a face element of triangles after the vertices) with faces int32 [F,3] besides."""
    with open(path, "rb") as fh:
        if fh.readline().strip() != b"ply":
            raise ValueError("not a PLY file")
        fmt, n, props, in_vertex = None, None, [], False
        n_faces, face_list = None, None
        while True:
            line = fh.readline()
            if not line:
                raise ValueError("unterminated PLY header")
            tok = line.decode("ascii").split()
            if not tok:
                continue
            if tok[0] == "format":
                fmt = tok[1]
            elif tok[0] == "element":
                in_vertex = tok[1] == "vertex"
                if in_vertex:
                    n = int(tok[2])
                elif tok[1] == "face":
                    n_faces = int(tok[2])
            elif tok[0] == "property" and not in_vertex and n_faces is not None and tok[1] == "list":
                face_list = tok[2:]
            elif tok[0] == "property" and in_vertex:
                if tok[1] == "list":
                    raise ValueError("list properties are not supported on the vertex element")
                props.append((tok[2], {"float": "<f4", "float32": "<f4", "double": "<f8", "float64": "<f8", "uchar": "u1",
                                       "uint8": "u1", "int": "<i4", "int32": "<i4", "short": "<i2", "ushort": "<u2"}[tok[1]]))
            elif tok[0] == "end_header":
                break
        if fmt != "binary_little_endian":
            raise ValueError(f"unsupported PLY format {fmt!r} (binary_little_endian only)")
        data = np.frombuffer(fh.read(n * np.dtype(props).itemsize), dtype=np.dtype(props), count=n)
        faces = None
        if n_faces is not None:
            if face_list is None or face_list[:2] not in (["uchar", "int"], ["uint8", "int32"], ["uchar", "int32"], ["uint8", "int"]):
                raise ValueError("unsupported face element (property list uchar int vertex_indices only)")
            face_type = np.dtype([("n", "u1"), ("v", "<i4", (3,))])
            records = np.frombuffer(fh.read(n_faces * face_type.itemsize), dtype=face_type, count=n_faces)
            if n_faces and not (records["n"] == 3).all():
                raise ValueError("unsupported face element (triangles only)")
            faces = np.ascontiguousarray(records["v"], np.int32).reshape(n_faces, 3)
    col = lambda k: np.asarray(data[k], np.float32)
    names = [p for p, _ in props]
    if all(c in names for c in ("red", "green", "blue")) and not any(p.startswith(("f_rest_", "f_dc_", "scale_", "rot")) for p in names):
        cloud = dict(positions=np.stack([col("x"), col("y"), col("z")], 1).reshape(n, 3),
                     rgb=np.stack([np.asarray(data[c]).astype(np.uint8) for c in ("red", "green", "blue")], 1).reshape(n, 3))
        if faces is not None:
            cloud["faces"] = faces
        return cloud
    rest = sorted((p for p, _ in props if p.startswith("f_rest_")), key=lambda s: int(s.split("_")[-1]))
    if len(rest) != 3 * _N_SPEC:
        raise ValueError(f"expected {3 * _N_SPEC} f_rest_* properties (SH degree 3), found {len(rest)}")
    spec = np.stack([col(k) for k in rest], 1).reshape(n, 3, _N_SPEC).transpose(0, 2, 1)  # -> coefficient-major
    feats = np.concatenate([np.stack([col("f_dc_0"), col("f_dc_1"), col("f_dc_2")], 1)[:, None, :], spec], 1).reshape(n, 48)
    scl = sorted((p for p, _ in props if p.startswith("scale_")), key=lambda s: int(s.split("_")[-1]))
    rot = sorted((p for p, _ in props if p.startswith("rot")), key=lambda s: int(s.split("_")[-1]))
    return dict(positions=np.stack([col("x"), col("y"), col("z")], 1), density_logit=col("opacity")[:, None],
                rotation_raw=np.stack([col(k) for k in rot], 1), log_scale=np.stack([col(k) for k in scl], 1),
                features48=np.ascontiguousarray(feats, np.float32))


def scene_from_ply(path):
    """Activated scene dict (the form scenes.py generators return)."""
    d = read_ply(path)
    q = d["rotation_raw"] / np.maximum(np.linalg.norm(d["rotation_raw"], axis=1, keepdims=True), 1e-12)
    return dict(positions=d["positions"], rotation=q.astype(np.float32), scale=np.exp(d["log_scale"]).astype(np.float32),
                density=(1.0 / (1.0 + np.exp(-d["density_logit"]))).astype(np.float32), features=d["features48"])


def export_native_model(model, path, rows=None):
    """rows: the row indices to write (an int64 tensor on the model's device, as selection.split_rows gives them); None: all."""
    raw, features = model.raw.detach(), model.features.detach()
    if rows is not None:
        raw, features = raw.index_select(0, rows), features.index_select(0, rows)
    raw = raw.cpu().numpy()
    write_ply(path, raw[:, 0:3], raw[:, 3:4], raw[:, 4:8], raw[:, 8:11], features.cpu().numpy())


def checkpoint_dict(model, extra=None):
    """Parameter entries of the reference's checkpoint (model/model.py:107-134 get_model_parameters)."""
    raw = model.raw.detach()
    d = {"positions": raw[:, 0:3].clone(), "rotation": raw[:, 4:8].clone(), "scale": raw[:, 8:11].clone(),
         "density": raw[:, 3:4].clone(), "features_albedo": model.features[:, :3].detach().clone(),
         "features_specular": model.features[:, 3:].detach().clone(), "n_active_features": model.n_active_features,
         "max_n_features": model.max_n_features}
    d.update(extra or {})
    return d
