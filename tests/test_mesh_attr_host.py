"""CPU: the vertex-attribute entry points -- declared, exported and bound; arguments refused before any launch; the PLY writer's colour
and label properties; the renderer's methods refuse what they cannot do."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("sn_rm_vertex_probe_points", "sn_rm_vertex_probe_composite")
OK, INVALID, UNSUPPORTED = 0, -1, -2


def test_symbols_declared_exported_and_bound():
    from sanerf_hq_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "sanerf_hip.h")).read()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for s in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % s, hdr), s
        assert hasattr(lib, s), s
        assert s in _lib.EXPORTED_SYMBOLS
    assert re.search(r"#define SN_ABI_VERSION 12\b", hdr) and _lib.ABI_VERSION == 12 and lib.sn_abi_version() == 12      # symbols were added only
    mk = open(os.path.join(ROOT, "sanerf-hq_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRCS\s*:=.*\bmesh_attr\.hip\b", mk, re.M)


def test_the_library_refuses_arguments_before_any_launch():
    """No device is touched: every call below returns from the host-side checks (the pointers are dummies)."""
    from sanerf_hq_amd import _lib
    l = _lib.lib()
    p = ctypes.c_void_p(4096)
    # probe points
    assert l.sn_rm_vertex_probe_points(None, None, 10, 3, 0, 8, 0.5, 0, None, None, None) == OK            # count 0: no pointer is looked at
    assert l.sn_rm_vertex_probe_points(p, p, 10, 0, 10, 8, 0.5, 0, None, p, None) == INVALID and b"NULL" in l.sn_last_error()
    assert l.sn_rm_vertex_probe_points(p, None, 10, 0, 10, 8, 0.5, 0, p, p, None) == INVALID
    assert l.sn_rm_vertex_probe_points(p, p, 10, 4, 7, 8, 0.5, 0, p, p, None) == INVALID and b"outside" in l.sn_last_error()
    for K in (0, 1, 2, 3, 5, 12, 64):
        assert l.sn_rm_vertex_probe_points(p, p, 10, 0, 10, K, 0.5, 0, p, p, None) == UNSUPPORTED and b"samples" in l.sn_last_error(), K
    for h in (0.0, -1.0, float("inf"), float("nan")):
        assert l.sn_rm_vertex_probe_points(p, p, 10, 0, 10, 8, h, 0, p, p, None) == INVALID and b"step" in l.sn_last_error(), h
    assert l.sn_rm_vertex_probe_points(p, p, 1 << 31, 0, 1 << 28, 16, 0.5, 0, p, p, None) == INVALID and b"2^32" in l.sn_last_error()
    # composite
    assert l.sn_rm_vertex_probe_composite(None, None, None, None, 0, 8, 0.5, 0, 0, None, None, None, None) == OK   # V = 0: a no-op
    assert l.sn_rm_vertex_probe_composite(None, p, p, p, 5, 8, 0.5, 0, 0, p, None, None, None) == INVALID and b"NULL" in l.sn_last_error()
    assert l.sn_rm_vertex_probe_composite(None, None, p, p, 5, 8, 0.5, 0, 0, p, p, None, None) == INVALID
    assert l.sn_rm_vertex_probe_composite(None, p, p, p, 5, 8, 0.5, 0, 0, p, p, p, None) == INVALID and b"labels" in l.sn_last_error()
    assert l.sn_rm_vertex_probe_composite(None, p, ctypes.c_void_p(4100), p, 5, 8, 0.5, 0, 0, p, p, None, None) == INVALID and b"aligned" in l.sn_last_error()
    for K in (0, 2, 6, 24, 33, 128):
        assert l.sn_rm_vertex_probe_composite(None, p, p, p, 5, K, 0.5, 0, 0, p, p, None, None) == UNSUPPORTED and b"samples" in l.sn_last_error(), K
    for h in (0.0, -0.5, float("inf"), float("nan")):
        assert l.sn_rm_vertex_probe_composite(None, p, p, p, 5, 8, h, 0, 0, p, p, None, None) == INVALID, h
    assert l.sn_rm_vertex_probe_composite(None, p, p, p, 1 << 28, 8, 0.5, 0, 0, p, p, None, None) == INVALID and b"2^28" in l.sn_last_error()


def test_the_operators_validate_on_the_host():
    """Bad K, h <= 0, missing normals, mismatched shapes: raised from Python, before a pointer is made (the tensors live on the CPU)."""
    from sanerf_hq_amd import raymarching as rm
    v, n = torch.zeros(5, 3), torch.ones(5, 3)
    for K in (0, 3, 5, 64):
        with pytest.raises(ValueError, match="samples"):
            rm.vertex_probe_points(v, n, K, 0.5)
        with pytest.raises(ValueError, match="samples"):
            rm.vertex_probe_composite(torch.zeros(5, K), torch.zeros(5, K, 15), torch.zeros(5, 3), 0.5)
    for h in (0.0, -1.0, float("inf"), float("nan"), 1e-60, 1e60):               # the last two are 0 and inf in fp32
        with pytest.raises(ValueError, match="probe step"):
            rm.vertex_probe_points(v, n, 8, h)
        with pytest.raises(ValueError, match="probe step"):
            rm.vertex_probe_composite(torch.zeros(5, 8), torch.zeros(5, 8, 15), torch.zeros(5, 3), h)
    with pytest.raises(ValueError, match="normals"):
        rm.vertex_probe_points(v, None, 8, 0.5)
    with pytest.raises(RuntimeError, match=r"\[V,3\]"):
        rm.vertex_probe_points(v, torch.ones(4, 3), 8, 0.5)
    with pytest.raises(ValueError, match="outside"):
        rm.vertex_probe_points(v, n, 8, 0.5, first=3, count=3)
    with pytest.raises(RuntimeError, match="do not match"):
        rm.vertex_probe_composite(torch.zeros(5, 8), torch.zeros(5, 8, 16), torch.zeros(5, 3), 0.5)
    with pytest.raises(RuntimeError, match="uint8"):
        rm.vertex_probe_composite(torch.zeros(5, 8), torch.zeros(5, 8, 15), torch.zeros(5, 3), 0.5, labels=torch.zeros(5, 8, dtype=torch.int64))
    with pytest.raises(ValueError, match="per-sample labels"):
        rm.vertex_probe_composite(torch.zeros(5, 8), torch.zeros(5, 8, 15), torch.zeros(5, 3), 0.5, want_labels=True)
    with pytest.raises(ValueError, match="32-bit"):
        rm.vertex_probe_composite(torch.zeros(5, 8), torch.zeros(5, 8, 15), torch.zeros(5, 3), 0.5, keep_mask=1 << 32)
    with pytest.raises(RuntimeError, match="CUDA"):                              # valid arguments reach the pointer check, and no further
        rm.vertex_probe_points(v, n, 8, 0.5)
    assert rm.PROBE_SAMPLES == (4, 8, 16, 32)


def test_renderer_methods_refuse_what_they_cannot_do():
    from sanerf_hq_amd.nerf import NeRFNetwork, NeRFRenderer
    from sanerf_hq_amd.synth import make_opt
    assert callable(NeRFRenderer.vertex_attributes)
    mesh = {"vertices": torch.zeros(4, 3), "normals": torch.ones(4, 3), "triangles": torch.zeros(0, 3, dtype=torch.int32)}
    model = NeRFNetwork(make_opt(num_steps=[16, 8, 4]))                         # no mask field
    with pytest.raises(RuntimeError, match="inference query"):
        model.vertex_attributes(mesh, 0.01)
    with torch.no_grad():
        with pytest.raises(ValueError, match="normals"):
            model.vertex_attributes({**mesh, "normals": None}, 0.01)
        with pytest.raises(ValueError, match="samples"):
            model.vertex_attributes(mesh, 0.01, samples=6)
        for h in (0.0, -1.0, float("nan"), float("inf")):
            with pytest.raises(ValueError, match="probe_step"):
                model.vertex_attributes(mesh, h)
        with pytest.raises(RuntimeError, match="mask field"):
            model.vertex_attributes(mesh, 0.01, labels=True)
        with pytest.raises(RuntimeError, match="mask field"):
            model.vertex_attributes(mesh, 0.01, instance_ids=[1])
        # extract_mesh refuses before it computes a density
        with pytest.raises(ValueError, match="normals=True"):
            model.extract_mesh(8, normals=False, vertex_colors=True)
        with pytest.raises(ValueError, match="normals=True"):
            model.extract_mesh(8, normals=False, vertex_labels=True)
        with pytest.raises(ValueError, match="probe_samples"):
            model.extract_mesh(8, vertex_colors=True, probe_samples=7)
        with pytest.raises(ValueError, match="probe_step"):
            model.extract_mesh(8, vertex_colors=True, probe_step=0.0)
        with pytest.raises(RuntimeError, match="mask field"):
            model.extract_mesh(8, vertex_labels=True)


# ---- the PLY writer ------------------------------------------------------------------------------------------------------------------------
_SIZES = {"float": ("<f4", 4), "uchar": ("u1", 1)}


def _read_ply(path):
    """A parser of its own for the binary little-endian PLY files save_mesh writes: vertex properties of mixed float / uchar type."""
    raw = open(path, "rb").read()
    end = raw.index(b"end_header\n") + len(b"end_header\n")
    lines = raw[:end].decode("ascii").split("\n")
    assert lines[0] == "ply" and lines[1] == "format binary_little_endian 1.0"
    elements, current = [], None
    for ln in lines[2:]:
        w = ln.split()
        if w[:1] == ["element"]:
            current = dict(name=w[1], count=int(w[2]), props=[])
            elements.append(current)
        elif w[:1] == ["property"]:
            current["props"].append(w[1:])
    assert [e["name"] for e in elements] == ["vertex", "face"]
    vert, face = elements
    dtype = np.dtype([(p[1], _SIZES[p[0]][0]) for p in vert["props"]])
    assert dtype.itemsize == sum(_SIZES[p[0]][1] for p in vert["props"])
    out = {"props": [tuple(p) for p in vert["props"]], "vertex": np.frombuffer(raw, dtype, vert["count"], end), "header_bytes": end,
           "vertex_bytes": dtype.itemsize * vert["count"]}
    pos = end + out["vertex_bytes"]
    assert face["props"] == [["list", "uchar", "int", "vertex_indices"]]
    rec = np.frombuffer(raw, np.dtype([("n", "u1"), ("v", "<i4", (3,))]), face["count"], pos)
    assert (rec["n"] == 3).all()
    out["face"] = rec["v"]
    out["face_bytes"] = 13 * face["count"]
    assert pos + out["face_bytes"] == len(raw)
    return out


def _mesh():
    import mesh_ref as mr
    return mr.isosurface(mr.sphere_volume(9, (4.2, 3.9, 4.1), 2.7), 0.0)


@pytest.mark.parametrize("with_normals", [False, True])
@pytest.mark.parametrize("what", ["colors", "labels", "both"])
def test_ply_round_trip_with_colours_and_labels(tmp_path, with_normals, what):
    from sanerf_hq_amd.nerf.utils import save_mesh
    m = _mesh()
    V = m["vertices"].shape[0]
    rng = np.random.default_rng(5)
    colors = rng.uniform(-0.2, 1.2, (V, 3)).astype(np.float32)
    colors[0] = (np.nan, np.inf, -np.inf)
    colors[1] = (0.25, 0.5, 0.75)                                  # 63.75, 127.5 (a tie: to even), 191.25
    colors[2] = (0.0, 1.0, 254.6 / 255)
    labels = rng.integers(0, 3, V).astype(np.uint8)
    labels[3] = 255
    kw = {}
    if what in ("colors", "both"):
        kw["colors"] = torch.from_numpy(colors)
    if what in ("labels", "both"):
        kw["labels"] = torch.from_numpy(labels)
    path = str(tmp_path / "m.ply")
    save_mesh(path, m["vertices"], m["triangles"], m["normals"] if with_normals else None, **kw)
    got = _read_ply(path)
    want_props = [("float", a) for a in "xyz"] + ([("float", "n" + a) for a in "xyz"] if with_normals else [])
    want_props += [("uchar", c) for c in ("red", "green", "blue")] if "colors" in kw else []
    want_props += [("uchar", "label")] if "labels" in kw else []
    assert got["props"] == want_props
    assert got["vertex_bytes"] == V * (12 + 12 * with_normals + 3 * ("colors" in kw) + ("labels" in kw))
    assert got["face_bytes"] == 13 * m["triangles"].shape[0]
    for i, a in enumerate("xyz"):
        assert np.array_equal(got["vertex"][a], m["vertices"][:, i])
        if with_normals:
            assert np.array_equal(got["vertex"]["n" + a], m["normals"][:, i])
    assert np.array_equal(got["face"], m["triangles"])
    if "colors" in kw:
        rgb = np.stack([got["vertex"][c] for c in ("red", "green", "blue")], axis=1)
        want = np.clip(np.rint(255.0 * np.where(np.isnan(colors), 0.0, colors).astype(np.float64)), 0, 255).astype(np.uint8)
        assert np.array_equal(rgb, want)
        assert rgb[0].tolist() == [0, 255, 0] and rgb[1].tolist() == [64, 128, 191] and rgb[2].tolist() == [0, 255, 255]
    if "labels" in kw:
        assert np.array_equal(got["vertex"]["label"], labels)


def test_uint8_colours_are_taken_as_they_are_and_bad_attributes_are_refused(tmp_path):
    from sanerf_hq_amd.nerf.utils import save_mesh
    m = _mesh()
    V = m["vertices"].shape[0]
    rgb = np.random.default_rng(6).integers(0, 256, (V, 3)).astype(np.uint8)
    path = str(tmp_path / "m.ply")
    save_mesh(path, m["vertices"], m["triangles"], colors=rgb)
    got = _read_ply(path)
    assert np.array_equal(np.stack([got["vertex"][c] for c in ("red", "green", "blue")], axis=1), rgb)
    with pytest.raises(ValueError, match="colors"):
        save_mesh(path, m["vertices"], m["triangles"], colors=rgb[:-1])
    with pytest.raises(ValueError, match="labels"):
        save_mesh(path, m["vertices"], m["triangles"], labels=np.zeros(V + 1, np.uint8))
    with pytest.raises(ValueError, match="labels"):
        save_mesh(path, m["vertices"], m["triangles"], labels=np.zeros(V, np.float32))
    with pytest.raises(ValueError, match="labels"):
        save_mesh(path, m["vertices"], m["triangles"], labels=np.full(V, 256, np.int64))
    save_mesh(path, np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32), colors=np.zeros((0, 3), np.float32), labels=np.zeros(0, np.uint8))
    got = _read_ply(path)
    assert got["vertex"].shape == (0,) and got["face"].shape == (0, 3) and len(got["props"]) == 7


@pytest.mark.parametrize("with_normals", [False, True])
def test_without_attributes_the_file_is_byte_identical_to_the_earlier_layout(tmp_path, with_normals):
    """The earlier writer, restated: header of float properties, [x y z (nx ny nz)] rows, 13-byte faces."""
    from sanerf_hq_amd.nerf.utils import save_mesh
    m = _mesh()
    v, t, n = m["vertices"].astype("<f4"), m["triangles"].astype("<i4"), m["normals"].astype("<f4")
    names = ["x", "y", "z"] + (["nx", "ny", "nz"] if with_normals else [])
    header = ["ply", "format binary_little_endian 1.0", f"element vertex {len(v)}"] + [f"property float {a}" for a in names]
    header += [f"element face {len(t)}", "property list uchar int vertex_indices", "end_header"]
    rows = np.concatenate([v, n], axis=1) if with_normals else v
    faces = b"".join(b"\x03" + row.tobytes() for row in t)
    want = ("\n".join(header) + "\n").encode("ascii") + np.ascontiguousarray(rows).tobytes() + faces
    path = str(tmp_path / "m.ply")
    save_mesh(path, m["vertices"], m["triangles"], m["normals"] if with_normals else None)
    assert open(path, "rb").read() == want
    save_mesh(path, m["vertices"], m["triangles"], m["normals"] if with_normals else None, colors=None, labels=None)
    assert open(path, "rb").read() == want
