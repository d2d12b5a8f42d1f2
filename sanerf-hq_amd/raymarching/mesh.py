"""Geometry export (mesh.hip, mesh_clean.hip, mesh_split.hip, mesh_simplify.hip, mesh_smooth.hip, mesh_raster.hip, mesh_attr.hip): lattice
positions, marching tetrahedra on a density lattice, the clean-up of the mesh, its split into one mesh per instance label, its simplification,
its smoothing, its image from a camera, and the surface probes that give its vertices a colour and an instance label.

    lattice_points     positions of a window of the vertices of an nx x ny x nz lattice, optionally contracted -- no meshgrid per chunk
    isosurface         volume [nx,ny,nz], iso -> {"vertices" [V,3], "normals" [V,3] or None, "triangles" [T,3] int32}
    mesh_components    triangles [T,3], V -> labels, triangle and vertex counts per connected component
    mesh_clean         a mesh without its small components (floaters, label noise): by triangle count and / or the largest k
    mesh_split         a mesh with a label per vertex -> one stand-alone mesh per instance id (tests/mesh_split_ref.py restates it)
    mesh_simplify      uniform vertex clustering: one vertex per occupied cell of a coarse lattice
    mesh_smooth        Taubin / Laplacian smoothing on integers, and the geometric normals of the result; mesh_vertex_normals alone
    mesh_rasterize     the mesh seen from one pinhole camera through a depth buffer: triangle id, depth, mask, interpolated attributes
    vertex_probe_points, vertex_probe_composite   K samples of a short ray into the surface at every vertex; their gated re-integration
                       into the colour head's input, the coverage and the voted label (tests/mesh_attr_ref64.py states it in fp64)
include/sanerf_hip.h states the definitions (inside test, edge slots, Kuhn tetrahedra, orientation from the table, both orders, normals;
valid triangles, components, keys, selection, the filtered mesh's order; cells, triangle classes, the integer sums; quantisation, corner
pairs, open vertices, the half-step, the geometric normals; the camera, placed vertices, drawn triangles, the fill rule, the depth key, the
resolve); tests/mesh_ref.py, tests/mesh_clean_ref.py, tests/mesh_simplify_ref.py, tests/mesh_smooth_ref.py and tests/mesh_raster_ref.py
restate them in numpy."""
from __future__ import annotations

from typing import Sequence

import torch

from .. import _buffers, _lib
from ._args import _f32

ISOSURFACE_MAX_VERTICES = (1 << 31) - 1        # lattice vertices of one volume; mesh vertices of one result (int32 triangle indices)


def _triple(v, name, kind=float):
    v = [kind(x) for x in (v.tolist() if torch.is_tensor(v) else v)]
    if len(v) != 3:
        raise ValueError(f"{name} must have 3 entries, got {len(v)}")
    return v


# ---- what the count / emit families share -------------------------------------------------------------------------------------------------
def _workspace(name, need, device, empty_ok=False):
    """The module's one scratch buffer `name` of this device with `need` bytes; need = 0 is the library's refusal of the sizes."""
    if need == 0 and not empty_ok:
        raise RuntimeError(f"{name}: " + _lib.lib().sn_last_error().decode())
    return _buffers.scratch(name, device, max(need, 16))


def _read_counts(counts):
    """The two uint32 totals of a count entry, read back from their int32 tensor."""
    return tuple(int(c) & 0xFFFFFFFF for c in counts.tolist())


def _capacities(what, cap_v, cap_t, per_vertex, out_triangles):
    """cap_v, cap_t defaulted to the rows of per_vertex[0] and of out_triangles; every buffer of per_vertex (None: one that is needed and
    missing) has at least cap_v rows, out_triangles at least cap_t."""
    cap_v = per_vertex[0].shape[0] if cap_v is None else int(cap_v)
    cap_t = out_triangles.shape[0] if cap_t is None else int(cap_t)
    if cap_t > out_triangles.shape[0] or any(b is None or b.shape[0] < cap_v for b in per_vertex):
        raise ValueError(f"{what}: a capacity exceeds its buffer")
    return cap_v, cap_t


def _rows3(what, *tensors):
    if any(t is not None and tuple(t.shape[1:]) != (3,) for t in tensors):
        raise RuntimeError(f"{what}: vertices, normals and triangles are [n,3]")


def _vertices_v3(vertices, what):
    if vertices.dim() != 2 or vertices.shape[1] != 3:
        raise RuntimeError(f"{what}: vertices must be [V,3], got {tuple(vertices.shape)}")


def _empty_mesh(nv, nt, device, normals):
    return {"vertices": torch.empty(nv, 3, device=device, dtype=torch.float32),
            "normals": torch.empty(nv, 3, device=device, dtype=torch.float32) if normals else None,
            "triangles": torch.empty(nt, 3, device=device, dtype=torch.int32)}


def lattice_points(origin: Sequence[float], step: Sequence[float], shape: Sequence[int], first: int = 0, count: int | None = None,
                   contract: bool = False, device=None) -> torch.Tensor:
    """xyz [count,3] of the lattice vertices first .. first + count - 1 (default: to the end) of a lattice of `shape` = (nx, ny, nz); linear
    index (x ny + y) nz + z.  p = origin + float(i) * step per axis, product and sum rounded separately, then -- contract=True -- through
    raymarching.contract's arithmetic: bit-equal to that operator on the same lattice made with torch."""
    nx, ny, nz = _triple(shape, "shape", int)
    total = nx * ny * nz
    count = total - first if count is None else int(count)
    if first < 0 or count < 0 or first + count > total:
        raise ValueError(f"lattice_points: vertices {first} .. {first + count - 1} outside the lattice of {total}")
    device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    xyz = torch.empty(count, 3, device=device, dtype=torch.float32)
    _lib.check(_lib.lib().sn_rm_lattice_points(_lib.host_f32(_triple(origin, "origin")), _lib.host_f32(_triple(step, "step")), nx, ny, nz,
                                               int(first), count, int(bool(contract)), _lib.dev(xyz, "xyz"), _lib.stream()),
               "sn_rm_lattice_points")
    return xyz


def isosurface_counts(volume: torch.Tensor, iso: float):
    """The first half of isosurface(): (counts, workspace) with counts = uint32 {n_vertices, n_triangles} as an int32 [2] tensor on the device
    (nothing is read back) and the workspace that isosurface_emit() takes.  The workspace is the module's one buffer per device: the next
    call on that device reuses it."""
    vol = _f32(volume)
    if vol.dim() != 3:
        raise RuntimeError(f"isosurface: volume must be [nx,ny,nz], got {tuple(vol.shape)}")
    nx, ny, nz = vol.shape
    L = _lib.lib()
    ws = _workspace("isosurface", int(L.sn_rm_isosurface_workspace_bytes(nx, ny, nz)), vol.device)
    counts = torch.empty(2, device=vol.device, dtype=torch.int32)
    _lib.check(L.sn_rm_isosurface_count(_lib.dev(vol, "volume"), nx, ny, nz, float(iso), ws.data_ptr(), ws.numel(),
                                        _lib.dev(counts, "counts", torch.int32), _lib.stream()), "sn_rm_isosurface_count")
    return counts, ws


def isosurface_emit(volume: torch.Tensor, iso: float, origin, step, workspace: torch.Tensor, vertices: torch.Tensor, normals, triangles: torch.Tensor,
                    cap_v: int | None = None, cap_t: int | None = None):
    """The second half: fills vertices [>= cap_v, 3] f32, normals (same shape, or None) and triangles [>= cap_t, 3] int32 from the workspace
    isosurface_counts() left.  Capacities below the counts truncate: the stored prefix is the full result's."""
    vol = _f32(volume)
    nx, ny, nz = vol.shape
    cap_v, cap_t = _capacities("isosurface_emit", cap_v, cap_t, [vertices] + ([] if normals is None else [normals]), triangles)
    _rows3("isosurface_emit", vertices, triangles, normals)
    _lib.check(_lib.lib().sn_rm_isosurface_emit(_lib.dev(vol, "volume"), nx, ny, nz, float(iso), _lib.host_f32(_triple(origin, "origin")),
                                                _lib.host_f32(_triple(step, "step")), workspace.data_ptr(), workspace.numel(),
                                                _lib.dev(vertices, "vertices"), _lib.dev(normals, "normals"),
                                                _lib.dev(triangles, "triangles", torch.int32), cap_v, cap_t, _lib.stream()),
               "sn_rm_isosurface_emit")


def isosurface(volume: torch.Tensor, iso: float, origin=(0.0, 0.0, 0.0), step=(1.0, 1.0, 1.0), normals: bool = True) -> dict:
    """Marching tetrahedra: the surface f = iso of volume [nx,ny,nz] (fp32, on the device; inside is f > iso) as
    {"vertices" [V,3] f32 at origin + index * step, "normals" [V,3] f32 pointing out of the inside (None with normals=False),
    "triangles" [T,3] int32, counter-clockwise seen from outside}.  Watertight inside the lattice; open where the surface leaves it.

    The size of the result depends on the data: the count runs first (two launches), its two totals are read back ONCE -- the only host
    synchronisation, which also makes this call uncapturable as a graph -- the outputs are allocated exactly, and one launch fills them.
    Deterministic: vertex and triangle order are fixed by the definition, and two calls give equal bits."""
    vol = _f32(volume)
    counts, ws = isosurface_counts(vol, iso)
    nv, nt = _read_counts(counts)
    if nv > ISOSURFACE_MAX_VERTICES or nt > ISOSURFACE_MAX_VERTICES:
        raise RuntimeError(f"isosurface: {nv} vertices / {nt} triangles exceed the int32 indices of the result")
    out = _empty_mesh(nv, nt, vol.device, normals)
    if nv or nt:
        isosurface_emit(vol, iso, origin, step, ws, out["vertices"], out["normals"], out["triangles"])
    return out


# ---- clean-up: connected components, floater removal (mesh_clean.hip) -------------------------------------------------------------------
COMPONENT_ROUNDS_PER_CALL = 4          # rounds per sweep call = per host read of the round flags
COMPONENT_MAX_ROUNDS = 4096            # a terminator for a bug, not a tuning value: propagation alone needs at most V rounds, real meshes single digits


def _triangles_i32(triangles: torch.Tensor, n_vertices: int):
    if triangles.dim() != 2 or triangles.shape[1] != 3:
        raise RuntimeError(f"triangles must be [T,3], got {tuple(triangles.shape)}")
    V, T = int(n_vertices), triangles.shape[0]
    if V < 0 or V > ISOSURFACE_MAX_VERTICES or T > ISOSURFACE_MAX_VERTICES:
        raise RuntimeError(f"mesh of {V} vertices / {T} triangles: both counts must be in [0, 2^31)")
    return triangles.contiguous(), V, T


def mesh_components(triangles: torch.Tensor, n_vertices: int) -> dict:
    """Connected components of an indexed mesh: triangles [T,3] int32 on the device over n_vertices vertices (a row with an index outside
    [0, V) connects nothing and counts nowhere) -> {"labels" [V] int32, the smallest vertex index of each vertex's component;
    "triangle_counts", "vertex_counts" [V] int32, nonzero at the roots (labels[r] == r) only; "counts" int32 [2] on the device = {roots,
    roots with at least one triangle}; "rounds": the rounds it took, the confirming one included}.

    The labels are a unique fixed point, reached by rounds of hook + jump launches in which no workgroup waits on another; the rounds are
    issued 4 to a call, and the 4 round flags are read back after each call -- one small copy per batch, which also makes this call
    uncapturable as a graph -- until a round reports that it lowered no label.  Deterministic: two calls give equal bits."""
    tri, V, T = _triangles_i32(triangles, n_vertices)
    p_tri = _lib.dev(tri, "triangles", torch.int32)
    dev = tri.device
    out = {k: torch.empty(V, device=dev, dtype=torch.int32) for k in ("labels", "triangle_counts", "vertex_counts")}
    out["counts"] = torch.zeros(2, device=dev, dtype=torch.int32)
    out["rounds"] = 0
    if V == 0:
        return out
    L, st = _lib.lib(), _lib.stream()
    p_lab = out["labels"].data_ptr()
    _lib.check(L.sn_rm_mesh_components_init(V, p_lab, st), "sn_rm_mesh_components_init")
    changed = torch.empty(COMPONENT_ROUNDS_PER_CALL, device=dev, dtype=torch.int32)
    rounds = 0
    while True:
        if rounds >= COMPONENT_MAX_ROUNDS:
            raise RuntimeError("mesh_components did not converge")
        _lib.check(L.sn_rm_mesh_components_sweep(p_tri, T, V, p_lab, COMPONENT_ROUNDS_PER_CALL, changed.data_ptr(), st),
                   "sn_rm_mesh_components_sweep")
        flags = changed.tolist()
        if flags[-1] == 0:                     # (an unchanged round is followed by unchanged rounds only)
            rounds += next(i for i, f in enumerate(flags) if f == 0) + 1
            break
        rounds += COMPONENT_ROUNDS_PER_CALL
    _lib.check(L.sn_rm_mesh_component_stats(p_tri, T, V, p_lab, out["triangle_counts"].data_ptr(), out["vertex_counts"].data_ptr(),
                                            out["counts"].data_ptr(), st), "sn_rm_mesh_component_stats")
    out["rounds"] = rounds
    return out


def mesh_filter_counts(triangles: torch.Tensor, n_vertices: int, components: dict, min_triangles: int = 0, keep_largest: int = 0):
    """The first half of mesh_clean(): (counts, workspace) with counts = {V', T'} as an int32 [2] tensor on the device (nothing is read
    back) and the workspace that mesh_filter_emit() takes -- the module's one "mesh_clean" buffer per device: the next call on that device
    reuses it.  components: what mesh_components() returned for this mesh.  keep_largest = k > 0: the k-th largest key comes from one
    torch.topk over the int64 keys on the device (the keys are unique, so it is deterministic) and stays there."""
    tri, V, T = _triangles_i32(triangles, n_vertices)
    dev = tri.device
    counts = torch.zeros(2, device=dev, dtype=torch.int32)
    L = _lib.lib()
    ws = _workspace("mesh_clean", int(L.sn_rm_mesh_clean_workspace_bytes(V, T)), dev, empty_ok=V == 0)
    if V == 0:
        return counts, ws
    tc = components["triangle_counts"]
    if keep_largest > 0:
        keys = (tc.to(torch.int64) << 32) | (0xFFFFFFFF - torch.arange(V, device=dev, dtype=torch.int64))
        min_key = torch.topk(keys, min(int(keep_largest), V)).values[-1:].contiguous()
    else:
        min_key = torch.zeros(1, device=dev, dtype=torch.int64)
    _lib.check(L.sn_rm_mesh_filter_count(_lib.dev(tri, "triangles", torch.int32), T, V, _lib.dev(components["labels"], "labels", torch.int32),
                                         _lib.dev(tc, "triangle_counts", torch.int32), min(int(min_triangles), 0xFFFFFFFF), min_key.data_ptr(),
                                         ws.data_ptr(), ws.numel(), counts.data_ptr(), _lib.stream()), "sn_rm_mesh_filter_count")
    return counts, ws


def mesh_filter_emit(triangles: torch.Tensor, vertices: torch.Tensor, normals, workspace: torch.Tensor, out_vertices: torch.Tensor, out_normals,
                     out_triangles: torch.Tensor, source_vertex=None, cap_v: int | None = None, cap_t: int | None = None):
    """The second half: fills out_vertices [>= cap_v, 3] f32, out_normals (same shape; iff normals is given), out_triangles [>= cap_t, 3]
    int32 and source_vertex [>= cap_v] int32 (or None) from the workspace mesh_filter_counts() left.  Capacities below the counts truncate:
    the stored prefix is the full result's."""
    tri, V, T = _triangles_i32(triangles, vertices.shape[0])
    per_vertex = [out_vertices] + ([] if normals is None else [out_normals]) + ([] if source_vertex is None else [source_vertex])
    cap_v, cap_t = _capacities("mesh_filter_emit", cap_v, cap_t, per_vertex, out_triangles)
    _rows3("mesh_filter_emit", vertices, out_vertices, out_triangles, out_normals if normals is not None else None)
    if normals is not None and tuple(normals.shape) != tuple(vertices.shape):
        raise RuntimeError("mesh_filter_emit: vertices, normals and triangles are [n,3]")
    _lib.check(_lib.lib().sn_rm_mesh_filter_emit(_lib.dev(tri, "triangles", torch.int32), T, V, _lib.dev(vertices, "vertices"),
                                                 _lib.dev(normals, "normals"), workspace.data_ptr(), workspace.numel(),
                                                 _lib.dev(out_vertices, "out_vertices"), _lib.dev(out_normals if normals is not None else None, "out_normals"),
                                                 _lib.dev(out_triangles, "out_triangles", torch.int32),
                                                 _lib.dev(source_vertex, "source_vertex", torch.int32), cap_v, cap_t, _lib.stream()),
               "sn_rm_mesh_filter_emit")


def mesh_clean(mesh: dict, min_triangles: int = 0, keep_largest: int = 0, return_source: bool = False) -> dict:
    """The mesh without its small connected components -- the floaters of a density field, the label noise of a gated one.  mesh: the keys
    of isosurface() ("vertices" [V,3] f32, "normals" [V,3] f32 or None, "triangles" [T,3] int32; any indexed mesh on the device).  A component
    is kept iff it has at least max(min_triangles, 1) valid triangles and -- keep_largest = k > 0 -- is among the k with the most triangles
    (ties: the component with the lower smallest vertex index first).  Kept vertices and triangles keep their order; rows are copied bit for
    bit and indices remapped.  return_source: also "source_vertex" [V'] int32, the old index of each kept vertex, to carry other attributes
    across.  With both options 0 the input dict is returned as it is, with no launch.

    mesh_components() reads its round flags back, and the two totals {V', T'} are read back once to allocate the result exactly: this call
    cannot be captured as a graph.  Deterministic: two calls give equal bits."""
    min_triangles, keep_largest = int(min_triangles), int(keep_largest)
    if min_triangles < 0 or keep_largest < 0:
        raise ValueError(f"mesh_clean: min_triangles = {min_triangles} and keep_largest = {keep_largest} must not be negative")
    if min_triangles == 0 and keep_largest == 0:
        return mesh
    vertices, normals, triangles = _f32(mesh["vertices"]), mesh["normals"], mesh["triangles"]
    normals = None if normals is None else _f32(normals)
    V, dev = vertices.shape[0], vertices.device
    comp = mesh_components(triangles, V)
    counts, ws = mesh_filter_counts(triangles, V, comp, min_triangles, keep_largest)
    nv, nt = _read_counts(counts)
    out = _empty_mesh(nv, nt, dev, normals is not None)
    source = torch.empty(nv, device=dev, dtype=torch.int32) if return_source else None
    if nv or nt:
        mesh_filter_emit(triangles, vertices, normals, ws, out["vertices"], out["normals"], out["triangles"], source)
    if return_source:
        out["source_vertex"] = source
    return out


# ---- split by vertex label: one mesh per instance (mesh_split.hip) ------------------------------------------------------------------------
MESH_SPLIT_PARTS = 33                  # include/sanerf_hip.h: SN_MESH_SPLIT_PARTS -- instance ids 0 .. 31, and part 32 for every label >= 32
_CARRIED = ("colors", "coverage", "labels")    # per-vertex attributes of extract_mesh that a part takes along through source_vertex


def _vertex_labels_u8(labels, V, what):
    if not torch.is_tensor(labels) or labels.dtype != torch.uint8 or tuple(labels.shape) != (V,):
        got = (tuple(labels.shape), labels.dtype) if torch.is_tensor(labels) else type(labels).__name__
        raise RuntimeError(f"{what}: vertex_labels must be a uint8 tensor [{V}], one label per vertex, got {got}")
    return labels.contiguous()


def mesh_split_counts(triangles: torch.Tensor, n_vertices: int, vertex_labels: torch.Tensor):
    """The first half of mesh_split(): (offsets, counts, workspace) with offsets = {"part_triangle_offsets", "part_vertex_offsets"}, int32
    [34] each -- the first row of every part, the totals last -- and counts = {V', T'} as an int32 [2] tensor, all on the device (nothing
    is read back), and the workspace that mesh_split_emit() takes -- the module's one "mesh_split" buffer per device: the next call on
    that device reuses it.  vertex_labels: [n_vertices] uint8."""
    tri, V, T = _triangles_i32(triangles, n_vertices)
    dev = tri.device
    lab = _vertex_labels_u8(vertex_labels, V, "mesh_split_counts")
    p_tri, p_lab = _lib.dev(tri, "triangles", torch.int32), _lib.dev(lab, "vertex_labels", torch.uint8)
    offsets = {k: torch.zeros(MESH_SPLIT_PARTS + 1, device=dev, dtype=torch.int32) for k in ("part_triangle_offsets", "part_vertex_offsets")}
    counts = torch.zeros(2, device=dev, dtype=torch.int32)
    L = _lib.lib()
    ws = _workspace("mesh_split", int(L.sn_rm_mesh_split_workspace_bytes(V, T)), dev, empty_ok=not (V and T))
    if V and T:
        _lib.check(L.sn_rm_mesh_split_count(p_tri, T, V, p_lab, ws.data_ptr(), ws.numel(), offsets["part_triangle_offsets"].data_ptr(), offsets["part_vertex_offsets"].data_ptr(),
                                            counts.data_ptr(), _lib.stream()), "sn_rm_mesh_split_count")
    return offsets, counts, ws


def mesh_split_emit(triangles: torch.Tensor, vertices: torch.Tensor, normals, workspace: torch.Tensor, out_vertices: torch.Tensor, out_normals,
                    out_triangles: torch.Tensor, source_vertex=None, source_triangle=None, cap_v: int | None = None, cap_t: int | None = None):
    """The second half: fills out_vertices [>= cap_v, 3] f32, out_normals (same shape; iff normals is given), out_triangles [>= cap_t, 3]
    int32, source_vertex [>= cap_v] and source_triangle [>= cap_t] int32 (or None) from the workspace mesh_split_counts() left.  Capacities
    below the counts truncate: the stored prefix is the full result's."""
    tri, V, T = _triangles_i32(triangles, vertices.shape[0])
    per_vertex = [out_vertices] + ([] if normals is None else [out_normals]) + ([] if source_vertex is None else [source_vertex])
    cap_v, cap_t = _capacities("mesh_split_emit", cap_v, cap_t, per_vertex, out_triangles)
    if source_triangle is not None and source_triangle.shape[0] < cap_t:
        raise ValueError("mesh_split_emit: a capacity exceeds its buffer")
    _rows3("mesh_split_emit", vertices, out_vertices, out_triangles, out_normals if normals is not None else None)
    if normals is not None and tuple(normals.shape) != tuple(vertices.shape):
        raise RuntimeError("mesh_split_emit: vertices, normals and triangles are [n,3]")
    _lib.check(_lib.lib().sn_rm_mesh_split_emit(_lib.dev(tri, "triangles", torch.int32), T, V, _lib.dev(vertices, "vertices"),
                                                _lib.dev(normals, "normals"), workspace.data_ptr(), workspace.numel(),
                                                _lib.dev(out_vertices, "out_vertices"), _lib.dev(out_normals if normals is not None else None, "out_normals"),
                                                _lib.dev(out_triangles, "out_triangles", torch.int32),
                                                _lib.dev(source_vertex, "source_vertex", torch.int32),
                                                _lib.dev(source_triangle, "source_triangle", torch.int32), cap_v, cap_t, _lib.stream()),
               "sn_rm_mesh_split_emit")


def mesh_split(mesh: dict, labels=None, return_source: bool = False) -> dict:
    """A labelled mesh taken apart: one mesh per instance.  mesh: the keys of isosurface() ("vertices" [V,3] f32, "normals" [V,3] f32 or
    None, "triangles" [T,3] int32; any indexed mesh on the device); labels [V] uint8, default mesh["labels"] -- what
    extract_mesh(vertex_labels=True) and vertex_attributes(labels=True) give.  Part p < 32 is instance id p and part 32 collects every
    label >= 32 (255 = "none" among them).  A triangle goes, whole, to the part that two of its corners have (three different ones: the
    lowest); a vertex goes to every part that has a triangle of it, so a seam vertex is duplicated.  include/sanerf_hip.h has the
    definition; tests/mesh_split_ref.py restates it.

    Returns {"parts": {part id: mesh}, non-empty parts only, each a view of the packed arrays with "vertices", "normals", "triangles"
    (indices local to the part: a stand-alone mesh) and, where the input mesh has them, "colors", "coverage" and "labels" gathered through
    source_vertex; "vertices", "normals", "triangles": the packed arrays, parts contiguous and in part order; "part_triangle_offsets",
    "part_vertex_offsets": int32 [34] on the device; return_source: "source_vertex" [V'], "source_triangle" [T'] int32, the input index of
    every packed row}.  Triangles keep their input order inside a part and vertices their increasing index; rows are copied bit for bit.
    Not done: seams are not re-cut along the label boundary, parts are not closed (a part is an open shell where it met its neighbour), and
    attributes are gathered, not recomputed.

    The two totals {V', T'} are read back once to allocate the result exactly (as mesh_clean does) and the 2 x 34 offsets once to slice
    it: this call cannot be captured as a graph.  Deterministic: two calls give equal bits."""
    vertices, normals, triangles = _f32(mesh["vertices"]), mesh["normals"], mesh["triangles"]
    normals = None if normals is None else _f32(normals)
    _vertices_v3(vertices, "mesh_split")
    V, dev = vertices.shape[0], vertices.device
    if labels is None:
        labels = mesh.get("labels")
        if labels is None:
            raise ValueError("mesh_split: no labels given and the mesh has no 'labels' (extract_mesh(vertex_labels=True))")
    labels = _vertex_labels_u8(labels, V, "mesh_split")
    carried = {k: mesh[k] for k in _CARRIED if mesh.get(k) is not None}
    offsets, counts, ws = mesh_split_counts(triangles, V, labels)
    nv, nt = _read_counts(counts)
    if nv > ISOSURFACE_MAX_VERTICES:
        raise RuntimeError(f"mesh_split: {nv} vertices exceed the int32 indices of the result")
    out = _empty_mesh(nv, nt, dev, normals is not None)
    want_source_v = return_source or bool(carried)
    source_v = torch.empty(nv, device=dev, dtype=torch.int32) if want_source_v else None
    source_t = torch.empty(nt, device=dev, dtype=torch.int32) if return_source else None
    if nv or nt:
        mesh_split_emit(triangles, vertices, normals, ws, out["vertices"], out["normals"], out["triangles"], source_v, source_t)
    packed = {k: v[source_v.long()] for k, v in carried.items()}
    toff, voff = offsets["part_triangle_offsets"].tolist(), offsets["part_vertex_offsets"].tolist()
    parts = {}
    for p in range(MESH_SPLIT_PARTS):
        (t0, t1), (v0, v1) = toff[p:p + 2], voff[p:p + 2]
        if t1 > t0:
            part = {"vertices": out["vertices"][v0:v1], "normals": None if normals is None else out["normals"][v0:v1],
                    "triangles": out["triangles"][t0:t1]}
            part.update({k: v[v0:v1] for k, v in packed.items()})
            parts[p] = part
    out.update(offsets)
    out["parts"] = parts
    if return_source:
        out["source_vertex"], out["source_triangle"] = source_v, source_t
    return out


# ---- simplification: uniform vertex clustering (mesh_simplify.hip) ------------------------------------------------------------------------
def _cell_lattice(origin, cell, dims):
    origin, cell, dims = _triple(origin, "origin"), _triple(cell, "cell"), _triple(dims, "dims", int)
    cells = dims[0] * dims[1] * dims[2]
    if min(dims) < 1 or cells > ISOSURFACE_MAX_VERTICES:
        raise ValueError(f"mesh_simplify: dims = {dims}: every entry at least 1 and the product below 2^31")
    return _lib.host_f32(origin), _lib.host_f32(cell), _lib.host_i32(dims), cells


def _mesh_f32(vertices, normals):
    if vertices.dim() != 2 or vertices.shape[1] != 3 or (normals is not None and tuple(normals.shape) != tuple(vertices.shape)):
        raise RuntimeError("mesh_simplify: vertices and normals are [V,3]")
    return _lib.dev(vertices, "vertices"), _lib.dev(normals, "normals")


def mesh_simplify_counts(vertices: torch.Tensor, normals, triangles: torch.Tensor, origin, cell, dims):
    """The first half of mesh_simplify(): (counts, workspace) with counts = {V', T'} as an int32 [2] tensor on the device (nothing is read
    back) and the workspace that mesh_simplify_emit() takes -- the module's one "mesh_simplify" buffer per device: the next call on that
    device reuses it.  origin, cell: 3 floats each; dims: 3 ints, the cells per axis (a vertex outside them has no cell)."""
    tri, V, T = _triangles_i32(triangles, vertices.shape[0])
    p_v, p_n = _mesh_f32(vertices, normals)
    h_origin, h_cell, h_dims, cells = _cell_lattice(origin, cell, dims)
    dev = vertices.device
    counts = torch.zeros(2, device=dev, dtype=torch.int32)
    L = _lib.lib()
    ws = _workspace("mesh_simplify", int(L.sn_rm_mesh_simplify_workspace_bytes(V, T, cells)), dev)
    _lib.check(L.sn_rm_mesh_simplify_count(p_v, p_n, _lib.dev(tri, "triangles", torch.int32), V, T, h_origin, h_cell, h_dims, ws.data_ptr(),
                                           ws.numel(), counts.data_ptr(), _lib.stream()), "sn_rm_mesh_simplify_count")
    return counts, ws


def mesh_simplify_emit(vertices: torch.Tensor, normals, triangles: torch.Tensor, origin, cell, dims, workspace: torch.Tensor,
                       out_vertices: torch.Tensor, out_normals, out_triangles: torch.Tensor, vertex_cluster=None, cap_v: int | None = None,
                       cap_t: int | None = None):
    """The second half: fills out_vertices [>= cap_v, 3] f32, out_normals (same shape; iff normals is given), out_triangles [>= cap_t, 3]
    int32 and vertex_cluster [V] int32 (or None) from the workspace mesh_simplify_counts() left for the same mesh and lattice.  Capacities
    below the counts truncate: the stored prefix is the full result's."""
    tri, V, T = _triangles_i32(triangles, vertices.shape[0])
    p_v, p_n = _mesh_f32(vertices, normals)
    h_origin, h_cell, h_dims, _ = _cell_lattice(origin, cell, dims)
    cap_v, cap_t = _capacities("mesh_simplify_emit", cap_v, cap_t, [out_vertices] + ([] if normals is None else [out_normals]), out_triangles)
    if vertex_cluster is not None and vertex_cluster.shape[0] < V:
        raise ValueError("mesh_simplify_emit: a capacity exceeds its buffer")
    _rows3("mesh_simplify_emit", out_vertices, out_triangles, out_normals if normals is not None else None)
    _lib.check(_lib.lib().sn_rm_mesh_simplify_emit(p_v, p_n, _lib.dev(tri, "triangles", torch.int32), V, T, h_origin, h_cell, h_dims,
                                                   workspace.data_ptr(), workspace.numel(), _lib.dev(out_vertices, "out_vertices"),
                                                   _lib.dev(out_normals if normals is not None else None, "out_normals"),
                                                   _lib.dev(out_triangles, "out_triangles", torch.int32),
                                                   _lib.dev(vertex_cluster, "vertex_cluster", torch.int32), cap_v, cap_t, _lib.stream()),
               "sn_rm_mesh_simplify_emit")


def _covering_lattice(vertices: torch.Tensor, cell):
    """(origin, dims) of the cell lattice over the bounding box of the finite vertices, the lower corner pulled back by half a cell; None
    without a finite vertex.  One aminmax on the device, its six values read back."""
    import numpy as np
    finite = vertices[torch.isfinite(vertices).all(dim=1)]
    if finite.shape[0] == 0:
        return None
    lo, hi = torch.aminmax(finite, dim=0)
    box = torch.stack([lo, hi]).tolist()
    origin, dims = [], []
    for a in range(3):
        o = np.float32(np.float32(box[0][a]) - np.float32(0.5) * np.float32(cell[a]))
        if not np.isfinite(o):
            raise ValueError("mesh_simplify: the bounding box overflows fp32")
        origin.append(float(o))
        dims.append(int(np.floor((float(np.float32(box[1][a])) - float(o)) / float(np.float32(cell[a])))) + 2)    # one spare cell for the fp32 rounding of s
    return origin, dims


def mesh_simplify(mesh: dict, cell, origin=None, dims=None, return_cluster: bool = False) -> dict:
    """Uniform vertex clustering: the mesh with one vertex per occupied cell of a lattice of `cell`-sized boxes (a float or a triple) -- the
    triangle budget of a lattice-dense isosurface brought down on the device.  mesh: the keys of isosurface() ("vertices" [V,3] f32,
    "normals" [V,3] f32 or None, "triangles" [T,3] int32; any indexed mesh on the device); the result has the same keys.  A vertex moves
    to the mean of ALL input vertices of its cell (normals: the normalised sum); a triangle whose corners fall into fewer than three cells
    is dropped, and so is every triangle whose set of three cells an earlier triangle already has; the others keep their order and
    orientation, and only cells they touch become vertices, in cell-key order.  include/sanerf_hip.h has the definition, exact to the
    bit; tests/mesh_simplify_ref.py restates it.  return_cluster: also "vertex_cluster" [V] int32, the new index of each old vertex (-1:
    none), to carry other attributes across.

    origin, dims: the cell lattice (cell i covers origin + [i, i + 1) cell per axis); a vertex outside it has no cell and its triangles are
    dropped.  With both None the lattice covers the bounding box of the finite vertices, its lower corner pulled back by half a cell: one
    torch.aminmax on the device, read back.  Not promised: manifoldness, and no error metric is weighed -- this is not quadric decimation.

    The two totals {V', T'} are read back once to allocate the result exactly (as isosurface and mesh_clean do): this call cannot be
    captured as a graph.  Deterministic, and independent of the order of the input vertices: the sums are integers."""
    cell = _triple(cell, "cell") if hasattr(cell, "__len__") else [float(cell)] * 3
    if not all(c > 0.0 and c < float("inf") for c in cell):
        raise ValueError(f"mesh_simplify: cell = {cell} must be positive and finite")
    if (origin is None) != (dims is None):
        raise ValueError("mesh_simplify: give origin and dims together, or neither")
    vertices, normals, triangles = _f32(mesh["vertices"]), mesh["normals"], mesh["triangles"]
    normals = None if normals is None else _f32(normals)
    _triangles_i32(triangles, vertices.shape[0])
    _lib.dev(vertices, "vertices")
    V, dev = vertices.shape[0], vertices.device
    lattice = (origin, dims) if origin is not None else (_covering_lattice(vertices, cell) if V else None)
    nv = nt = 0
    if V and lattice is not None:
        origin, dims = lattice
        counts, ws = mesh_simplify_counts(vertices, normals, triangles, origin, cell, dims)
        nv, nt = _read_counts(counts)
    out = _empty_mesh(nv, nt, dev, normals is not None)
    cluster = torch.full((V,), -1, device=dev, dtype=torch.int32) if return_cluster else None
    if nv or nt:
        mesh_simplify_emit(vertices, normals, triangles, origin, cell, dims, ws, out["vertices"], out["normals"], out["triangles"], cluster)
    if return_cluster:
        out["vertex_cluster"] = cluster
    return out


# ---- smoothing in fixed point, geometric normals (mesh_smooth.hip) --------------------------------------------------------------------------
def smooth_quantisation(lo, hi):
    """(origin [3], quantum) that put the box lo .. hi inside the integer range [0, 2^22): with E the longest side of the box in fp64,
    quantum = fp32(E / 2^21) and origin_a = fp32(lo_a - 524288 quantum) (the product is exact, the difference one fp64 rounding).  The box
    then spans 2^19 .. 2^19 + 2^21 along its longest side: at least a quarter of its extent stays free on each side for the negative mu
    step.  None when E is 0, not finite, or too small for the quantum to be a positive fp32 number.  Host arithmetic only."""
    import numpy as np
    lo, hi = _triple(lo, "lo"), _triple(hi, "hi")
    E = max(hi[a] - lo[a] for a in range(3))
    with np.errstate(all="ignore"):
        quantum = np.float32(E / 2097152.0)
        origin = [np.float32(lo[a] - 524288.0 * float(quantum)) for a in range(3)]
    if not (E > 0.0 and np.isfinite(quantum) and quantum > 0 and all(np.isfinite(o) for o in origin)):
        return None
    return [float(o) for o in origin], float(quantum)


def _smooth_factors(lam, mu, what):
    """lambda and mu as the fp32 values the library receives, tested the way it tests them."""
    lam32, mu32 = (float(torch.tensor(float(x), dtype=torch.float32)) for x in (lam, mu))
    if not (0.0 < lam32 <= 1.0):
        raise ValueError(f"{what}: lambda = {lam} must be in (0, 1]")
    if not (mu32 == 0.0 or -1.0 <= mu32 < -lam32):
        raise ValueError(f"{what}: mu = {mu} must be 0 (plain Laplacian smoothing) or in [-1, -lambda)")
    return lam32, mu32


def _smooth_iterations(iterations, what):
    import operator
    try:
        n = -1 if isinstance(iterations, bool) else operator.index(iterations)
    except TypeError:
        n = -1
    if not 0 <= n < 1 << 32:
        raise ValueError(f"{what}: {iterations!r} iterations: a non-negative integer is needed")
    return n


def _smooth_quant_args(origin, quantum, what):
    origin, quantum = _triple(origin, "origin"), float(quantum)
    q32 = float(torch.tensor(quantum, dtype=torch.float32))
    if not (0.0 < q32 < float("inf")):
        raise ValueError(f"{what}: quantum = {quantum} must be positive and finite in fp32")
    if not all(abs(float(torch.tensor(o, dtype=torch.float32))) < float("inf") for o in origin):
        raise ValueError(f"{what}: origin = {origin} must be finite in fp32")
    return _lib.host_f32(origin), q32


def mesh_smooth_build(vertices: torch.Tensor, triangles: torch.Tensor, origin, quantum) -> torch.Tensor:
    """The first phase of mesh_smooth(): quantises vertices [V,3] f32 to Q = rint((p - origin) / quantum) and inverts triangles [T,3] int32
    into every vertex's row of (next, prev) pairs, with the open flags.  Returns the workspace that mesh_smooth_steps() and
    mesh_smooth_emit() take -- the module's one "mesh_smooth" buffer per device: the next build on that device reuses it.  Nothing is read
    back."""
    tri, V, T = _triangles_i32(triangles, vertices.shape[0])
    _vertices_v3(vertices, "mesh_smooth")
    p_v = _lib.dev(vertices, "vertices")
    h_origin, q32 = _smooth_quant_args(origin, quantum, "mesh_smooth_build")
    ws = _workspace("mesh_smooth", int(_lib.lib().sn_rm_mesh_smooth_workspace_bytes(V, T)), vertices.device)
    _lib.check(_lib.lib().sn_rm_mesh_smooth_build(p_v, _lib.dev(tri, "triangles", torch.int32), V, T, h_origin, q32, ws.data_ptr(), ws.numel(),
                                                  _lib.stream()), "sn_rm_mesh_smooth_build")
    return ws


def mesh_smooth_steps(n_vertices: int, n_triangles: int, workspace: torch.Tensor, iterations: int, lam: float = 0.5, mu: float = -0.53,
                      pin_open: bool = True):
    """The second phase: `iterations` iterations -- a half-step with lam, then (mu != 0) one with mu, one launch each -- on the integers
    mesh_smooth_build() left in the workspace for a mesh of these sizes.  Calls compose: 3 then 2 iterations equal 5."""
    iterations = _smooth_iterations(iterations, "mesh_smooth_steps")
    lam32, mu32 = _smooth_factors(lam, mu, "mesh_smooth_steps")
    _lib.check(_lib.lib().sn_rm_mesh_smooth_steps(int(n_vertices), int(n_triangles), iterations, lam32, mu32, int(bool(pin_open)),
                                                  workspace.data_ptr(), workspace.numel(), _lib.stream()), "sn_rm_mesh_smooth_steps")


def mesh_smooth_emit(vertices: torch.Tensor, n_triangles: int, origin, quantum, workspace: torch.Tensor, out_vertices: torch.Tensor,
                     out_normals=None, vertex_flags=None):
    """The third phase: fills out_vertices [V,3] f32, out_normals [V,3] f32 (or None) and vertex_flags [V] uint8 (or None; bit 0 placed,
    bit 1 open, bit 2 moved) from the workspace and the vertices, origin and quantum the build was given.  It leaves the workspace as it
    is: more steps may follow."""
    V = vertices.shape[0]
    if (tuple(out_vertices.shape) != (V, 3) or (out_normals is not None and tuple(out_normals.shape) != (V, 3))
            or (vertex_flags is not None and tuple(vertex_flags.shape) != (V,))):
        raise ValueError("mesh_smooth_emit: out_vertices and out_normals are [V,3], vertex_flags is [V]")
    h_origin, q32 = _smooth_quant_args(origin, quantum, "mesh_smooth_emit")
    _lib.check(_lib.lib().sn_rm_mesh_smooth_emit(_lib.dev(vertices, "vertices"), V, int(n_triangles), h_origin, q32, workspace.data_ptr(),
                                                 workspace.numel(), _lib.dev(out_vertices, "out_vertices"), _lib.dev(out_normals, "out_normals"),
                                                 _lib.dev(vertex_flags, "vertex_flags", torch.uint8), _lib.stream()), "sn_rm_mesh_smooth_emit")


def _bounding_quantisation(vertices: torch.Tensor):
    """smooth_quantisation of the bounding box of the finite vertices; None without one.  One aminmax on the device, its six values read back."""
    finite = vertices[torch.isfinite(vertices).all(dim=1)]
    if finite.shape[0] == 0:
        return None
    lo, hi = torch.aminmax(finite, dim=0)
    box = torch.stack([lo, hi]).tolist()
    return smooth_quantisation(box[0], box[1])


def mesh_smooth(mesh: dict, iterations: int = 10, lam: float = 0.5, mu: float = -0.53, pin_open: bool = True, origin=None, quantum=None,
                normals=None, return_flags: bool = False) -> dict:
    """Taubin smoothing (mu = 0: plain Laplacian smoothing) of an indexed triangle mesh with the uniform umbrella, in fixed point on the
    device, and the geometric normals of the result.  mesh: the keys of isosurface() ("vertices" [V,3] f32, "normals" [V,3] f32 or None,
    "triangles" [T,3] int32; any indexed mesh on the device).  The result has the same keys; "triangles" is the input tensor; "normals" are
    the area-weighted normals of the SMOOTHED triangles when `normals` is true (default: iff the input has normals; the input's values are
    not read), else None.  return_flags: also "vertex_flags" [V] uint8 -- bit 0 placed, bit 1 open, bit 2 moved.

    One iteration moves every vertex by lam times the difference to the mean of its neighbours, then by mu times the new difference
    (mu < -lam: the step that undoes the shrinkage).  Positions are integers Q = rint((p - origin) / quantum) in [0, 2^22) per axis, so
    every sum is exact: the result equals tests/mesh_smooth_ref.py bit for bit and depends on neither the order of the vertices nor the
    run; include/sanerf_hip.h has the definition.  Vertices on an open edge stay where they are with pin_open; a vertex that does not
    move keeps its input bits; a vertex outside the integer range, or with a non-finite coordinate, is left alone and ignored by its
    neighbours.

    origin (3 floats), quantum (one float): the quantisation; give both or neither.  With both given NOTHING is read back on the host --
    the sizes of the outputs are the input's.  With neither, smooth_quantisation of the bounding box of the finite vertices is used (the
    box well inside the range): one torch.aminmax, read back.  A mesh without a finite vertex or with a box of extent 0 is
    returned with its vertices unchanged and all normals zero.  Deterministic: two calls give equal bits."""
    iterations = _smooth_iterations(iterations, "mesh_smooth")
    _smooth_factors(lam, mu, "mesh_smooth")
    if (origin is None) != (quantum is None):
        raise ValueError("mesh_smooth: give origin and quantum together, or neither")
    if origin is not None:
        _smooth_quant_args(origin, quantum, "mesh_smooth")
    vertices, triangles = _f32(mesh["vertices"]), mesh["triangles"]
    _, V, T = _triangles_i32(triangles, vertices.shape[0])
    _vertices_v3(vertices, "mesh_smooth")
    _lib.dev(vertices, "vertices")
    want_normals = (mesh.get("normals") is not None) if normals is None else bool(normals)
    dev = vertices.device
    quant = (origin, quantum) if origin is not None else (_bounding_quantisation(vertices) if V else None)
    out = dict(mesh)
    if quant is None or V == 0:
        out["vertices"] = vertices.clone()
        out["normals"] = torch.zeros(V, 3, device=dev, dtype=torch.float32) if want_normals else None
        if return_flags:
            out["vertex_flags"] = torch.zeros(V, device=dev, dtype=torch.uint8)
        return out
    origin, quantum = quant
    ws = mesh_smooth_build(vertices, triangles, origin, quantum)
    if iterations:
        mesh_smooth_steps(V, T, ws, iterations, lam, mu, pin_open)
    out["vertices"] = torch.empty(V, 3, device=dev, dtype=torch.float32)
    out["normals"] = torch.empty(V, 3, device=dev, dtype=torch.float32) if want_normals else None
    flags = torch.empty(V, device=dev, dtype=torch.uint8) if return_flags else None
    mesh_smooth_emit(vertices, T, origin, quantum, ws, out["vertices"], out["normals"], flags)
    if return_flags:
        out["vertex_flags"] = flags
    return out


def mesh_vertex_normals(mesh: dict, origin=None, quantum=None) -> torch.Tensor:
    """[V,3] f32: the area-weighted normals of the mesh's own triangles at its vertices -- mesh_smooth's geometric normals with no step
    taken (build + emit), on positions quantised as mesh_smooth quantises them.  (0,0,0) at a vertex without a valid triangle.  origin,
    quantum: as for mesh_smooth."""
    return mesh_smooth(mesh, iterations=0, origin=origin, quantum=quantum, normals=True)["normals"]


# ---- the rasteriser: a mesh seen from one pinhole camera (mesh_raster.hip) -------------------------------------------------------------------
RASTER_MAX_SIDE = 8192                 # H, W
RASTER_SMALL_MAX_PIXELS = 16           # pixel centres in a triangle's clipped bounding box up to which its own lane scans it (the sweep in profiles/mesh_raster_bench.txt)
RASTER_SMALL_MAX_LIMIT = (1 << 31) - 1


def _raster_sizes(V, T, H, W, what):
    import operator
    try:
        H, W = operator.index(H), operator.index(W)
    except TypeError:
        raise ValueError(f"{what}: H and W must be integers") from None
    if not (1 <= H <= RASTER_MAX_SIDE and 1 <= W <= RASTER_MAX_SIDE):
        raise ValueError(f"{what}: H = {H}, W = {W} must be in [1, {RASTER_MAX_SIDE}]")
    return int(V), int(T), H, W


def _raster_camera(pose, intrinsics, device, what):
    """pose [4,4] and intrinsics [4] as contiguous fp32 tensors on the device.  A tensor that already is one is passed as it is, so that a
    captured graph sees what is written into it later."""
    def one(x, n, shape, name):
        t = x if torch.is_tensor(x) else torch.as_tensor(x, dtype=torch.float32)
        if t.numel() != n:
            raise ValueError(f"{what}: {name} must have {n} entries ({shape}), got {tuple(t.shape)}")
        if not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()):
            t = t.to(device=device, dtype=torch.float32).contiguous()
        return t
    return one(pose, 16, "[4,4]", "pose"), one(intrinsics, 4, "[4]", "intrinsics")


def _raster_near(near, what):
    near32 = float(torch.tensor(float(near), dtype=torch.float32))
    if not (0.0 < near32 < float("inf")):
        raise ValueError(f"{what}: near = {near} must be positive and finite in fp32")
    return near32


def mesh_raster_project(vertices: torch.Tensor, n_triangles: int, pose: torch.Tensor, intrinsics: torch.Tensor, H: int, W: int, near: float,
                        counts: torch.Tensor) -> torch.Tensor:
    """The first phase of mesh_rasterize(): every vertex of vertices [V,3] f32 into the camera (pose [4,4], intrinsics [4] = fx, fy, cx, cy:
    fp32 tensors ON THE DEVICE, read when the kernel runs) as a row {X, Y, 1/z, placed} of the workspace; clears the H x W depth buffer,
    the queue and counts (int32 [4]).  Returns the workspace that mesh_raster_draw() and mesh_raster_resolve() take -- the module's one
    "mesh_raster" buffer per device: the next projection on that device reuses it.  Nothing is read back."""
    _vertices_v3(vertices, "mesh_raster")
    V, T, H, W = _raster_sizes(vertices.shape[0], n_triangles, H, W, "mesh_raster_project")
    if tuple(counts.shape) != (4,) or pose.numel() != 16 or intrinsics.numel() != 4:
        raise ValueError("mesh_raster_project: pose is [4,4], intrinsics [4], counts int32 [4]")
    near32 = _raster_near(near, "mesh_raster_project")
    p_v = _lib.dev(vertices, "vertices")
    ws = _workspace("mesh_raster", int(_lib.lib().sn_rm_mesh_raster_workspace_bytes(V, T, H, W)), vertices.device)
    _lib.check(_lib.lib().sn_rm_mesh_raster_project(p_v, V, T, _lib.dev(pose, "pose"), _lib.dev(intrinsics, "intrinsics"), H, W, near32,
                                                    ws.data_ptr(), ws.numel(), _lib.dev(counts, "counts", torch.int32), _lib.stream()),
               "sn_rm_mesh_raster_project")
    return ws


def _raster_clip_args(what, V, vertices, pose, intrinsics, near):
    """What the clipped kernels read beside the rows -- the projection's own vertices [V,3], pose, intrinsics and near -- as the pointers and
    the fp32 value the library takes."""
    if vertices is None or pose is None or intrinsics is None or near is None:
        raise ValueError(f"{what}: clip=True needs the projection's vertices, pose, intrinsics and near")
    _vertices_v3(vertices, what)
    if vertices.shape[0] != V or pose.numel() != 16 or intrinsics.numel() != 4:
        raise ValueError(f"{what}: vertices are [{V},3], pose is [4,4], intrinsics [4]")
    near32 = _raster_near(near, what)
    return _lib.dev(vertices, "vertices"), _lib.dev(pose, "pose"), _lib.dev(intrinsics, "intrinsics"), near32


def mesh_raster_draw(triangles: torch.Tensor, n_vertices: int, H: int, W: int, workspace: torch.Tensor, counts: torch.Tensor, cull: bool = False,
                     small_max_pixels: int | None = None, clip: bool = False, vertices=None, pose=None, intrinsics=None, near=None,
                     clip_counts=None):
    """The second phase: the depth test of triangles [T,3] int32 against the rows mesh_raster_project() left, two launches.  A triangle whose
    clipped bounding box holds at most small_max_pixels pixel centres (default RASTER_SMALL_MAX_PIXELS) is scanned by its own lane, the
    others by a wave each from a queue on the device; the value changes the time only, never the result.  counts (int32 [4]) gains the
    drawn, the dropped, the degenerate and the culled.

    clip=True cuts the triangles that cross the near plane instead of dropping them (sn_rm_mesh_raster_draw_clip): it needs the
    projection's vertices, pose, intrinsics (device tensors, read when the kernels run) and near, and clip_counts (int32 [2]), which it
    clears and fills with the clipped triangles and their drawn pieces."""
    tri, V, T = _triangles_i32(triangles, n_vertices)
    V, T, H, W = _raster_sizes(V, T, H, W, "mesh_raster_draw")
    small = RASTER_SMALL_MAX_PIXELS if small_max_pixels is None else int(small_max_pixels)
    if not 0 <= small <= RASTER_SMALL_MAX_LIMIT:
        raise ValueError(f"mesh_raster_draw: small_max_pixels = {small_max_pixels} must be in [0, 2^31)")
    if tuple(counts.shape) != (4,):
        raise ValueError("mesh_raster_draw: counts is int32 [4]")
    if clip:
        if clip_counts is None or tuple(clip_counts.shape) != (2,):
            raise ValueError("mesh_raster_draw: clip=True needs clip_counts, int32 [2]")
        p_v, p_pose, p_intr, near32 = _raster_clip_args("mesh_raster_draw", V, vertices, pose, intrinsics, near)
        _lib.check(_lib.lib().sn_rm_mesh_raster_draw_clip(p_v, _lib.dev(tri, "triangles", torch.int32), V, T, p_pose, p_intr, H, W, near32,
                                                          int(bool(cull)), small, workspace.data_ptr(), workspace.numel(),
                                                          _lib.dev(counts, "counts", torch.int32), _lib.dev(clip_counts, "clip_counts", torch.int32),
                                                          _lib.stream()), "sn_rm_mesh_raster_draw_clip")
        return
    _lib.check(_lib.lib().sn_rm_mesh_raster_draw(_lib.dev(tri, "triangles", torch.int32), V, T, H, W, int(bool(cull)), small, workspace.data_ptr(),
                                                 workspace.numel(), _lib.dev(counts, "counts", torch.int32), _lib.stream()), "sn_rm_mesh_raster_draw")


def mesh_raster_resolve(triangles: torch.Tensor, n_vertices: int, H: int, W: int, workspace: torch.Tensor, triangle_id: torch.Tensor,
                        depth: torch.Tensor, mask: torch.Tensor, colors=None, image=None, normals=None, normal=None, labels=None, label=None,
                        bg_color: float = 1.0, clip: bool = False, vertices=None, pose=None, intrinsics=None, near=None):
    """The third phase: one lane per pixel turns the depth buffer into triangle_id [H,W] int32 (-1 where empty), depth [H,W] f32 (0) and
    mask [H,W] uint8, and interpolates the attributes that are given, perspective-correct in fp64: colors [V,3] f32 -> image [H,W,3] f32
    (bg_color where empty), normals [V,3] f32 -> normal [H,W,3] (not renormalised; 0), labels [V] uint8 -> label [H,W] uint8 (the corner
    with the largest weight; 255).  An attribute and its image come together.

    clip=True after a draw with clip=True (sn_rm_mesh_raster_resolve_clip): a winner that the near plane cut is rebuilt from the
    projection's vertices, pose, intrinsics and near, which it needs, and its attributes go through the triangle's own corners."""
    tri, V, T = _triangles_i32(triangles, n_vertices)
    V, T, H, W = _raster_sizes(V, T, H, W, "mesh_raster_resolve")
    if any(tuple(x.shape) != (H, W) for x in (triangle_id, depth, mask)):
        raise ValueError("mesh_raster_resolve: triangle_id, depth and mask are [H,W]")
    for a, o, name, a_shape, o_shape in ((colors, image, "colors / image", (V, 3), (H, W, 3)), (normals, normal, "normals / normal", (V, 3), (H, W, 3)),
                                         (labels, label, "labels / label", (V,), (H, W))):
        if (a is None) != (o is None):
            raise ValueError(f"mesh_raster_resolve: {name} come together")
        if a is not None and (tuple(a.shape) != a_shape or tuple(o.shape) != o_shape):
            raise ValueError(f"mesh_raster_resolve: {name} must be {list(a_shape)} and {list(o_shape)}")
    camera = _raster_clip_args("mesh_raster_resolve", V, vertices, pose, intrinsics, near) if clip else None
    outputs = (workspace.data_ptr(), workspace.numel(), _lib.dev(triangle_id, "triangle_id", torch.int32), _lib.dev(depth, "depth"),
               _lib.dev(mask, "mask", torch.uint8), _lib.dev(image, "image"), _lib.dev(normal, "normal"), _lib.dev(label, "label", torch.uint8),
               _lib.stream())
    attributes = (_lib.dev(colors, "colors"), _lib.dev(normals, "normals"), _lib.dev(labels, "labels", torch.uint8), float(bg_color))
    if clip:
        p_v, p_pose, p_intr, near32 = camera
        _lib.check(_lib.lib().sn_rm_mesh_raster_resolve_clip(p_v, _lib.dev(tri, "triangles", torch.int32), V, T, p_pose, p_intr, H, W, near32,
                                                             *attributes, *outputs), "sn_rm_mesh_raster_resolve_clip")
        return
    _lib.check(_lib.lib().sn_rm_mesh_raster_resolve(_lib.dev(tri, "triangles", torch.int32), V, T, H, W, *attributes, *outputs),
               "sn_rm_mesh_raster_resolve")


def mesh_rasterize(mesh: dict, pose, intrinsics, H: int, W: int, near: float = 0.05, cull: bool = False, colors=None, labels=None, normals=None,
                   bg_color: float = 1.0, small_max_pixels: int | None = None) -> dict:
    """The mesh seen from one pinhole camera, with a depth buffer, exact to the bit: {"triangle_id" [H,W] int32 (-1 where empty), "depth" [H,W]
    f32 (the camera-space -z of the surface, the field render's `depth` for get_rays' unnormalised directions; 0 where empty), "mask" [H,W]
    uint8, "counts" int32 [4] = triangles drawn / dropped (a corner that is not placed, or a bad index) / degenerate / culled} and, with the
    attribute, "image" [H,W,3] f32 from colors [V,3], "label" [H,W] uint8 from labels [V] uint8, "normal" [H,W,3] f32 from normals [V,3].

    mesh: "vertices" [V,3] f32 and "triangles" [T,3] int32 on the device -- what isosurface() and NeRFRenderer.extract_mesh() return;
    colors and labels default to the dict's own "colors" / "labels" where it has them; normals are taken only when given.  pose [4,4]
    (cam2world) and intrinsics [4] = (fx, fy, cx, cy) in get_rays' convention: the pixel (i, j) has its centre at (i + 0.5, j + 0.5), the
    camera looks along -z, y up.  Given as contiguous fp32 device tensors they are read by the kernels when they run: a captured graph
    replays with whatever camera they hold then.  Anything else is copied to the device first.

    A vertex nearer than `near`, outside the guard band of 2^14 pixels around the origin of the pixel grid, or not finite is not placed, and
    a triangle with such a corner is dropped whole: there is no clipping.  cull drops the faces whose outside (counter-clockwise, as
    isosurface() orients them) looks away.  One sample per pixel at its centre, the top-left rule on shared edges, nearest surface wins,
    the lower triangle index at equal depth bits: the result depends on neither the order of the triangles nor the run, and equals
    tests/mesh_raster_ref.py bit for bit; include/sanerf_hip.h has the definition.  Four launches, nothing is read back.

    mesh_rasterize_clip() is the same call with the near plane cutting the triangles that cross it."""
    return _rasterize("mesh_rasterize", False, mesh, pose, intrinsics, H, W, near, cull, colors, labels, normals, bg_color, small_max_pixels)


def mesh_rasterize_clip(mesh: dict, pose, intrinsics, H: int, W: int, near: float = 0.05, cull: bool = False, colors=None, labels=None, normals=None,
                        bg_color: float = 1.0, small_max_pixels: int | None = None) -> dict:
    """mesh_rasterize() with near-plane clipping, for a camera inside the mesh: a triangle with one or two corners behind the plane z = near
    (nearer than it, or behind the camera) is cut there instead of being dropped, so a floor or a wall that passes the camera ends in a
    clean edge, as the field's render of that camera does.  Same arguments, same outputs, and "clip_counts" int32 [2] = the clipped
    triangles and the pieces of them that were drawn ("counts" counts a clipped triangle once).  A triangle without a corner behind the
    plane gives the bits mesh_rasterize() gives.

    Only the near plane clips: a corner outside the guard band or not finite still drops its triangle, and so does a crossing point that
    leaves the guard band.  The crossing points are fp64 functions of the two vertices alone, so two triangles that share a cut edge share
    its end; the result equals tests/mesh_raster_clip_ref.py bit for bit, whatever the order of the triangles or the run.  Four launches
    and a 8-byte clear, nothing is read back; capturable as mesh_rasterize() is."""
    return _rasterize("mesh_rasterize_clip", True, mesh, pose, intrinsics, H, W, near, cull, colors, labels, normals, bg_color, small_max_pixels)


def _rasterize(what, clip, mesh, pose, intrinsics, H, W, near, cull, colors, labels, normals, bg_color, small_max_pixels):
    vertices, triangles = _f32(mesh["vertices"]), mesh["triangles"]
    _vertices_v3(vertices, what)
    tri, V, T = _triangles_i32(triangles, vertices.shape[0])
    V, T, H, W = _raster_sizes(V, T, H, W, what)
    near = _raster_near(near, what)
    bg = float(bg_color)
    if small_max_pixels is not None and not 0 <= int(small_max_pixels) <= RASTER_SMALL_MAX_LIMIT:
        raise ValueError(f"{what}: small_max_pixels = {small_max_pixels} must be in [0, 2^31)")
    _lib.dev(vertices, "vertices")
    dev = vertices.device
    colors = mesh.get("colors") if colors is None else colors
    labels = mesh.get("labels") if labels is None else labels
    colors = None if colors is None else _f32(colors)
    normals = None if normals is None else _f32(normals)
    for a, name, shape in ((colors, "colors", (V, 3)), (normals, "normals", (V, 3)), (labels, "labels", (V,))):
        if a is not None and tuple(a.shape) != shape:
            raise ValueError(f"{what}: {name} must be {list(shape)}, got {tuple(a.shape)}")
    if labels is not None and labels.dtype != torch.uint8:
        raise ValueError(f"{what}: labels must be uint8, got {labels.dtype}")
    pose, intrinsics = _raster_camera(pose, intrinsics, dev, what)
    out = {"triangle_id": torch.empty(H, W, device=dev, dtype=torch.int32), "depth": torch.empty(H, W, device=dev, dtype=torch.float32),
           "mask": torch.empty(H, W, device=dev, dtype=torch.uint8), "counts": torch.empty(4, device=dev, dtype=torch.int32)}
    if colors is not None:
        out["image"] = torch.empty(H, W, 3, device=dev, dtype=torch.float32)
    if normals is not None:
        out["normal"] = torch.empty(H, W, 3, device=dev, dtype=torch.float32)
    if labels is not None:
        out["label"] = torch.empty(H, W, device=dev, dtype=torch.uint8)
    camera = dict(clip=True, vertices=vertices, pose=pose, intrinsics=intrinsics, near=near) if clip else {}
    if clip:
        out["clip_counts"] = torch.empty(2, device=dev, dtype=torch.int32)
    ws = mesh_raster_project(vertices, T, pose, intrinsics, H, W, near, out["counts"])
    mesh_raster_draw(tri, V, H, W, ws, out["counts"], cull, small_max_pixels, clip_counts=out.get("clip_counts"), **camera)
    mesh_raster_resolve(tri, V, H, W, ws, out["triangle_id"], out["depth"], out["mask"], colors, out.get("image"), normals, out.get("normal"),
                        labels.contiguous() if labels is not None else None, out.get("label"), bg, **camera)
    return out


# ---- vertex attributes: surface probes (mesh_attr.hip) -------------------------------------------------------------------------------------
PROBE_SAMPLES = (4, 8, 16, 32)         # K of a vertex probe: what the label kernel takes as samples per row
PROBE_GEO = 15                         # geometry channels per sample (network.py:94)


def _probe_args(K, h, what):
    K, h = int(K), float(h)
    if K not in PROBE_SAMPLES:
        raise ValueError(f"{what}: samples = {K} must be one of {PROBE_SAMPLES}")
    if not (0.0 < h < float("inf")) or not (0.0 < float(torch.tensor(h, dtype=torch.float32)) < float("inf")):
        raise ValueError(f"{what}: the probe step h = {h} must be positive and finite in fp32")
    return K, h


def vertex_probe_points(vertices: torch.Tensor, normals: torch.Tensor, samples: int, h: float, first: int = 0, count: int | None = None,
                        contract: bool = False):
    """(xyz [count,K,3], dirs [count,3]) of the surface probes of the vertices first .. first + count - 1 (default: to the end) of a mesh:
    d = -n / |n| ((0, 0, -1) for a zero or non-finite normal), p_i = v + (i + 1/2 - K/2) h d, product and sum rounded separately, then --
    contract=True -- through raymarching.contract's arithmetic.  K = samples in {4, 8, 16, 32}; h > 0."""
    K, h = _probe_args(samples, h, "vertex_probe_points")
    if normals is None:
        raise ValueError("vertex_probe_points: the probes need the mesh normals")
    if vertices.dim() != 2 or vertices.shape[1] != 3 or tuple(normals.shape) != tuple(vertices.shape):
        raise RuntimeError(f"vertex_probe_points: vertices and normals are [V,3], got {tuple(vertices.shape)} and {tuple(normals.shape)}")
    V = vertices.shape[0]
    count = V - first if count is None else int(count)
    first = int(first)
    if first < 0 or count < 0 or first + count > V:
        raise ValueError(f"vertex_probe_points: vertices {first} .. {first + count - 1} outside the mesh of {V}")
    if V > ISOSURFACE_MAX_VERTICES or count * K >= 1 << 32:
        raise ValueError(f"vertex_probe_points: {V} vertices / {count} x {K} samples exceed one call")
    v, n = _f32(vertices), _f32(normals)
    xyz = torch.empty(count, K, 3, device=v.device, dtype=torch.float32)
    dirs = torch.empty(count, 3, device=v.device, dtype=torch.float32)
    _lib.check(_lib.lib().sn_rm_vertex_probe_points(_lib.dev(v, "vertices"), _lib.dev(n, "normals"), V, first, count, K, h, int(bool(contract)),
                                                    _lib.dev(xyz, "xyz"), _lib.dev(dirs, "dirs"), _lib.stream()), "sn_rm_vertex_probe_points")
    return xyz, dirs


def vertex_probe_composite(sigmas: torch.Tensor, geo_feat: torch.Tensor, dirs: torch.Tensor, h: float, labels=None, keep_mask: int = 0xFFFFFFFF,
                           invert: bool = False, want_labels: bool = False):
    """One launch: sigmas [V,K], geo_feat [V,K,15], dirs [V,3], labels [V,K] uint8 or None -> (f [V,31], coverage [V], vertex_label [V] uint8
    or None).  gate = (label in keep_mask) xor invert (true without labels); y = gate ? h sigma : 0; w = (1 - exp(-y)) exp(-sum of the y in
    front), NaN -> 0; coverage = sum w; f = [sum w geo / coverage | SH4(d / |d|)], with the plain mean of the K geo rows where the coverage is
    below 2^-126.  want_labels (needs labels): the vertex label is the lowest id with the largest sum of w over its samples, 255 where no
    vote is positive.  include/sanerf_hip.h states the definition, tests/mesh_attr_ref64.py its fp64 twin.  No autograd."""
    if sigmas.dim() != 2:
        raise RuntimeError(f"vertex_probe_composite: sigmas must be [V,K], got {tuple(sigmas.shape)}")
    V, K = sigmas.shape
    K, h = _probe_args(K, h, "vertex_probe_composite")
    if tuple(geo_feat.shape) != (V, K, PROBE_GEO) or tuple(dirs.shape) != (V, 3):
        raise RuntimeError(f"vertex_probe_composite: geo_feat {tuple(geo_feat.shape)} / dirs {tuple(dirs.shape)} do not match sigmas [{V},{K}] "
                           f"(geo_feat has {PROBE_GEO} channels)")
    if labels is not None and (labels.dtype != torch.uint8 or tuple(labels.shape) != (V, K)):
        raise RuntimeError(f"vertex_probe_composite: labels must be uint8 [{V},{K}], got {labels.dtype} {tuple(labels.shape)}")
    if want_labels and labels is None:
        raise ValueError("vertex_probe_composite: vertex labels need the per-sample labels")
    if not 0 <= int(keep_mask) < (1 << 32):
        raise ValueError("vertex_probe_composite: keep_mask is a 32-bit mask")
    if V * 16 >= 1 << 32:
        raise ValueError(f"vertex_probe_composite: at most 2^28 - 1 vertices per call (got {V})")
    sg, gf, dr = _f32(sigmas), _f32(geo_feat), _f32(dirs)
    if gf.data_ptr() % 16:
        gf = gf.clone()                    # (a view at an odd offset: the kernel reads 16-byte pieces)
    lb = None if labels is None else labels.detach().contiguous()
    dev = sg.device
    f = torch.empty(V, 16 + PROBE_GEO, device=dev, dtype=torch.float32)
    coverage = torch.empty(V, device=dev, dtype=torch.float32)
    vlabel = torch.empty(V, device=dev, dtype=torch.uint8) if want_labels else None
    _lib.check(_lib.lib().sn_rm_vertex_probe_composite(_lib.dev(lb, "labels", torch.uint8), _lib.dev(sg, "sigmas"), _lib.dev(gf, "geo_feat"),
                                                       _lib.dev(dr, "dirs"), V, K, h, int(keep_mask), int(bool(invert)), _lib.dev(f, "f"),
                                                       _lib.dev(coverage, "coverage"), _lib.dev(vlabel, "vertex_label", torch.uint8),
                                                       _lib.stream()), "sn_rm_vertex_probe_composite")
    return f, coverage, vlabel
