"""Geometry export (mesh.hip): lattice positions and marching tetrahedra on a density lattice.

    lattice_points     positions of a window of the vertices of an nx x ny x nz lattice, optionally contracted -- no meshgrid per chunk
    isosurface         volume [nx,ny,nz], iso -> {"vertices" [V,3], "normals" [V,3] or None, "triangles" [T,3] int32}
include/sanerf_hip.h states the definition (inside test, edge slots, Kuhn tetrahedra, orientation from the table, both orders, normals);
tests/mesh_ref.py restates it in numpy, operation for operation."""
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
    need = int(L.sn_rm_isosurface_workspace_bytes(nx, ny, nz))
    if need == 0:
        raise RuntimeError("isosurface: " + L.sn_last_error().decode())
    ws = _buffers.scratch("isosurface", vol.device, need)
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
    cap_v = vertices.shape[0] if cap_v is None else int(cap_v)
    cap_t = triangles.shape[0] if cap_t is None else int(cap_t)
    if cap_v > vertices.shape[0] or cap_t > triangles.shape[0] or (normals is not None and normals.shape[0] < cap_v):
        raise ValueError("isosurface_emit: a capacity exceeds its buffer")
    if vertices.dim() != 2 or vertices.shape[1] != 3 or triangles.dim() != 2 or triangles.shape[1] != 3 or (normals is not None and tuple(normals.shape[1:]) != (3,)):
        raise RuntimeError("isosurface_emit: vertices, normals and triangles are [n,3]")
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
    nv, nt = (int(c) & 0xFFFFFFFF for c in counts.tolist())
    if nv > ISOSURFACE_MAX_VERTICES or nt > ISOSURFACE_MAX_VERTICES:
        raise RuntimeError(f"isosurface: {nv} vertices / {nt} triangles exceed the int32 indices of the result")
    dev = vol.device
    vertices = torch.empty(nv, 3, device=dev, dtype=torch.float32)
    nrm = torch.empty(nv, 3, device=dev, dtype=torch.float32) if normals else None
    triangles = torch.empty(nt, 3, device=dev, dtype=torch.int32)
    if nv or nt:
        isosurface_emit(vol, iso, origin, step, ws, vertices, nrm, triangles)
    return {"vertices": vertices, "normals": nrm, "triangles": triangles}
