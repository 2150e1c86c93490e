"""Midpoint subdivision of a triangle mesh in numpy: what MeshFeatureField.subdivide_mesh (tools/map.py:800-808) gets from
trimesh.remesh.subdivide, which is not required here.  No device, no library: importable on its own."""
import numpy as np


def subdivide_midpoint(vertices, faces):
    """One round of 1-to-4 midpoint subdivision: -> (vertices' [V + E, 3] float64, faces' [4 F, 3] int64).
    One new vertex per unique (undirected) edge, appended behind the originals in the lexicographic order of the edges' sorted end points; the
    midpoints are computed in float64.  The four children of face (a, b, c) with midpoints ab, bc, ca stand at 4 f .. 4 f + 3 in trimesh's order:
    (a, ab, ca), (ab, b, bc), (ca, bc, c), (ab, bc, ca) -- every child keeps its parent's orientation.  Which number a new vertex gets is not
    observable in anything interpolated over the mesh."""
    v = np.asarray(vertices, dtype=np.float64)
    f = np.asarray(faces).astype(np.int64)
    if v.ndim != 2 or v.shape[1] != 3 or f.ndim != 2 or f.shape[1] != 3:
        raise ValueError(f"subdivide_midpoint: vertices are [V, 3] and faces [F, 3], but got {tuple(v.shape)} and {tuple(f.shape)}")
    if f.size and (f.min() < 0 or f.max() >= len(v)):
        raise ValueError(f"subdivide_midpoint: every face indexes into the {len(v)} vertices")
    edges = np.sort(f[:, [0, 1, 1, 2, 2, 0]].reshape(-1, 2), axis=1)  # (a,b), (b,c), (c,a) per face
    unique, inverse = np.unique(edges, axis=0, return_inverse=True)
    mid = (v[unique[:, 0]] + v[unique[:, 1]]) * 0.5
    m = inverse.reshape(-1, 3) + len(v)
    ab, bc, ca = m[:, 0], m[:, 1], m[:, 2]
    fine = np.stack([f[:, 0], ab, ca, ab, f[:, 1], bc, ca, bc, f[:, 2], ab, bc, ca], axis=1).reshape(-1, 3)
    return np.concatenate([v, mid], axis=0), fine


def subdivide_until(vertices, faces, min_vnum):
    """subdivide_midpoint until the mesh has at least min_vnum vertices (tools/map.py:804-806; a mesh that has them already comes back as it is,
    as float64 / int64)."""
    v, f = np.asarray(vertices, dtype=np.float64), np.asarray(faces).astype(np.int64)
    if len(f) == 0 and len(v) < min_vnum:
        raise ValueError("subdivide_until: a mesh without faces never grows")
    while len(v) < min_vnum:
        v, f = subdivide_midpoint(v, f)
    return v, f
