"""The start of the texture pipeline: feature patches sampled from the trained curved field -- NeRFNetwork.export_field ->
MeshFeatureField.sample_patches (tools/map.py:951-1128), the non-trimesh path (use_trimesh_raycast=False, cast_on_mfs=True).

  host helpers (numpy float64, the reference's own lines op for op)
    patch_grid_gap        :966-969   mean unique-edge length times pattern_rate
    principal_direction   :973-981   sklearn's PCA(3).fit(v).components_[0] without sklearn
    patch_calibration     :985       the S pixel coordinates of a patch side
    patch_frames          :1030-1038 T[:3,:4] per candidate: x, y, z axis and centre
  export_field            the batched form: per chunk of candidates ONE front call (nerftex_patch_front: rays, trace, scan distance, verdicts,
                          ordered acceptance) and ONE read-back, then the projector and the hash encoders over the accepted patches' hits
  _export_field_reference the staged form: the reference's loop patch by patch over RayTracer.trace, a K = 1 neighbour query and .item() tests

Verdict codes (`verdicts`, one per candidate): 0 accepted, 1 below y = 0 with no scan cloud (:1026), 2 a NaN ray origin (:1074), 3 farther than
min(0.1, 3 h_threshold) from the scan cloud (:1078), 4 a ray missed the mesh (:1083), 5 not looked at: max_patch_num was reached (:1113).

This module imports numpy only; torch and the HIP library are loaded by the two export functions.
"""
import numpy as np

ACCEPTED, BELOW, NAN_ORIGIN, FAR, MISSED, NOT_NEEDED = 0, 1, 2, 3, 4, 5
CHUNK_RAYS = 1 << 18  # the default chunk: as many candidates as give about this many rays
MAX_CHUNK = 65535     # candidates per front call (one grid row each)


def patch_grid_gap(vertices, faces, pattern_rate=1 / 50):
    """tools/map.py:966-969: the mean length of the unique undirected edges (trimesh's `edges_unique`) times pattern_rate."""
    v = np.asarray(vertices, dtype=np.float64)
    f = np.asarray(faces).astype(np.int64)
    edges_unique = np.unique(np.sort(f[:, [0, 1, 1, 2, 2, 0]].reshape(-1, 2), axis=1), axis=0)
    edges = v[edges_unique]
    edges = np.linalg.norm(edges[:, 0] - edges[:, 1], axis=-1)
    mean_edge_length = edges.mean()
    return float(mean_edge_length * pattern_rate)


def principal_direction(vertices):
    """sklearn.decomposition.PCA(n_components=3).fit(vertices).components_[0] (tools/map.py:973-981): the first right singular vector of the
    centred vertices, with sklearn's sign convention (svd_flip on the rows of V^T: the entry of largest magnitude is positive)."""
    v = np.asarray(vertices, dtype=np.float64)
    centred = v - v.mean(axis=0)
    _, _, vt = np.linalg.svd(centred, full_matrices=False)
    first = vt[0]
    return first * np.sign(first[np.argmax(np.abs(first))])


def patch_calibration(patch_size, grid_gap):
    """tools/map.py:985.  Pixel p = i S + j of a patch has the local coordinates (cal[i], cal[j]) (:986-987: meshgrid(indexing='ij'), stacked,
    reshaped)."""
    return np.linspace(-patch_size * grid_gap / 2, patch_size * grid_gap / 2, patch_size)


def patch_frames(points, normals, first_component):
    """tools/map.py:1030-1038 per candidate: -> [n,3,4] float64, T[:3,:4] = [x_axis | y_axis | z_axis | centre] (columns).  The
    `y_axis.sum() == 0` fallback is the reference's, exactly as written; where the normal is parallel to first_component the fallback is
    zero as well and the frame is NaN (such a candidate is refused by the NaN test of :1074)."""
    points = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    normals = np.asarray(normals, dtype=np.float64).reshape(-1, 3)
    first_component = np.asarray(first_component, dtype=np.float64)
    out = np.empty((points.shape[0], 3, 4), dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        for i in range(points.shape[0]):
            z_axis = normals[i]
            y_axis = np.cross(z_axis, first_component)
            if y_axis.sum() == 0:
                y_axis = np.cross(z_axis, np.array([1., 1., 1.01]) * first_component)
            y_axis = y_axis / np.linalg.norm(y_axis)
            x_axis = np.cross(y_axis, z_axis)
            out[i, :, :3] = np.stack([x_axis, y_axis, z_axis], -1)
            out[i, :, 3] = points[i]
    return out


def scan_limit(h_threshold):
    """min(0.1, 3 h_threshold) of tools/map.py:1078, rounded to fp32: the value both forms compare the fp32 distances with."""
    return float(np.float32(min(1e-1, 3 * h_threshold)))


# ------------------------------------------------------------------------------------------------------------ what both forms share
class _Setup:
    """The arguments of export_field resolved: candidates, frames, calibration, the tracer to cast on, the scan cloud's grid."""

    def __init__(self, field, sample_points, sample_normals, scan_points, first_component, grid_gap, pattern_rate, patch_size, max_patch_num, sample_mesh):
        import ctypes

        import torch

        from nerftex_hip import check, lib
        from RayTracer import RayTracer

        if getattr(field, "imported", False):
            raise NotImplementedError("CurvedField.export_field: the field reads an imported map; patches are sampled from the field's own mesh and table -- "
                                      "switch_import() back first")
        self.S, self.max_patch_num = int(patch_size), int(max_patch_num)
        if self.S < 1 or self.max_patch_num < 1:
            raise ValueError(f"CurvedField.export_field: patch_size and max_patch_num are at least 1, but got {patch_size} and {max_patch_num}")
        self.points = np.asarray(sample_points, dtype=np.float64).reshape(-1, 3)
        self.normals = np.asarray(sample_normals, dtype=np.float64).reshape(-1, 3)
        if self.points.shape != self.normals.shape:
            raise ValueError(f"CurvedField.export_field: one normal per candidate, but got {self.points.shape[0]} points and {self.normals.shape[0]} normals")
        self.dev = field.projector.mesh_vertices.device
        own_v, own_f = field.projector.mesh_vertices.detach().cpu().numpy(), field.mesh_faces
        if sample_mesh is None:
            cast_v, cast_f, self.tracer = own_v, own_f, field.projector.tracer
        else:
            cast_v, cast_f = np.asarray(sample_mesh[0]), np.asarray(sample_mesh[1])
            self.tracer = RayTracer(cast_v, cast_f)
        self.first_component = principal_direction(own_v) if first_component is None else np.asarray(first_component, dtype=np.float64)
        self.grid_gap = patch_grid_gap(cast_v, cast_f, pattern_rate) if grid_gap is None else float(grid_gap)
        self.calibration = patch_calibration(self.S, self.grid_gap)
        self.frames = patch_frames(self.points, self.normals, self.first_component)
        self.frames32 = np.ascontiguousarray(self.frames.astype(np.float32).reshape(-1, 12))
        self.cal32 = torch.from_numpy(self.calibration.astype(np.float32)).to(self.dev)
        self.limit = scan_limit(field.h_threshold)
        self.scan = None
        if scan_points is not None:
            host = np.ascontiguousarray(np.asarray(scan_points, dtype=np.float32).reshape(-1, 3))
            self.scan = ctypes.c_void_p()
            check(lib.nerftex_knn_create(host.ctypes.data, host.shape[0], ctypes.byref(self.scan)))
        n = self.points.shape[0]
        self.verdicts = np.zeros(n, dtype=np.uint8)
        if self.scan is None:
            self.verdicts[self.points[:, 1] < 0] = BELOW  # :1026
        self.sent = np.flatnonzero(self.verdicts == ACCEPTED)  # the candidates whose rays are cast, in candidate order

    def close(self):
        if self.scan is not None and self.scan.value:
            from nerftex_hip import lib

            lib.nerftex_knn_destroy(self.scan)
            self.scan = None


def _gather(field, inter):
    """:1087-1101 over the hits [N,3] of accepted patches, autocast off: -> (patches [N,16], local_tbn [N,9], phi_embed [N,8] or None)."""
    import torch

    with torch.no_grad(), torch.autocast("cuda", enabled=False):
        p_sur, _, _, _, local_tbn = field.projector.project(inter, K=field.projector.K, h_threshold=field.h_threshold)
        patch = field.encoder(p_sur, bound=field.bound)
        phi = field.normal_net.phi_embedding(p_sur) if field.normal_net is not None else None
    return patch.float(), local_tbn.reshape(-1, 9), None if phi is None else phi.float()


def _result(field, su, ids, patches, coors, local_tbn, phi, rays, record_rays):
    """The returned dict from the per-patch device tensors (lists, in patch order) and the accepted candidates' ids."""
    import torch

    S, P = su.S, len(ids)
    ids = np.asarray(ids, dtype=np.int64)

    def stack(parts, width):
        if parts is None:
            return None
        if not parts:
            return np.zeros((0, S, S, width), dtype=np.float32)
        return torch.cat(parts).reshape(P, S, S, width).cpu().numpy()

    frames32 = su.frames32.reshape(-1, 3, 4)[ids]
    return {
        "patches": stack(patches, field.encoder.output_dim),
        "grid_gap": su.grid_gap,
        "patch_coors": stack(coors, 3),
        "patch_norms": su.normals[ids].astype(np.float32),
        "patch_sample_tbn": np.ascontiguousarray(frames32[:, :, :3].transpose(0, 2, 1)).reshape(P, 9),
        "patch_local_tbn": stack(local_tbn, 9),
        "picked_vertices": su.points[ids].astype(np.float32),
        "patch_phi_embed": stack(phi, field.normal_net.encoder.output_dim) if field.normal_net is not None else None,
        "patch_rays": stack(rays if record_rays else None, 6),
        "candidate_ids": ids,
        "verdicts": su.verdicts,
    }


def _close_loop(su, ids):
    """The reference's loop has ended at the candidate that filled the last slot (:1113): whatever comes behind it was never looked at."""
    if len(ids) >= su.max_patch_num:
        su.verdicts[ids[su.max_patch_num - 1] + 1:] = NOT_NEEDED


# ------------------------------------------------------------------------------------------------------------------ the batched form
def export_field(field, sample_points, sample_normals, *, scan_points=None, first_component=None, grid_gap=None, pattern_rate=1 / 50, patch_size=128,
                 max_patch_num=2000, sample_mesh=None, record_rays=False, patches_per_chunk=None):
    """CurvedField.export_field(fused=True): see there."""
    import ctypes

    import torch

    from nerftex_hip import PatchFrontDesc, check, lib, ptr, stream

    su = _Setup(field, sample_points, sample_normals, scan_points, first_component, grid_gap, pattern_rate, patch_size, max_patch_num, sample_mesh)
    try:
        S, S2, dev = su.S, su.S * su.S, su.dev
        per_chunk = max(1, CHUNK_RAYS // S2) if patches_per_chunk is None else int(patches_per_chunk)
        per_chunk = max(1, min(per_chunk, MAX_CHUNK, 0xffffffff // S2))
        count = torch.zeros(1, dtype=torch.int32, device=dev)  # the device-resident running count
        frames_dev = torch.from_numpy(su.frames32).to(dev)
        ids, patches, coors, local_tbn, phi, rays = [], [], [], [], [], []
        for a in range(0, su.sent.shape[0], per_chunk):
            cand = su.sent[a:a + per_chunk]
            B = cand.shape[0]
            frames = frames_dev[torch.from_numpy(cand).to(dev)].contiguous()
            origins = torch.empty(B * S2, 3, device=dev)
            inter = torch.empty(B, S2, 3, device=dev)
            ray = torch.empty(B, S2, 6, device=dev) if record_rays else None
            stats = torch.empty(B, 4, dtype=torch.int32, device=dev)
            verdict = torch.empty(B, dtype=torch.uint8, device=dev)
            slot = torch.empty(B, dtype=torch.int32, device=dev)
            desc = PatchFrontDesc(tracer=su.tracer._handle.value, scan=None if su.scan is None else su.scan.value, frames=ptr(frames), calibration=ptr(su.cal32),
                                  B=B, S=S, max_scan_dist=su.limit, max_patch_num=su.max_patch_num, origins=ptr(origins), intersections=ptr(inter), rays=ptr(ray),
                                  stats=ptr(stats), verdict=ptr(verdict), slot=ptr(slot), count=ptr(count))
            check(lib.nerftex_patch_front(ctypes.byref(desc), stream()))
            back = torch.cat([slot, verdict.to(torch.int32)]).cpu().numpy()  # the chunk's one read-back
            slots, su.verdicts[cand] = back[:B], back[B:].astype(np.uint8)
            taken = np.flatnonzero(slots >= 0)
            assert np.array_equal(slots[taken], len(ids) + np.arange(taken.shape[0])), "nerftex_patch_front: slots are consecutive in candidate order"
            if taken.shape[0]:
                pick = torch.from_numpy(taken).to(dev)
                hits = inter[pick].reshape(-1, 3).contiguous()
                f, t, e = _gather(field, hits)
                patches.append(f), coors.append(hits), local_tbn.append(t), phi.append(e)
                if record_rays:
                    rays.append(ray[pick].reshape(-1, 6))
                ids += cand[taken].tolist()
            if len(ids) >= su.max_patch_num:
                break
        _close_loop(su, ids)
        return _result(field, su, ids, patches, coors, local_tbn, phi, rays, record_rays)
    finally:
        su.close()


# -------------------------------------------------------------------------------------------------------------------- the staged form
def _export_field_reference(field, sample_points, sample_normals, *, scan_points=None, first_component=None, grid_gap=None, pattern_rate=1 / 50, patch_size=128,
                            max_patch_num=2000, sample_mesh=None, record_rays=False):
    """CurvedField.export_field(fused=False): the reference's loop (tools/map.py:1024-1114) patch by patch over the package's own calls --
    RayTracer.trace, nerftex_knn_query over the scan cloud with K = 1, `.item()` tests.  The ray origins are formed by separate torch
    elementwise ops in the order of nerftex_patch_front: (T[a,0] x + T[a,1] y) + T[a,3], lifted by 0.1f T[a,2]."""
    import torch

    from nerftex_hip import check, lib, ptr, stream

    su = _Setup(field, sample_points, sample_normals, scan_points, first_component, grid_gap, pattern_rate, patch_size, max_patch_num, sample_mesh)
    try:
        S, S2, dev = su.S, su.S * su.S, su.dev
        x, y = su.cal32.repeat_interleave(S), su.cal32.repeat(S)  # pixel i S + j: (cal[i], cal[j])
        lift = torch.tensor(0.1, dtype=torch.float32, device=dev)
        ids, patches, coors, local_tbn, phi, rays = [], [], [], [], [], []
        for i in range(su.points.shape[0]):
            if su.verdicts[i] == BELOW:
                continue
            T = torch.from_numpy(su.frames32[i].reshape(3, 4)).to(dev)
            ray_origins = torch.stack([(T[k, 0] * x + T[k, 1] * y) + T[k, 3] for k in range(3)], dim=-1).contiguous()
            if ray_origins.isnan().any().item():
                su.verdicts[i] = NAN_ORIGIN
                continue
            if su.scan is not None:
                idx = torch.empty(S2, 1, dtype=torch.int32, device=dev)
                nn_dist = torch.empty(S2, 1, dtype=torch.float32, device=dev)
                check(lib.nerftex_knn_query(su.scan, ptr(ray_origins), S2, 1, ptr(idx), ptr(nn_dist), stream()))
                if nn_dist.max().item() > su.limit:
                    su.verdicts[i] = FAR
                    continue
            ray_origins = ray_origins + lift * T[:, 2]
            ray_directions = (-T[:, 2]).expand(S2, 3).contiguous()
            intersections, _, depth, _ = su.tracer.trace(ray_origins, ray_directions)
            if depth.max().item() > 9.5:
                su.verdicts[i] = MISSED
                continue
            f, t, e = _gather(field, intersections)
            patches.append(f), coors.append(intersections), local_tbn.append(t), phi.append(e)
            if record_rays:
                rays.append(torch.cat([ray_origins, ray_directions], dim=-1))
            ids.append(i)
            if len(ids) == su.max_patch_num:
                break
        _close_loop(su, ids)
        return _result(field, su, ids, patches, coors, local_tbn, phi, rays, record_rays)
    finally:
        su.close()
