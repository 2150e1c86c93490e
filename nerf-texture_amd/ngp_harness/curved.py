"""Config 4 harness: the curved-field texture of the reference without its six un-vendored packages (frnn, pytorch3d, tinycudann,
xatlas, open3d, trimesh).

  MeshProjector      tools/map.py:340-502: K nearest mesh vertices (the role of frnn: csrc/knn.hip) -> Shepard-weighted coarse normal
                     -> two BVH closest-hit traces along +-normal -> nearer hit = surface point, signed height, face, frame, mask;
                     `project` is the fused kernel (nerftex_curved_project), `project_reference` the reference's op sequence;
  CurvedField        MeshFeatureField.forward (tools/map.py:620-641, 717-737) + network_curvedfield.NeRFNetwork.forward / density
                     (nerf/network_curvedfield.py:229-243, 283-300, 382-409) with the static light model: projector ->
                     GridEncoder_clustering(p_sur) ++ FreqEncoder(height) (16 + 25 = 41, padded to 48 with ones the way tcnn pads)
                     -> FFMLP 48-32-16 -> trunc_exp / geo features; reflection of the view direction about the coarse normal -> SH(4)
                     ++ geo (31, padded to 32) -> FFMLP 32-64-64-3 -> sigmoid; both masked by the height mask.  A field
                     `ngp_harness.model.Renderer` can march.  The tcnn networks are served by the in-tree FFMLP (the reference's own
                     transplant of the same fully-fused kernel): tests/golden/ref_python_curvedfield.npz pins the chain against the
                     reference's modules executed with exactly that substitution.  light_model="SH" (main.py's model, :272-349):
                     no direction encoding and no colour MLP; the SH light head (light.SHLightNet) shades with the fine normal of the
                     factorized normal net.  import_field / import_shape: an imported planar feature map rendered on its own plane or
                     on a new UV-mapped mesh (the 'field' and 'shape' branches of MeshFeatureField.forward, tools/map.py:646-700); with the
                     normal net or the light model, the planar map comes with its phi_embed, local_tbn and sample_tbn maps (:670-675);
                     unhash / import_unhash_vertices: the field's own table baked onto the vertices of a finely subdivided mesh and
                     interpolated at the hit (the 'unhash' branch, :708-714; the static light model only);
  CurvedFieldLookup  round 1's minimal chain (analytic normals -> traces -> hash lookup), kept for its test.
"""
from typing import NamedTuple, Optional

import numpy as np
import torch

from gridencoder import GridEncoder_clustering
from nerftex_hip import (LIGHT_VISUAL, SH_LIGHT_SPECULAR, CurvedImportInferDesc, CurvedInferDesc, CurvedLightImportInferDesc, CurvedLightInferDesc,
                         CurvedLightPatchInferDesc, CurvedLightShapeInferDesc, CurvedPatchInferDesc, CurvedShapeInferDesc, CurvedUnhashInferDesc, RelightDesc, ptr)
from RayTracer import RayTracer

from .subdivide import subdivide_midpoint, subdivide_until  # noqa: F401  (subdivide_midpoint: for the callers who bake a mesh of their own)


def star_flower_mesh(n_lat=72, n_lon=144, lobes=5, amp=0.18, radius=0.7):
    """UV-sphere with r(theta, phi) = radius * (1 + amp * sin(theta)^2 * cos(lobes * phi)): ~20 k triangles."""
    theta = np.linspace(0, np.pi, n_lat + 1)
    phi = np.linspace(0, 2 * np.pi, n_lon, endpoint=False)
    T, P = np.meshgrid(theta, phi, indexing="ij")
    r = radius * (1 + amp * np.sin(T) ** 2 * np.cos(lobes * P))
    v = np.stack([r * np.sin(T) * np.cos(P), r * np.cos(T), r * np.sin(T) * np.sin(P)], -1).reshape(-1, 3)
    faces = []
    for i in range(n_lat):
        for j in range(n_lon):
            a = i * n_lon + j
            b = i * n_lon + (j + 1) % n_lon
            c = (i + 1) * n_lon + j
            d = (i + 1) * n_lon + (j + 1) % n_lon
            if i > 0:
                faces.append((a, c, b))
            if i < n_lat - 1:
                faces.append((b, c, d))
    return v.astype(np.float32), np.asarray(faces, dtype=np.uint32)


def vertex_normals(vertices, faces):
    """Area-weighted vertex normals of a triangle mesh (what open3d's compute_vertex_normals gives the reference, tools/map.py:396)."""
    v = torch.as_tensor(vertices, dtype=torch.float32)
    f = torch.as_tensor(np.asarray(faces, dtype=np.int64))
    fn = torch.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]], dim=-1)
    vn = torch.zeros_like(v)
    for k in range(3):
        vn.index_add_(0, f[:, k], fn)
    return vn / (vn.norm(dim=-1, keepdim=True) + 1e-12)


def knn_bruteforce(xyz, vertices, K=8, chunk=8192):
    """K nearest mesh vertices per point, ascending (distances euclidean), by cdist + topk: the test reference of MeshProjector.knn."""
    idx, dist = [], []
    for a in range(0, xyz.shape[0], chunk):
        d = torch.cdist(xyz[a:a + chunk], vertices)
        dd, ii = torch.topk(d, K, dim=-1, largest=False, sorted=True)
        idx.append(ii.int())
        dist.append(dd)
    return torch.cat(idx).contiguous(), torch.cat(dist).contiguous()


class diff_project_layer(torch.autograd.Function):
    """tools/map.py:171-186: the projection made differentiable in x by FIAT -- forward hands (xyz, p_sur, sdf, normal) through unchanged; the
    backward routes dL/dp_sur (its component parallel to the surface: the foot point moves with x along the tangent plane) and dL/dsdf (along
    the unit normal: the height changes with x along it) to dL/dxyz.  Used by MeshProjector.project(requires_grad_xyz=True) -> the visual /
    light-model branch of network_curvedfield.py:236-259, where sigma is differentiated with respect to the sample position."""

    @staticmethod
    def forward(ctx, xyz, p_sur, sdf, normal):
        ctx.save_for_backward(normal)
        return xyz, p_sur, sdf, normal

    @staticmethod
    def backward(ctx, g_xyz, g_psur, g_sdf, g_normal):
        normal = ctx.saved_tensors[0]
        normal = normal / (normal.norm(dim=-1, keepdim=True) + 1e-5)
        g_xyz_parallel2surface = g_psur - normal * (normal * g_psur).sum(dim=-1, keepdim=True)
        g_xyz_along_normal = g_sdf * normal
        return g_xyz_along_normal + g_xyz_parallel2surface, g_psur, g_sdf, g_normal


def freq_encode(x, multires=12):
    """tools/encoding.py:5-43 FreqEncoder as get_encoder('frequency', multires=...) builds it (log-sampled bands 2^0 .. 2^(multires-1), input
    included): [x, sin(x f_0), cos(x f_0), sin(x f_1), ...].  Framework ops -- differentiable; the fused projector kernel evaluates the same
    ladder for the no-grad path."""
    bands = (2.0 ** torch.linspace(0.0, multires - 1, multires)).tolist()
    out = [x]
    for f in bands:
        out += [torch.sin(x * f), torch.cos(x * f)]
    return torch.cat(out, dim=-1)


def shape_vertices(vertices, normalize=True):
    """The float64 vertices `shape_preprocess` rounds to fp32 -- what the reference's trimesh mesh holds behind NeRFNetwork.import_shape's
    normalisation, and what its calculate_tbn reads (`uv_face_frames`)."""
    v = np.array(vertices, dtype=np.float64)
    if normalize:
        v -= np.mean(v, axis=0)
        v /= (np.absolute(v).max() + 1e-5)
        v /= 1.2
    return v


def shape_preprocess(vertices, faces, uvs, normalize=True):
    """What NeRFNetwork.import_shape and MeshProjector's constructor make of a loaded mesh before anything touches a device:
    -> (vertices [V,3] fp32, uvs [V,2] fp32 in [-1,1], face_uv [F,6] fp32 = uvs[faces], recommended_sdf_factor).
    normalize (network_curvedfield.py:496-498, float64): centre by the vertex mean, divide by max|v| + 1e-5, then by 1.2.
    uvs (tools/map.py:361, fp32): mapped to [-1,1] by their single global minimum and maximum.
    recommended_sdf_factor (:373-386): the mean 3-D length (float64) over the mean UV length (fp32) of the unique edges."""
    v = shape_vertices(vertices, normalize)
    f = np.asarray(faces).astype(np.int64)
    uv = torch.FloatTensor(np.asarray(uvs, dtype=np.float32))
    uv = ((uv - uv.min()) / (uv.max() - uv.min()) * 2 - 1.).numpy()
    edges = np.sort(f[:, [0, 1, 1, 2, 2, 0]].reshape(-1, 2), axis=1)
    edges = np.unique(edges, axis=0)
    e3 = v[edges]
    mean_edge_length = np.linalg.norm(e3[:, 0] - e3[:, 1], axis=-1).mean()
    e2 = uv[edges]
    mean_edges_uv = np.linalg.norm(e2[:, 0] - e2[:, 1], axis=-1).mean()
    return v.astype(np.float32), uv, np.ascontiguousarray(uv[f].reshape(-1, 6)), float(mean_edge_length / mean_edges_uv)


def uv_face_frames(vertices, faces, uvs):
    """The per-face frames of a UV-mapped mesh as MeshProjector's constructor computes them (calculate_tbn, tools/map.py:119-138, called at :366
    with the normalised mesh and the [-1, 1] UVs): -> [F, 3, 3] fp32, rows t, b, n.  Per face, in float64 over the vertices: the 2 x 2 matrix of
    the two UV edges is inverted (a matrix of rank < 2 gets 1e-3 added to its element [1, 1] first, every such matrix when there is one) and
    multiplied by the two 3-D edges -> t, b; n is the face normal (the normalised cross product of the first two edges, trimesh's
    `face_normals`); b is replaced by n x t; every row is divided by its length.  The UV edges keep the dtype `uvs` comes in: the reference
    hands over fp32 UVs, so rank and inverse are numpy's fp32 ones there, and `shape_preprocess` returns them as fp32 for that reason."""
    v = np.asarray(vertices, dtype=np.float64)
    f = np.asarray(faces).astype(np.int64)
    uv = np.asarray(uvs)
    if not np.issubdtype(uv.dtype, np.floating):
        uv = uv.astype(np.float64)
    fv, fuv = v[f], uv[f]
    e3 = fv[:, 1:] - fv[:, :1]
    e2 = fuv[:, 1:] - fuv[:, :1]
    rank = np.linalg.matrix_rank(e2)
    if rank.min() < 2:
        e2[np.where(rank < 2)[0], 1, 1] += 1e-3
    tb = np.einsum("fij,fjk->fik", np.linalg.inv(e2), e3)  # [t; b] per face
    n = np.cross(e3[:, 0], e3[:, 1])
    n = n / np.linalg.norm(n, axis=-1, keepdims=True)
    tbn = np.concatenate([tb, n[:, None]], axis=1)
    tbn[:, 1] = np.cross(tbn[:, 2], tbn[:, 0], axis=-1)
    tbn = tbn / np.linalg.norm(tbn, axis=-1, keepdims=True)
    return tbn.astype(np.float32)


def shape_knn_normal(xyz, idx, dis, mesh_vertices, vertex_normals):
    """knn(use_dir_vec=False, weighting='DualD', nn_consis_check=True) of tools/map.py:454-501, op for op: dual-distance weights over the
    neighbours on the nearest one's side of the point.  0 / 0 = NaN where every kept distance ties (as in the reference)."""
    normals = vertex_normals[idx.long()]
    dir_vec_ori = xyz.unsqueeze(-2) - mesh_vertices[idx.long()]
    dir_vec = dir_vec_ori / (dir_vec_ori.norm(dim=-1, keepdim=True) + 1e-5)
    dir_vec_cosine = (dir_vec * dir_vec[..., :1, :]).sum(-1)
    dis = torch.where(dir_vec_cosine > 0, dis, 1e5 * torch.ones_like(dis))
    dk = dis.max(dim=-1, keepdim=True)[0]
    d1 = dis.min(dim=-1, keepdim=True)[0]
    weights = (dk - dis) / (dk - d1 + 1e-5) * (dk + d1) / (dk + dis)
    weights = weights / torch.sum(weights, dim=-1, keepdims=True)
    normals = normals / (normals.norm(dim=-1, keepdim=True) + 1e-5)
    normal = (normals * weights.unsqueeze(-1)).sum(-2)
    return normal / (normal.norm(dim=-1, keepdim=True) + 1e-5)


def points_to_barycentric(triangles, points):
    """tools/map.py:85-93: area coordinates of `points` [N,3] in `triangles` [N,3,3] (sub-triangle areas over their sum + 1e-5)."""
    p2v = triangles - points.unsqueeze(-2)
    s0 = torch.cross(p2v[..., 1, :], p2v[..., 2, :], dim=-1).norm(dim=-1)
    s1 = torch.cross(p2v[..., 2, :], p2v[..., 0, :], dim=-1).norm(dim=-1)
    s2 = torch.cross(p2v[..., 0, :], p2v[..., 1, :], dim=-1).norm(dim=-1)
    barycentric = torch.stack([s0, s1, s2], dim=-1)
    return barycentric / (barycentric.sum(dim=-1, keepdim=True) + 1e-5)


class MeshProjector(torch.nn.Module):
    """The part of tools/map.py's MeshProjector the curved field uses per sample -- `knn` (:454-501) and `project` (:414-433):
    `project(xyz, K=8, h_threshold=None, requires_grad_xyz=False, use_dir_vec=True) -> (p_sur, sdf, h_mask, normal, tbn)` is the
    reference's signature and tuple, served by the fused kernel (nerftex_curved_project: neighbour-weighted normal + two BVH traces + select
    + mask + frame in one launch) whenever use_dir_vec is on; `project_fused` is that kernel's full output (adds the face index and
    FreqEncoder(height)); `project_reference` restates the reference's framework-op sequence over RayTracer.trace."""

    def __init__(self, vertices, faces, h_threshold=0.05, K=8, vertex_normals=None, tbn=None):
        """vertex_normals / tbn: the mesh's own (the reference takes them from open3d and from its UV map, tools/map.py:365-366,396);
        default: area-weighted normals and an edge-aligned per-face frame."""
        super().__init__()
        import ctypes

        from nerftex_hip import check, lib

        self.tracer = RayTracer(vertices, faces)
        v = torch.as_tensor(np.asarray(vertices), dtype=torch.float32)
        f = torch.as_tensor(np.asarray(faces, dtype=np.int64))
        self.register_buffer("mesh_vertices", v.contiguous())
        vn = globals()["vertex_normals"](vertices, faces) if vertex_normals is None else torch.as_tensor(np.asarray(vertex_normals), dtype=torch.float32)
        self.register_buffer("vertex_normals", vn.contiguous())
        if tbn is None:
            e1, e2 = v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]]
            t = e1 / (e1.norm(dim=-1, keepdim=True) + 1e-12)
            n = torch.cross(e1, e2, dim=-1)
            n = n / (n.norm(dim=-1, keepdim=True) + 1e-12)
            tbn = torch.stack([t, torch.cross(n, t, dim=-1), n], dim=1)  # a per-face frame (rows t, b, n)
        self.register_buffer("tbn", torch.as_tensor(np.asarray(tbn), dtype=torch.float32).contiguous())
        self.h_threshold, self.K, self.depth_threshold = h_threshold, min(K, v.shape[0]), 9.5
        # the vertex grid of the neighbour search (tools/map.py:396 builds frnn's once, too)
        self._knn = ctypes.c_void_p()
        host = np.ascontiguousarray(v.numpy(), dtype=np.float32)
        check(lib.nerftex_knn_create(host.ctypes.data, host.shape[0], ctypes.byref(self._knn)))

    def __del__(self):
        h = getattr(self, "_knn", None)
        if h is not None and h.value:
            from nerftex_hip import lib

            lib.nerftex_knn_destroy(h)
            self._knn = None

    @torch.no_grad()
    def knn(self, xyz, K=None):
        """(idx [N,K] int32, dis [N,K]) -- the K nearest mesh vertices, ascending, euclidean: what knn() holds after
        `dis.sqrt()` (tools/map.py:456-458).  Exact (csrc/knn.hip)."""
        from nerftex_hip import check, lib, ptr, stream

        K = self.K if K is None else min(K, self.mesh_vertices.shape[0])
        xyz = xyz.float().contiguous()
        idx = torch.empty(xyz.shape[0], K, dtype=torch.int32, device=xyz.device)
        dis = torch.empty(xyz.shape[0], K, dtype=torch.float32, device=xyz.device)
        check(lib.nerftex_knn_query(self._knn, ptr(xyz), xyz.shape[0], K, ptr(idx), ptr(dis), stream()))
        return idx, dis

    def knn_normal(self, xyz, idx, dis, dir_vec_wdist=0.05, use_dir_vec=True):
        """knn() with weighting='Shepard' (tools/map.py:454-501), op for op; use_dir_vec: the inverse-distance mean of the directions to the
        neighbours joins their normals as one more candidate (:473-481)."""
        normals = self.vertex_normals[idx.long()]
        dir_vec_ori = xyz.unsqueeze(-2) - self.mesh_vertices[idx.long()]
        dir_vec = dir_vec_ori / (dir_vec_ori.norm(dim=-1, keepdim=True) + 1e-5)
        if use_dir_vec:
            weights_invd = 1 / (dis + 1e-7)
            mean_dir_vec = (weights_invd.unsqueeze(-1) * dir_vec).sum(1, keepdims=True)
            normal_test = normals.mean(1, keepdims=True)
            mean_dir_vec = torch.where((mean_dir_vec * normal_test).sum(dim=-1, keepdims=True) < 0, -mean_dir_vec, mean_dir_vec)
            mean_dir_vec = mean_dir_vec / (mean_dir_vec.norm(dim=-1, keepdim=True) + 1e-5)
            normals = torch.cat([normals, mean_dir_vec], dim=1)
            dis = torch.cat([dis, float(np.clip(dir_vec_wdist, 1e-5, np.inf)) * torch.ones_like(dis[:, :1])], dim=1)
        weights = 1 / (dis + 1e-7)
        weights = weights / torch.sum(weights, dim=-1, keepdims=True)
        normals = normals / (normals.norm(dim=-1, keepdim=True) + 1e-5)
        normal = (normals * weights.unsqueeze(-1)).sum(-2)
        return normal / (normal.norm(dim=-1, keepdim=True) + 1e-5)

    def _height_limit(self, h_threshold):
        """min(depth_threshold, h_threshold) of tools/map.py:427-429; None = no limit but the tracer's own (9.5).  The module's default
        (its constructor's h_threshold) applies when the caller passes the sentinel `...`."""
        if h_threshold is ...:
            h_threshold = self.h_threshold
        return float(min(self.depth_threshold, np.inf if h_threshold is None else h_threshold))

    @torch.no_grad()
    def project_reference(self, xyz, neighbours=None, K=None, h_threshold=..., use_dir_vec=True):
        idx, dis = self.knn(xyz, K) if neighbours is None else neighbours
        normal = self.knn_normal(xyz, idx, dis, use_dir_vec=use_dir_vec)
        p1, _, d1, f1 = self.tracer.trace(xyz, normal)
        p2, _, d2, f2 = self.tracer.trace(xyz, -normal)
        cond = d1 < d2
        p_sur = torch.where(cond.unsqueeze(-1), p1, p2)
        sdf = torch.where(cond, -d1, d2).unsqueeze(-1)
        face_idx = torch.where(cond, f1, f2)
        h_mask = (sdf.abs() < self._height_limit(h_threshold)).squeeze(-1)
        return p_sur, sdf, h_mask, normal, self.tbn[face_idx], face_idx

    def project(self, xyz, K=8, h_threshold=None, requires_grad_xyz=False, use_dir_vec=True):
        """tools/map.py:414-433, the reference's signature and return value: -> (p_sur [N,3], sdf [N,1], h_mask [N] bool, normal [N,3],
        tbn [N,3,3]).  requires_grad_xyz: the outputs carry the reference's gradient to xyz (`diff_project_layer`)."""
        with torch.no_grad():
            if use_dir_vec:
                p_sur, sdf, h_mask, normal, tbn, _, _ = self.project_fused(xyz.detach(), multires=0, K=K, h_threshold=h_threshold)
            else:  # (no kernel for the plain neighbour-normal average: the reference's op sequence over the tracer)
                p_sur, sdf, h_mask, normal, tbn, _ = self.project_reference(xyz.detach().float().contiguous(), K=K, h_threshold=h_threshold, use_dir_vec=False)
        if requires_grad_xyz:
            xyz, p_sur, sdf, normal = diff_project_layer.apply(xyz, p_sur, sdf, normal)
        return p_sur, sdf, h_mask, normal, tbn

    @torch.no_grad()
    def project_fused(self, xyz, multires=12, neighbours=None, K=None, h_threshold=...):
        """-> p_sur [N,3], sdf [N,1], h_mask [N] bool, normal [N,3], tbn [N,3,3], face_idx [N], z_embed [N, 1 + 2 multires]: `project`
        (use_dir_vec=True) plus the face index and FreqEncoder(height), one launch behind the neighbour search.
        neighbours: (idx [N,K] int32, dis [N,K]) of a neighbour search done elsewhere; default = the library's own (self.knn).
        h_threshold: `...` = the module's own (its constructor argument), None = no limit but the tracer's (9.5)."""
        from nerftex_hip import check, lib, ptr, stream

        xyz = xyz.float().contiguous()
        N, dev = xyz.shape[0], xyz.device
        idx, dis = self.knn(xyz, K) if neighbours is None else neighbours
        idx, dis = idx.int().contiguous(), dis.float().contiguous()
        p_sur = torch.empty(N, 3, device=dev)
        sdf = torch.empty(N, device=dev)
        mask = torch.empty(N, dtype=torch.uint8, device=dev)
        normal = torch.empty(N, 3, device=dev)
        face_idx = torch.empty(N, dtype=torch.int64, device=dev)
        tbn = torch.empty(N, 9, device=dev)
        z = torch.empty(N, 1 + 2 * multires, device=dev)
        check(lib.nerftex_curved_project(self.tracer._handle, ptr(xyz), ptr(idx), ptr(dis), N, idx.shape[1], ptr(self.mesh_vertices), ptr(self.vertex_normals), self.mesh_vertices.shape[0], 0.05,
                                         self._height_limit(h_threshold), ptr(self.tbn), multires, ptr(p_sur), ptr(sdf), ptr(mask), ptr(normal), ptr(face_idx), ptr(tbn),
                                         ptr(z), stream()))
        return p_sur, sdf.unsqueeze(-1), mask.bool(), normal, tbn.view(N, 3, 3), face_idx, z


class LipLayer(torch.nn.Module):
    """tools/map.py:211-228: y = act(W_n x + b) with the rows of W scaled down to an l1 norm of at most softplus(c) (a Lipschitz bound that is
    itself trained)."""

    def __init__(self, in_dim, out_dim, act=True):
        super().__init__()
        self.act = act
        self.W = torch.nn.Parameter(torch.randn(out_dim, in_dim).float() * 1e-1)
        self.b = torch.nn.Parameter(torch.zeros(out_dim, dtype=torch.float32))
        self.c = torch.nn.Parameter(torch.ones([], dtype=torch.float32))

    def bound(self):
        return torch.nn.functional.softplus(self.c)

    def normalization(self):
        absrowsum = self.W.abs().sum(dim=1)
        scale = torch.minimum(torch.ones_like(absrowsum), self.bound() / absrowsum)
        return self.W * scale[..., None]

    def forward(self, x):
        y = torch.einsum("ab,nb->na", self.normalization(), x) + self.b
        return torch.relu(y) if self.act else y


class LipMLP(torch.nn.Module):
    """tools/map.py:189-208: num_layers hidden LipLayers of n_neurons + a linear LipLayer; regularization() = the product of the layers' bounds."""

    def __init__(self, in_dim, out_dim, n_neurons=64, num_layers=3):
        super().__init__()
        dims = [in_dim] + [n_neurons] * num_layers
        self.layers = torch.nn.ModuleList([LipLayer(a, b) for a, b in zip(dims[:-1], dims[1:])] + [LipLayer(dims[-1], out_dim, act=False)])
        # the reference registers its layers twice (tools/map.py:190-199: `self.layers` and `self.layers_seq = nn.Sequential(*layers)`): its checkpoints
        # carry both `layers.N.*` and `layers_seq.N.*` keys for the same tensors.  The same modules under the second name: a strict load succeeds
        self.layers_seq = torch.nn.Sequential(*self.layers)

    def forward(self, x):
        for layer in self.layers:
            x = layer(x)
        return x

    def regularization(self):
        loss = 1.0
        for layer in self.layers:
            loss = loss * layer.bound()
        return loss


class FactorizedNormalNet(torch.nn.Module):
    """tools/map.py:231-337 `Factorized_Normal_Net` (lip=True, direct_pred_coor=False: what MeshFeatureField builds by default, :585-588): the fine
    normal in the local frame as two angles -- phi (anisotropic) from a hash grid of its own over the surface point (L = 4, 512 -> 1024,
    2^19 rows, align_corners: :235; one more G1 caller, and a G3 caller when p_sur carries a gradient) ++ the first 12 height bands, theta
    (isotropic) from the first 32 texture features ++ the same height bands, each through a 2 x 16 LipMLP; normal = (sin t cos p, sin t sin p,
    cos t), optionally rotated by a per-point frame.  The networks are 16 wide: framework ops, as in the reference (its tcnn alternative,
    lip=False, is the un-vendored dependency)."""

    def __init__(self, x_dim, z_dim, theta_scale=np.pi / 2 * 1.1, phi_scale=np.pi * 2 * 1.1, bound_output=False, low_freq_band_len_f=32, low_freq_band_len_z=12):
        super().__init__()
        from gridencoder import GridEncoder

        self.encoder = GridEncoder(input_dim=3, num_levels=4, level_dim=2, base_resolution=512, log2_hashmap_size=19, desired_resolution=1024, gridtype="hash",
                                   align_corners=True)
        self.low_freq_band_len_x = min(x_dim, low_freq_band_len_f)
        self.low_freq_band_len_z = min(z_dim, low_freq_band_len_z)
        self.phi_net = LipMLP(in_dim=self.encoder.output_dim + self.low_freq_band_len_z, out_dim=1, n_neurons=16, num_layers=2)
        self.theta_net = LipMLP(in_dim=self.low_freq_band_len_x + self.low_freq_band_len_z, out_dim=1, n_neurons=16, num_layers=2)
        self.theta_scale, self.phi_scale, self.bound_output = theta_scale, phi_scale, bound_output

    def regularization(self):
        return self.phi_net.regularization() + self.theta_net.regularization()

    @staticmethod
    def toCoor(phi, theta):
        sin_theta = torch.sin(theta)
        return torch.cat([sin_theta * torch.cos(phi), sin_theta * torch.sin(phi), torch.cos(theta)], dim=-1)

    def phi_embedding(self, p_sur):
        return self.encoder(p_sur)

    def forward(self, z_embed, x_embed, p_sur=None, phi_embed=None, tbn=None, return_rot_angles=False):
        assert p_sur is None or phi_embed is None, "Only one of p_sur and phi_embed is None"
        if p_sur is not None:
            phi_embed = self.encoder(p_sur)
        zl = z_embed[..., :self.low_freq_band_len_z].float()
        phi = self.phi_net(torch.cat([phi_embed.float(), zl], dim=-1))
        theta = self.theta_net(torch.cat([x_embed[..., :self.low_freq_band_len_x].float(), zl], dim=-1))
        if self.bound_output:
            theta = self.theta_scale * torch.sigmoid(theta)
            phi = self.phi_scale * torch.sigmoid(phi)
        if return_rot_angles:
            return theta, phi
        normal = self.toCoor(phi=phi, theta=theta)
        return normal if tbn is None else torch.einsum("na,nab->nb", normal, tbn)


class CurvedFieldLookup(torch.nn.Module):
    def __init__(self, vertices, faces, bound=1.0, h_threshold=0.05):
        super().__init__()
        self.tracer = RayTracer(vertices, faces)
        self.bound = bound
        self.h_threshold = min(9.5, h_threshold)
        # tools/map.py:563
        self.encoder = GridEncoder_clustering(input_dim=3, num_levels=8, level_dim=2, base_resolution=512, log2_hashmap_size=19,
                                              desired_resolution=1024, gridtype="hash", align_corners=True)

    @torch.no_grad()
    def project(self, x, normals):
        """Nearest surface point along +-normal (tools/map.py:419-430)."""
        p_pos, _, d_pos, f_pos = self.tracer.trace(x, normals)
        p_neg, _, d_neg, f_neg = self.tracer.trace(x, -normals)
        use_pos = d_pos < d_neg  # tools/map.py:421: strict, a tie (double miss) takes the -normal record
        p_sur = torch.where(use_pos.unsqueeze(-1), p_pos, p_neg)
        sdf = torch.where(use_pos, -d_pos, d_neg)  # outside the surface (hit along -n) is positive height
        face = torch.where(use_pos, f_pos, f_neg)
        return p_sur, sdf, face

    def forward(self, x, normals):
        p_sur, sdf, face = self.project(x, normals)
        h_mask = sdf.abs() < self.h_threshold
        feat = self.encoder(p_sur, bound=self.bound)
        return feat, sdf, face, h_mask


class _TruncExp(torch.autograd.Function):  # tools/activation.py:5-17
    @staticmethod
    def forward(ctx, x):
        x = x.float()
        ctx.save_for_backward(x)
        return torch.exp(x)

    @staticmethod
    def backward(ctx, g):
        (x,) = ctx.saved_tensors
        return g * torch.exp(x.clamp(-15, 15))


class _SourceLookup(NamedTuple):
    """What CurvedField._source_lookup hands embed(), density() and forward(), whichever source is imported."""
    h_mask: torch.Tensor
    normal: Optional[torch.Tensor]  # raw; None: the planar map's (0, 0, 1)
    xin: torch.Tensor
    phi: Optional[torch.Tensor] = None  # lit only
    frames: tuple = ()  # lit only, in `_rotate_fine`'s order


class _CurvedPack(torch.autograd.Function):
    """[x_embed | half(z_embed) | ones] -- the sigma net's padded input (tools/map.py:641 `torch.cat` + tcnn's padding with ones) as one launch."""

    @staticmethod
    def forward(ctx, x_embed, z_embed):
        from nerftex_hip import check, lib, ptr, stream

        x_embed, z_embed = x_embed.contiguous(), z_embed.contiguous()
        out = torch.empty(x_embed.shape[0], 48, dtype=torch.float16, device=x_embed.device)
        check(lib.nerftex_curved_pack_inputs(ptr(x_embed), ptr(z_embed), x_embed.shape[0], ptr(out), stream()))
        return out

    @staticmethod
    def backward(ctx, g):
        return g[:, :16].contiguous(), None


class _CurvedMid(torch.autograd.Function):
    """sigma net output h -> (sigma = trunc_exp(h[:, 0]), the colour net's input [SH4(reflected view direction) | h[:, 1:16] | 1]): the ~20 framework ops
    of network_curvedfield.py:283-306 as one launch; the backward is the ngp field's (nerftex_field_mid_backward: trunc_exp's derivative + the slice)."""

    @staticmethod
    def forward(ctx, h, normal, dirs, fc_weight, eval_mode):
        from nerftex_hip import check, lib, ptr, stream

        h, normal, dirs = h.contiguous(), normal.contiguous().float(), dirs.contiguous().float()
        B = h.shape[0]
        sigma = torch.empty(B, dtype=torch.float16, device=h.device)
        cin = torch.empty(B, 32, dtype=torch.float16, device=h.device)
        check(lib.nerftex_curved_mid_forward(ptr(h), ptr(normal), ptr(dirs), B, float(fc_weight), int(eval_mode), ptr(sigma), ptr(cin), stream()))
        ctx.save_for_backward(h)
        ctx.set_materialize_grads(False)
        return sigma, cin

    @staticmethod
    def backward(ctx, g_sigma, g_cin):
        from nerftex_hip import check, lib, ptr, stream

        (h,) = ctx.saved_tensors
        B = h.shape[0]
        g_sigma = torch.zeros(B, dtype=torch.float32, device=h.device) if g_sigma is None else g_sigma.contiguous().float()
        g_cin = torch.zeros(B, 32, dtype=torch.float16, device=h.device) if g_cin is None else g_cin.contiguous().half()
        g_h = torch.empty_like(h)
        check(lib.nerftex_field_mid_backward(ptr(g_sigma), ptr(g_cin), ptr(h), B, ptr(g_h), stream()))
        return g_h, None, None, None, None


class _CurvedOut(torch.autograd.Function):
    """(colour net output, sigma, h_mask) -> (masked sigma, masked sigmoid colour): sigmoid + two zeros_like + two where as one launch."""

    @staticmethod
    def forward(ctx, hc, sigma_raw, mask):
        from nerftex_hip import check, lib, ptr, stream

        assert hc.dtype == torch.float16 and hc.shape[1] == 3 and hc.stride(1) == 1
        B = hc.shape[0]
        sigma_raw, mask_b = sigma_raw.contiguous(), mask.contiguous().view(torch.uint8)
        sigma = torch.empty(B, dtype=torch.float16, device=hc.device)
        color = torch.empty(B, 3, dtype=torch.float16, device=hc.device)
        check(lib.nerftex_curved_out_forward(ptr(hc), int(hc.stride(0)), ptr(sigma_raw), ptr(mask_b), B, ptr(sigma), ptr(color), stream()))
        ctx.save_for_backward(color, mask)
        ctx.set_materialize_grads(False)
        return sigma, color

    @staticmethod
    def backward(ctx, g_sigma, g_color):
        color, mask = ctx.saved_tensors
        g_raw = None if g_sigma is None else torch.where(mask, g_sigma, torch.zeros_like(g_sigma))
        g_hc = None if g_color is None else (g_color * (1 - color)) * color  # (0 where masked: the colour is 0 there)
        return g_hc, g_raw, None


class PointGrid:
    """The neighbour grid (nerftex_knn) over a point cloud without a mesh -- an imported patch's points --, destroyed with the object."""

    def __init__(self, points, device):
        import ctypes

        from nerftex_hip import check, lib

        host = np.ascontiguousarray(points, dtype=np.float32)
        self._handle, self.n_points = ctypes.c_void_p(), int(host.shape[0])
        with torch.cuda.device(device):
            check(lib.nerftex_knn_create(host.ctypes.data, host.shape[0], ctypes.byref(self._handle)))

    @property
    def value(self):
        return self._handle.value

    def __del__(self):
        h = getattr(self, "_handle", None)
        if h is not None and h.value:
            try:
                from nerftex_hip import lib
            except ImportError:  # (the interpreter is shutting down: the process's memory goes with it)
                return
            lib.nerftex_knn_destroy(h)
            self._handle = None


class CurvedField(torch.nn.Module):
    """The curved-field network with the static light model (see the module docstring), over a MeshProjector.

    forward(x, d) -> (sigma [N], rgb [N,3], {}) and density(x) -> {"sigma", "geo_feat"}: the interface Renderer marches.
    prob_model: the reference's second table of log-variances (tools/map.py:564-566, 627-630); its noise is drawn with torch.randn
    unless no_noise."""

    def __init__(self, vertices, faces, bound=1.0, h_threshold=0.05, K=8, num_level=8, hidden_dim=32, geo_feat_dim=15, hidden_dim_color=64,
                 num_layers=2, num_layers_color=3, dir_degree=4, prob_model=False, vertex_normals=None, tbn=None, pred_normal=False, light_model=None, white_light=True,
                 use_specular=True):
        super().__init__()
        if light_model in ("SG", "Envmap"):
            raise NotImplementedError(f"CurvedField(light_model={light_model!r}): of the reference's light models only 'SH' (main.py's) is built here; "
                                      "the SG and Envmap models, imported environment maps and visibility probes are out of scope")
        if light_model not in (None, "SH"):
            raise ValueError(f"CurvedField: light_model is None (the static light model) or 'SH', but got {light_model!r}")
        pred_normal = pred_normal or light_model == "SH"  # the light head shades with the fine normal
        from ffmlp import FFMLP
        from gridencoder import GridEncoder
        from shencoder import SHEncoder

        self.bound, self.h_threshold, self.geo_feat_dim, self.multires, self.fc_weight = bound, h_threshold, geo_feat_dim, 12, 1.0
        self.projector = MeshProjector(vertices, faces, h_threshold=h_threshold, K=K, vertex_normals=vertex_normals, tbn=tbn)
        self.mesh_faces = np.array(torch.as_tensor(faces).cpu() if torch.is_tensor(faces) else faces, dtype=np.int64)  # (export_field: the mesh's unique edges)
        self._init_import_state()
        kw = dict(input_dim=3, num_levels=num_level, level_dim=2, base_resolution=512, log2_hashmap_size=19, desired_resolution=1024, gridtype="hash",
                  align_corners=True)
        self.encoder = GridEncoder_clustering(**kw)  # tools/map.py:563
        self.encoder_var = GridEncoder(**kw) if prob_model else None
        if prob_model:
            torch.nn.init.normal_(self.encoder_var.embeddings, std=1e-5)  # reset_parameters(std=1e-5), tools/map.py:566
        # pred_normal (the reference's default, tools/map.py:547, :585-588): the factorized fine-normal net.  Its consumer is the light model
        # (network_curvedfield.py:331-380): with light_model="SH" forward() shades with the fine normal; without a light model forward() keeps
        # the coarse normal (render_light_model False, :283) and the fine normal is what `embed(..., with_fine_normal=True)` / `fine_normal()` return
        self.normal_net = FactorizedNormalNet(x_dim=self.encoder.output_dim, z_dim=1 + 2 * self.multires) if pred_normal else None
        if pred_normal:
            self.normal_net.encoder.embeddings.data.uniform_(0, 1e-3)  # tools/map.py:588
        self.in_dim = self.encoder.output_dim + 1 + 2 * self.multires  # 16 + 25
        self.in_pad = (self.in_dim + 15) // 16 * 16
        self.sigma_net = FFMLP(input_dim=self.in_pad, output_dim=1 + geo_feat_dim, hidden_dim=hidden_dim, num_layers=num_layers)
        self.light_model = light_model
        if light_model == "SH":  # network_curvedfield.py:115-118, :207-208: the light head instead of the direction encoding and the colour MLP
            from .light import SHLightNet

            self.light_net = SHLightNet(input_dim=geo_feat_dim, white_light=white_light, use_specular=use_specular)  # (NeRFNetwork's keywords and defaults, :61)
            self.light_visual_mode, self.smooth_grad_weight = "Full", 1e-1
            self.shade_visibility = True  # network_curvedfield.py:86: under imported lighting in eval, one lighting per visibility probe (read by _forward_light only)
            self.encoder_dir = self.color_net = None
            return
        self.encoder_dir = SHEncoder(input_dim=3, degree=dir_degree)
        self.color_in = self.encoder_dir.output_dim + geo_feat_dim
        self.color_pad = (self.color_in + 15) // 16 * 16
        self.color_net = FFMLP(input_dim=self.color_pad, output_dim=3, hidden_dim=hidden_dim_color, num_layers=num_layers_color)

    # ---- an imported planar feature texture (MeshFeatureField.import_field, tools/map.py:912-927; the 'field' branch of its forward, :646-668) ----

    def _init_import_state(self):
        """The import state of MeshFeatureField as its constructor leaves it (tools/map.py:604-618): nothing imported."""
        self.imported, self.rescale, self.features_imported, self.bounds = False, False, None, None
        self.uv_utilize_rate, self.sdf_offset, self._import_version = 1.0, 0.0, 0
        # ... and of the 'shape' branch (:615-618): no second mesh, sdf_scale_factor 1, K_for_uv 5
        self.imported_type, self.shape_projector, self.shape_faces, self.shape_uvs, self.shape_face_uv = None, None, None, None, None
        self.sdf_scale_factor, self.K_for_uv, self.recommended_sdf_factor = 1.0, 5, None
        # ... and the maps of the `pred_normal` part (:920-923): none
        self.phi_embed_imported = self.local_tbn_imported = self.sample_tbn_ids_imported = self.sample_tbn_inv_imported = None
        self.frame_map_imported = self.sample_inv_rows_imported = None
        # ... and the new mesh's per-face frames (`new_tbn`, :542): none
        self.shape_face_tbn = None
        # ... and of the 'patch' branch (:929-937; the counter: network_curvedfield.py's patch_id): no patch, the counter at 0
        self.patch_id = 0
        self.patch_points = self.patch_normals = self.patch_phi_embed = self.patch_local_tbn = None
        self.patch_geom = self.patch_lit = self._patch_knn = None
        # ... and of the 'unhash' branch (:842-873): no fine mesh, no per-vertex rows
        self.unhash_tracer = self.unhash_vertices = self.unhash_faces = self.unhash_face_vertices = None

    def _lit(self):
        """A field whose forward reads a fine normal: the normal net, or a light model (which shades with it)."""
        return self.normal_net is not None or getattr(self, "light_model", None) is not None

    def _import_light_maps(self, H, W, phi_embed, local_tbn, sample_tbn, sample_tbn_ids, dev):
        """The four maps of MeshFeatureField.import_field's `pred_normal` part (tools/map.py:916-923), checked and brought to the device:
        phi_embed [H,W,8], local_tbn [H,W,9] or [H,W,3,3], sample_tbn [P,3,3] or [P,9] (inverted once, in fp32 on the host: :921),
        sample_tbn_ids [H,W] with every id in [0, P).  Beside them the two arrays the kernels read (include/nerftex_hip.h): the frame map
        [H,W,12] = [frame | id | 0 0] and the inverted patch frames padded to [P,12]."""
        def arr(a):
            return torch.as_tensor(np.asarray(a) if not torch.is_tensor(a) else a).detach().cpu()

        phi, loc, smp, ids = arr(phi_embed), arr(local_tbn), arr(sample_tbn), arr(sample_tbn_ids)
        if tuple(phi.shape) != (H, W, 8):
            raise ValueError(f"CurvedField.import_field: phi_embed is [H, W, 8] = {(H, W, 8)}, but got {tuple(phi.shape)}")
        if tuple(loc.shape) not in ((H, W, 9), (H, W, 3, 3)):
            raise ValueError(f"CurvedField.import_field: local_tbn is [H, W, 9] or [H, W, 3, 3] with H, W = {(H, W)}, but got {tuple(loc.shape)}")
        if not ((smp.dim() == 3 and tuple(smp.shape[1:]) == (3, 3)) or (smp.dim() == 2 and smp.shape[1] == 9)) or smp.shape[0] < 1:
            raise ValueError(f"CurvedField.import_field: sample_tbn is [P, 3, 3] or [P, 9] with P >= 1, but got {tuple(smp.shape)}")
        if tuple(ids.shape) != (H, W):
            raise ValueError(f"CurvedField.import_field: sample_tbn_ids is [H, W] = {(H, W)}, but got {tuple(ids.shape)}")
        P = int(smp.shape[0])
        ids = ids.to(torch.float32)
        whole = ids.long()  # (what the reference's `.long()` of the sampled float makes of it)
        if not bool(torch.isfinite(ids).all()) or int(whole.min()) < 0 or int(whole.max()) >= P or P > (1 << 24):
            raise ValueError(f"CurvedField.import_field: every id of sample_tbn_ids must lie in [0, P) = [0, {P}), P at most 2^24")
        loc = loc.to(torch.float32).reshape(H, W, 9)
        inv = torch.linalg.inv(smp.to(torch.float32).reshape(P, 3, 3))
        frame = torch.zeros(H, W, 12, dtype=torch.float32)
        frame[..., :9], frame[..., 9] = loc, ids
        rows = torch.zeros(P, 12, dtype=torch.float32)
        rows[:, :9] = inv.reshape(P, 9)
        self.phi_embed_imported = phi.to(device=dev, dtype=torch.float32).contiguous()
        self.local_tbn_imported, self.sample_tbn_ids_imported = loc.to(dev).contiguous(), ids.to(dev).contiguous()
        self.sample_tbn_inv_imported = inv.to(dev).contiguous()
        self.frame_map_imported, self.sample_inv_rows_imported = frame.to(dev).contiguous(), rows.to(dev).contiguous()

    def import_field(self, features, grid_gap, rescale=None, *, phi_embed=None, local_tbn=None, sample_tbn=None, sample_tbn_ids=None):
        """NeRFNetwork.import_field -> MeshFeatureField.import_field for a planar map (`mesh is None`, network_curvedfield.py:457-475):
        features [H, W, 16] (numpy or tensor, the array the reference receives, in its axis order) is kept channel-last in fp32 on the field's
        device, bounds = [grid_gap H / 2, grid_gap W / 2], `imported` is set and `rescale` TOGGLES as the reference's does (False at
        construction, so True after the first import: u, v = x, y scaled by uv_utilize_rate; False: x, y divided by the bounds); rescale=
        sets it instead.  From here on embed() / density() / forward() / infer() read the map and touch neither the projector nor the hash
        table, until switch_import().  The caller re-estimates the occupancy grid (Renderer.initialize_states), as the reference does.
        A field with the fine-normal net or a light model needs the four maps of the reference's `pred_normal` part as well (`_import_light_maps`,
        tools/map.py:670-675): phi_embed, local_tbn, sample_tbn, sample_tbn_ids; a field without a normal net takes none of them."""
        maps = (phi_embed, local_tbn, sample_tbn, sample_tbn_ids)
        if not self._lit() and any(m is not None for m in maps):
            raise ValueError("CurvedField.import_field: phi_embed, local_tbn, sample_tbn and sample_tbn_ids are read by the fine-normal net only; this field "
                             "has none and would ignore them")
        if self._lit() and any(m is not None for m in maps) and any(m is None for m in maps):
            raise ValueError("CurvedField.import_field: phi_embed, local_tbn, sample_tbn and sample_tbn_ids come together, all four or none")
        if self._lit() and phi_embed is None:
            raise NotImplementedError("CurvedField.import_field: a field with the fine-normal net or a light model would also need the imported phi_embed, "
                                      "local_tbn and sample_tbn maps (tools/map.py:670-675); only the static light model without a normal net imports here")
        f = torch.as_tensor(np.asarray(features) if not torch.is_tensor(features) else features).detach()
        if f.dim() != 3 or f.shape[-1] != self.encoder.output_dim or f.shape[0] < 1 or f.shape[1] < 1:
            raise ValueError(f"CurvedField.import_field: features are [H, W, {self.encoder.output_dim}], but got {tuple(f.shape)}")
        dev = self.sigma_net.weights.device
        H, W = int(f.shape[0]), int(f.shape[1])
        if self._lit():  # (before anything of the state changes: a refused import leaves the field as it was)
            self._import_light_maps(H, W, phi_embed, local_tbn, sample_tbn, sample_tbn_ids, dev)
        self.features_imported = f.to(device=dev, dtype=torch.float32).contiguous()
        self.bounds = [0.5 * float(grid_gap) * H, 0.5 * float(grid_gap) * W]
        self.imported, self.imported_type = True, "field"
        self.rescale = (not self.rescale) if rescale is None else bool(rescale)
        self._import_version += 1

    # ---- the imported map on a new UV-mapped mesh (NeRFNetwork.import_shape, network_curvedfield.py:494-501; the 'shape' branch, tools/map.py:693-700) ----

    def import_shape(self, vertices, faces, uvs, vertex_normals=None, normalize=True, *, new_tbn=None):
        """NeRFNetwork.import_shape -> MeshFeatureField.import_shape (tools/map.py:939-949) for a mesh given as arrays: vertices [V,3], faces
        [F,3], per-vertex uvs [V,2] (what `mesh.visual.uv` holds; the xatlas parametrisation of a mesh without UVs is not built here),
        vertex_normals [V,3] (default: area-weighted, the role of open3d's).  normalize: the reference's centring and scaling of the loaded mesh
        (`shape_preprocess`).  A second MeshProjector over the mesh, the per-face UV table, sdf_scale_factor = recommended_sdf_factor /
        bounds[0]; from here on embed() / density() / forward() / infer() project onto THIS mesh and read the imported map at the hit's
        interpolated UV, until switch_shape_feature() or switch_import().  The reference prints a message and returns when no map was
        imported; here that is a RuntimeError.  The caller re-estimates the occupancy grid (Renderer.initialize_states).
        new_tbn (a field with the fine-normal net or a light model needs it, and the four lit maps of import_field): the new mesh's per-face
        frames the fine normal is rotated by last (`new_tbn = self.tbn[face_idx]`, tools/map.py:542, :728-729) -- "uv": the reference's,
        `uv_face_frames` over the preprocessed mesh and UVs; or an array [F, 3, 3] taken as given (the role `tbn=` plays for the field's own
        mesh).  Kept as `shape_face_tbn` [F', 12] fp32 by ORIGINAL face id: 9 floats and three zeros per face, padded where `shape_face_uv`
        is.  A field without a normal net takes none.  A refused call changes nothing of the field's state."""
        if self.features_imported is None or self.imported_type not in ("field", "shape"):
            raise RuntimeError("CurvedField.import_shape: a feature map has to be imported first (import_field)")
        if new_tbn is not None and not self._lit():
            raise ValueError("CurvedField.import_shape: new_tbn is read by the fine-normal net only; this field has none and would ignore it")
        if new_tbn is not None and self.phi_embed_imported is None:
            raise RuntimeError("CurvedField.import_shape: a field with the fine-normal net or a light model reads the imported phi_embed, local_tbn, "
                               "sample_tbn and sample_tbn_ids maps on the new mesh too; import them first (import_field)")
        if new_tbn is None and (self.normal_net is not None or getattr(self, "light_model", None) is not None):
            raise NotImplementedError("CurvedField.import_shape: a field with the fine-normal net or a light model would also need the imported phi_embed, "
                                      "local_tbn and sample_tbn maps and the new mesh's frames (tools/map.py:702-707, :728-729); only the static light model "
                                      "without a normal net imports here")
        v, uv, face_uv, factor = shape_preprocess(vertices, faces, uvs, normalize=normalize)
        face_tbn = None
        if new_tbn is not None:  # (before anything of the state changes)
            if isinstance(new_tbn, str):
                if new_tbn != "uv":
                    raise ValueError(f"CurvedField.import_shape: new_tbn is \"uv\" or an array [F, 3, 3], but got {new_tbn!r}")
                try:
                    frames = uv_face_frames(shape_vertices(vertices, normalize), faces, uv)  # (the float64 vertices, as the reference's mesh holds them)
                except np.linalg.LinAlgError:  # (a UV edge matrix the 1e-3 rule does not mend: the reference stops here, too)
                    frames = np.full((len(face_uv), 3, 3), np.nan, np.float32)
            else:
                frames = np.asarray(new_tbn.detach().cpu() if torch.is_tensor(new_tbn) else new_tbn, dtype=np.float32)
            if tuple(frames.shape) != (len(face_uv), 3, 3):
                raise ValueError(f"CurvedField.import_shape: new_tbn holds one frame per face, [F, 3, 3] = {(len(face_uv), 3, 3)}, but got {tuple(frames.shape)}")
            if not np.isfinite(frames).all():
                raise ValueError("CurvedField.import_shape: every frame of new_tbn must be finite (a face without area, or UV corners that coincide?)")
            face_tbn = np.zeros((len(face_uv) + (8 if len(face_uv) <= 8 else 0), 12), np.float32)  # (padded as the UV table below)
            face_tbn[:len(face_uv), :9] = frames.reshape(-1, 9)
        dev = self.sigma_net.weights.device
        self.shape_projector = MeshProjector(v, np.asarray(faces), h_threshold=self.h_threshold, K=self.K_for_uv, vertex_normals=vertex_normals).to(dev)
        self.shape_faces = torch.as_tensor(np.asarray(faces).astype(np.int64)).to(dev)
        self.shape_uvs = torch.from_numpy(uv).to(dev)
        if len(face_uv) <= 8:  # (RayTracer pads so small a mesh with 8 far-away faces: the table follows the tracer's face count, the rows are never hit)
            face_uv = np.concatenate([face_uv, np.zeros((8, 6), np.float32)], 0)
        self.shape_face_uv = torch.from_numpy(face_uv).to(dev).contiguous()
        self.shape_face_tbn = None if face_tbn is None else torch.from_numpy(face_tbn).to(dev).contiguous()
        self.recommended_sdf_factor = factor
        self.sdf_scale_factor = factor / self.bounds[0]
        self.imported, self.imported_type = True, "shape"
        self._import_version += 1

    def switch_shape_feature(self):
        """network_curvedfield.py:508-517: between the planar map ('field') and the map on the imported mesh ('shape')."""
        if self.imported_type == "field" and self.shape_projector is not None:
            self.imported_type = "shape"
        elif self.imported_type == "shape":
            self.imported_type = "field"
        else:
            raise RuntimeError("CurvedField.switch_shape_feature: no shape has been imported")
        self._import_version += 1

    def set_k_for_uv(self, k_for_uv=5):
        self.K_for_uv = int(k_for_uv)
        self._import_version += 1

    def set_sdf_factor(self, sdf_factor=1.0):
        self.sdf_scale_factor = float(sdf_factor)
        self._import_version += 1

    def _shape_active(self):
        return bool(getattr(self, "imported", False)) and getattr(self, "imported_type", None) == "shape"

    def _shape_scalars(self):
        """(K, sdf_scale, sdf_offset, uv_rate, h_threshold) of nerftex_shape_lookup for the state as it is.  The scale is the reference's
        max(1e-5, sdf_scale_factor / uv_utilize_rate) in Python double, rounded to fp32: what its CPU division of a tensor by a Python float does."""
        scale = float(np.float32(max(1e-5, float(self.sdf_scale_factor) / float(self.uv_utilize_rate))))
        K = max(1, min(int(self.K_for_uv), int(self.shape_projector.mesh_vertices.shape[0])))
        return K, scale, float(self.sdf_offset), float(self.uv_utilize_rate), float(self.h_threshold)

    # what the lookup kernels write per sample, by name: (trailing shape, dtype)
    _LOOKUP_BUFFERS = {"p_uv": ((2,), torch.float32), "sdf": ((), torch.float32), "mask": ((), torch.uint8), "normal": ((3,), torch.float32),
                       "face": ((), torch.int64), "xin": ((48,), torch.float16), "phi": ((8,), torch.float32), "ids": ((), torch.int32),
                       "frame": ((9,), torch.float32), "idx": ((8,), torch.int32), "dis": ((8,), torch.float32), "weights": ((8,), torch.float32), "bary": ((3,), torch.float32)}

    @classmethod
    def _lookup_buffers(cls, x, *names):
        """The lookup wrappers' one allocator: an uninitialised [N, ...] output on x's device per name of `_LOOKUP_BUFFERS`."""
        return [torch.empty(x.shape[0], *cls._LOOKUP_BUFFERS[n][0], dtype=cls._LOOKUP_BUFFERS[n][1], device=x.device) for n in names]

    def _shape_query(self, x, neighbours):
        """What the two shape lookups start from: the samples as the kernels read them, their neighbours on the imported mesh (default: the
        library's search) and the arguments the two entries share, the tracer .. the UV table's face count."""
        x, p, uv = x.detach().float().contiguous(), self.shape_projector, self.shape_face_uv
        idx, dis = p.knn(x, self._shape_scalars()[0]) if neighbours is None else neighbours
        idx, dis = idx.int().contiguous(), dis.float().contiguous()
        return x, (p.tracer._handle, ptr(x), ptr(idx), ptr(dis), x.shape[0], idx.shape[1], ptr(p.mesh_vertices), ptr(p.vertex_normals),
                   p.mesh_vertices.shape[0], ptr(uv), uv.shape[0]), (idx, dis)

    @torch.no_grad()
    def _shape_lookup(self, x, neighbours=None):
        """nerftex_knn_query + nerftex_shape_lookup: -> p_uv [N,2], sdf [N], h_mask [N] bool, normal [N,3] (raw), face [N], xin [N,48] half."""
        from nerftex_hip import check, lib, stream

        x, head, _keep = self._shape_query(x, neighbours)
        f, (_, scale, off, rate, h) = self.features_imported, self._shape_scalars()
        p_uv, sdf, mask, normal, face, xin = out = self._lookup_buffers(x, "p_uv", "sdf", "mask", "normal", "face", "xin")
        check(lib.nerftex_shape_lookup(*head, ptr(f), f.shape[0], f.shape[1], scale, off, rate, h, int(self.multires), *map(ptr, out), stream()))
        return p_uv, sdf, mask.bool(), normal, face, xin

    def _shape_embed_reference(self, x, neighbours=None, details=False):
        """The 'shape' branch op by op, the reference's expressions (tools/map.py:695-700 over :454-543 and :85-93) over RayTracer.trace:
        -> embed [N,41] fp32, normal_coarse, h_mask (details: + p_uv, sdf, the raw normal, face).  The divisor is a 0-d tensor, as in
        `_import_embed_reference`.  neighbours: a neighbour list from elsewhere (default: the library's search over the imported mesh)."""
        x = x.float()
        p = self.shape_projector
        K, scale, off, rate, h = self._shape_scalars()
        idx, dis = p.knn(x, K) if neighbours is None else neighbours
        normal = shape_knn_normal(x, idx, dis, p.mesh_vertices, p.vertex_normals)
        p1, _, d1, f1 = p.tracer.trace(x, normal)
        p2, _, d2, f2 = p.tracer.trace(x, -normal)
        cond = d1 < d2
        sdf = torch.where(cond, -d1, d2).unsqueeze(-1) / torch.tensor(scale, dtype=torch.float32, device=x.device) - off
        p_sur = torch.where(cond.unsqueeze(-1), p1, p2)
        face = torch.where(cond, f1, f2)
        h_mask = (sdf.abs() < min(9.5, h)).squeeze(-1)
        face_mask = face == -1
        h_mask = torch.logical_and(h_mask, torch.logical_not(face_mask))
        face0 = torch.where(face_mask, torch.zeros_like(face), face)
        vertex_idx = self.shape_faces[face0]
        bary = points_to_barycentric(p.mesh_vertices[vertex_idx], p_sur)
        uv = (self.shape_uvs[vertex_idx] * bary.unsqueeze(-1)).sum(-2)
        p_uv = uv * rate
        embed = torch.cat([self._sample_map(self.features_imported, p_uv).permute(1, 0), freq_encode(sdf, self.multires)], dim=-1)
        normal_coarse = normal / (normal.norm(dim=-1, keepdim=True) + 1e-5)
        if details:
            return embed, normal_coarse, h_mask, p_uv, sdf[..., 0], normal, face
        return embed, normal_coarse, h_mask

    def _shape_light_fused(self, x):
        """_import_light_fused() for the maps on the imported mesh: the lit shape lookup serves the default shapes under fp16 autocast, once the
        four lit maps and the new mesh's frames are there."""
        return (self._lit() and self._shape_active() and self.phi_embed_imported is not None and self.shape_face_tbn is not None
                and self._sigma_fused(x))

    @torch.no_grad()
    def _shape_light_lookup(self, x, neighbours=None):
        """nerftex_knn_query + nerftex_shape_light_lookup: -> p_uv [N,2], sdf [N], h_mask [N] bool, normal [N,3] (raw), face [N], xin [N,48] half,
        phi [N,8] fp32, id [N] int32, local_tbn, sample_tbn_inv, new_tbn [N,3,3]."""
        from nerftex_hip import check, lib, stream

        x, head, _keep = self._shape_query(x, neighbours)
        f, rows, frames, (_, scale, off, rate, h) = self.features_imported, self.sample_inv_rows_imported, self.shape_face_tbn, self._shape_scalars()
        out = self._lookup_buffers(x, "p_uv", "sdf", "mask", "normal", "face", "xin", "phi", "ids", "frame", "frame", "frame")
        check(lib.nerftex_shape_light_lookup(*head, ptr(frames), frames.shape[0], ptr(f), ptr(self.phi_embed_imported), ptr(self.frame_map_imported), ptr(rows),
                                             f.shape[0], f.shape[1], rows.shape[0], scale, off, rate, h, int(self.multires), *map(ptr, out), stream()))
        p_uv, sdf, mask, normal, face, xin, phi, ids, *tbn = out
        return (p_uv, sdf, mask.bool(), normal, face, xin, phi, ids) + tuple(t.view(x.shape[0], 3, 3) for t in tbn)

    def _shape_light_embed_reference(self, x, neighbours=None, details=False):
        """The 'shape' branch with `pred_normal` op by op (tools/map.py:693-707, :722-730): `_shape_embed_reference`'s expressions, the four
        grid_sample calls of `_import_light_embed_reference` at its p_uv, the hit face's frame (face -1 reads face 0), the normal net and the
        three rotations.  -> embed [N,41] fp32, normal_coarse, h_mask, normal_fine (details: + p_uv, sdf, face, the sampled phi_embed,
        local_tbn, id, sample_tbn_inv rows and new_tbn)."""
        embed, normal_coarse, h_mask, p_uv, sdf, _, face = self._shape_embed_reference(x, neighbours=neighbours, details=True)
        phi, local_tbn, ids, sample_tbn_inv = self._lit_maps_reference(p_uv)
        face0 = torch.where(face == -1, torch.zeros_like(face), face)
        new_tbn = self.shape_face_tbn.to(p_uv.device)[face0, :9].reshape(-1, 3, 3)
        x_embed, z_embed = embed[:, :self.encoder.output_dim], embed[:, self.encoder.output_dim:]
        local = self.normal_net(phi_embed=phi, z_embed=z_embed, x_embed=x_embed)
        fine = self._rotate_fine(local, local_tbn, sample_tbn_inv, new_tbn)
        if details:
            return embed, normal_coarse, h_mask, fine, p_uv, sdf, face, phi, local_tbn, ids, sample_tbn_inv, new_tbn
        return embed, normal_coarse, h_mask, fine

    # ---- an exported feature patch (NeRFNetwork.import_patch, network_curvedfield.py:477-492; the 'patch' branch, tools/map.py:676-692) ----

    def import_patch(self, field_dict=None, patch_id=None, *, features=..., points=..., normals=..., local_tbn=None, phi_embed=None):
        """NeRFNetwork.import_patch -> MeshFeatureField.import_patch (tools/map.py:929-937): ONE patch of an export as an oriented point cloud the
        samples are resampled from (8 nearest points, the reference's dual-distance weights) -- what shows an exported patch before any synthesis.
        field_dict: what `export_field` returns (`patches`, `patch_coors`, `patch_norms`, `patch_local_tbn`, `patch_phi_embed`); patch_id picks
        the patch, None follows the reference's counter `self.patch_id` (taken modulo the patch count, advanced after the import; an explicit
        patch_id leaves the counter alone).  Or explicit arrays (keywords): features [V,16], points [V,3], normals [3] (the patch's one normal,
        as the reference stores it at every point) or [V,3]; a field with the fine-normal net or a light model needs local_tbn [V,9] or
        [V,3,3] and phi_embed [V,8] as well, a field without takes neither (a field_dict's are not read there).  V >= 8.
        From here on embed() / density() / forward() / infer() read the patch and touch neither the projector nor the hash table, until
        switch_import() or the next import_field() / import_patch().  The caller re-estimates the occupancy grid
        (Renderer.initialize_states), as the reference does.  A refused call changes nothing of the field's state."""
        explicit = (features, points, normals)
        if field_dict is not None:
            if any(a is not ... for a in explicit) or local_tbn is not None or phi_embed is not None:
                raise ValueError("CurvedField.import_patch: a field_dict or explicit arrays, not both")
            missing = [k for k in ("patches", "patch_coors", "patch_norms", "patch_local_tbn", "patch_phi_embed") if k not in field_dict]
            if missing:
                raise ValueError(f"CurvedField.import_patch: the field_dict lacks {missing} (it is what export_field returns)")
            count = int(np.asarray(field_dict["patch_coors"]).shape[0])
            if count < 1:
                raise ValueError("CurvedField.import_patch: the field_dict holds no patch")
            pid = self.patch_id % count if patch_id is None else int(patch_id)
            if not 0 <= pid < count:
                raise ValueError(f"CurvedField.import_patch: patch_id lies in [0, {count}), but got {patch_id}")
            features = np.asarray(field_dict["patches"][pid])
            features = features.reshape(-1, features.shape[-1])
            points, normals = np.asarray(field_dict["patch_coors"][pid]).reshape(-1, 3), np.asarray(field_dict["patch_norms"][pid])
            if self._lit():  # (a field without a normal net does not read them: the reference hands them over and ignores them)
                local_tbn = np.asarray(field_dict["patch_local_tbn"][pid]).reshape(-1, 9)
                phi = field_dict["patch_phi_embed"]
                phi_embed = None if phi is None else np.asarray(phi[pid]).reshape(-1, np.asarray(phi[pid]).shape[-1])
                local_tbn = None if phi is None else local_tbn  # (an export of a field without a normal net: refused below, as a patch without either)
        elif any(a is ... for a in explicit):
            raise ValueError("CurvedField.import_patch: a field_dict (what export_field returns), or features=, points= and normals=")
        elif patch_id is not None:
            raise ValueError("CurvedField.import_patch: patch_id picks a patch of a field_dict; explicit arrays are one patch")
        if not self._lit() and (local_tbn is not None or phi_embed is not None):
            raise ValueError("CurvedField.import_patch: local_tbn and phi_embed are read by the fine-normal net only; this field has none and would ignore them")
        if self._lit() and (local_tbn is None) != (phi_embed is None):
            raise ValueError("CurvedField.import_patch: local_tbn and phi_embed come together, both or none")
        if self._lit() and phi_embed is None:
            raise NotImplementedError("CurvedField.import_patch: a field with the fine-normal net or a light model would also need the patch's local_tbn and "
                                      "phi_embed (tools/map.py:687-692); only the static light model without a normal net imports without them")

        def arr(a):
            return torch.as_tensor(np.asarray(a) if not torch.is_tensor(a) else a).detach().cpu().to(torch.float32)

        f, p, n = arr(features), arr(points), arr(normals)
        if f.dim() != 2 or f.shape[1] != self.encoder.output_dim or f.shape[0] < 8:
            raise ValueError(f"CurvedField.import_patch: features are [V, {self.encoder.output_dim}] with V >= 8 (a sample reads its 8 nearest points), "
                             f"but got {tuple(f.shape)}")
        V = int(f.shape[0])
        if tuple(p.shape) != (V, 3) or not bool(torch.isfinite(p).all()):
            raise ValueError(f"CurvedField.import_patch: points are [V, 3] = {(V, 3)} and finite, but got {tuple(p.shape)}")
        if tuple(n.shape) not in ((3,), (V, 3)) or not bool(torch.isfinite(n).all()):
            raise ValueError(f"CurvedField.import_patch: normals are [3] or [V, 3] = {(V, 3)} and finite, but got {tuple(n.shape)}")
        n = n.expand(V, 3).contiguous()  # (:485-486: the one normal at every point)
        geom = torch.zeros(V, 8, dtype=torch.float32)
        geom[:, :3], geom[:, 4:7] = p, n
        lit = phi = loc = None
        if self._lit():
            phi, loc = arr(phi_embed), arr(local_tbn)
            if tuple(phi.shape) != (V, 8):
                raise ValueError(f"CurvedField.import_patch: phi_embed is [V, 8] = {(V, 8)}, but got {tuple(phi.shape)}")
            if tuple(loc.shape) not in ((V, 9), (V, 3, 3)):
                raise ValueError(f"CurvedField.import_patch: local_tbn is [V, 9] or [V, 3, 3] with V = {V}, but got {tuple(loc.shape)}")
            loc = loc.reshape(V, 9)
            lit = torch.zeros(V, 20, dtype=torch.float32)
            lit[:, :8], lit[:, 8:17] = phi, loc
        dev = self.sigma_net.weights.device
        grid = PointGrid(p.numpy(), dev) if dev.type == "cuda" else None  # (the last thing that can fail; without a device the op-by-op route searches by brute force)
        self.features_imported = f.to(dev).contiguous()
        self.patch_points, self.patch_normals, self.patch_geom = p.to(dev).contiguous(), n.to(dev), geom.to(dev).contiguous()
        self.patch_phi_embed, self.patch_local_tbn = (None, None) if lit is None else (phi.to(dev).contiguous(), loc.to(dev).contiguous())
        self.patch_lit = None if lit is None else lit.to(dev).contiguous()
        self._patch_knn = grid
        self.imported, self.imported_type = True, "patch"
        if field_dict is not None and patch_id is None:
            self.patch_id = pid + 1
        self._import_version += 1

    def _patch_active(self):
        return bool(getattr(self, "imported", False)) and getattr(self, "imported_type", None) == "patch"

    def _patch_fused(self, x):
        """Whether the patch lookup kernel serves this call: a neighbour grid on the device, the default shapes under fp16 autocast without the
        probabilistic table (the static light model: unless `fused_glue` is off)."""
        return (self._patch_active() and self._patch_knn is not None and self._sigma_fused(x) and (self._lit() or getattr(self, "fused_glue", True))
                and self._on_device_of(x, self.features_imported, self.patch_geom))

    @torch.no_grad()
    def _patch_lookup(self, x, lit=False):
        """nerftex_patch_lookup (lit: nerftex_patch_light_lookup): -> sdf [N], h_mask [N] bool, normal [N,3] (raw), xin [N,48] half, idx [N,8],
        dis [N,8] (the search's), weights [N,8] (+ lit: phi [N,8] fp32, local_tbn [N,3,3])."""
        from nerftex_hip import check, lib, stream

        x = x.detach().float().contiguous()
        N, f = x.shape[0], self.features_imported
        sdf, mask, normal, xin, idx, dis, weights = out = self._lookup_buffers(x, "sdf", "mask", "normal", "xin", "idx", "dis", "weights")
        head = (self._patch_knn.value, ptr(x), ptr(self.patch_geom), ptr(f))
        tail = (f.shape[0], float(self.h_threshold), int(self.multires), N, *map(ptr, out))
        if not lit:
            check(lib.nerftex_patch_lookup(*head, *tail, stream()))
            return sdf, mask.bool(), normal, xin, idx, dis, weights
        phi, tbn = self._lookup_buffers(x, "phi", "frame")
        check(lib.nerftex_patch_light_lookup(*head, ptr(self.patch_lit), *tail, ptr(phi), ptr(tbn), stream()))
        return sdf, mask.bool(), normal, xin, idx, dis, weights, phi, tbn.view(N, 3, 3)

    def _patch_neighbours(self, x):
        """The 8 nearest patch points of every sample (idx, Euclidean distances, ascending): the library's exact search where the grid is, brute
        force elsewhere."""
        from nerftex_hip import check, lib, ptr, stream

        if x.is_cuda and self._patch_knn is not None:
            x = x.contiguous()
            idx = torch.empty(x.shape[0], 8, dtype=torch.int32, device=x.device)
            dis = torch.empty(x.shape[0], 8, dtype=torch.float32, device=x.device)
            check(lib.nerftex_knn_query(self._patch_knn.value, ptr(x), x.shape[0], 8, ptr(idx), ptr(dis), stream()))
            return idx, dis
        points, idx, dis = self.patch_points.to(x.device), [], []
        for a in range(0, x.shape[0], 8192):  # (differences, not the matrix-product form of cdist: that one loses half the digits of a distance)
            d = torch.cdist(x[a:a + 8192], points, compute_mode="donot_use_mm_for_euclid_dist")
            dd, ii = torch.topk(d, 8, dim=-1, largest=False, sorted=True)
            idx.append(ii.int())
            dis.append(dd)
        return torch.cat(idx).contiguous(), torch.cat(dis).contiguous()

    def _patch_embed_reference(self, x, neighbours=None, with_fine_normal=False, details=False):
        """The 'patch' branch op by op, the reference's expressions line by line (tools/map.py:678-692 over weighted_project(weighting='DualD'),
        :435-452, and knn(use_dir_vec=False, direct_above_check=True, direct_above_threshold=1., weighting='Shepard'), :454-501):
        -> embed [N,41] fp32, normal_coarse, h_mask (+ normal_fine with with_fine_normal; details: + sdf, the raw normal, idx, dis after the
        direct-above select, weights, and with the fine normal the weighted phi_embed and local_tbn).  neighbours: a neighbour list from
        elsewhere (default: `_patch_neighbours`)."""
        x = x.float()
        points, vertex_normals = self.patch_points.to(x.device), self.patch_normals.to(x.device)
        idx, dis = self._patch_neighbours(x) if neighbours is None else neighbours
        idx = idx.long()
        # knn(), :459-471
        normals = vertex_normals[idx]
        dir_vec_ori = x.unsqueeze(-2) - points[idx]
        dir_vec = dir_vec_ori / (dir_vec_ori.norm(dim=-1, keepdim=True) + 1e-5)
        p2n_dis_min = 2 * torch.cross(normals, dir_vec, dim=-1).norm(dim=-1).min(dim=-1)[0]
        direct_above_mask = (p2n_dis_min < 1.0).reshape([-1, 1])
        dis = torch.where(direct_above_mask, dis, 1e5 * torch.ones_like(dis))
        dir_vec_ori = torch.where(direct_above_mask.unsqueeze(-1), dir_vec_ori, 1e5 * torch.ones_like(dir_vec_ori))
        # :486-499
        weights = 1 / (dis + 1e-7)
        weights = weights / torch.sum(weights, dim=-1, keepdim=True)
        normals = normals / (normals.norm(dim=-1, keepdim=True) + 1e-5)
        normal = (normals * weights.unsqueeze(-1)).sum(-2)
        normal = normal / (normal.norm(dim=-1, keepdim=True) + 1e-5)
        # weighted_project(), :437-448 (sdf_scale 1, sdf_offset 0: neither setter reaches this branch)
        sdfs = (dir_vec_ori * normal.unsqueeze(1)).sum(-1)
        dist2D_sq = ((dir_vec_ori - sdfs.unsqueeze(-1) * normal.unsqueeze(1)) ** 2).norm(dim=-1)
        dk = dist2D_sq.max(dim=-1, keepdim=True)[0]
        d1 = dist2D_sq.min(dim=-1, keepdim=True)[0]
        weights = (dk - dist2D_sq) / (dk - d1 + 1e-5) * (dk + d1) / (dk + dist2D_sq)
        weights = weights / (weights.sum(-1, keepdim=True) + 1e-5)
        sdf = (sdfs * weights).sum(-1, keepdim=True) / max(1e-5, 1.0) - 0.0
        # forward(), :679-685
        x_embed = (weights.unsqueeze(-1) * self.features_imported.to(x.device)[idx]).sum(-2)
        z_embed = freq_encode(sdf, self.multires)
        h_mask = sdf[..., 0].abs() < self.h_threshold
        h_mask = torch.logical_and(h_mask, dis.min(dim=-1)[0] < self.h_threshold)
        embed = torch.cat([x_embed, z_embed], dim=-1)
        normal_coarse = normal / (normal.norm(dim=-1, keepdim=True) + 1e-5)  # :720
        out = (embed, normal_coarse, h_mask)
        more = (sdf[..., 0], normal, idx, dis, weights)
        if with_fine_normal:  # :687-692, :722-730: ONE rotation, by the weighted local_tbn
            phi = (weights.unsqueeze(-1) * self.patch_phi_embed.to(x.device)[idx]).sum(-2)
            local_tbn = (weights.unsqueeze(-1).unsqueeze(-1) * self.patch_local_tbn.to(x.device)[idx].reshape(*idx.shape, 3, 3)).sum(-3)
            local = self.normal_net(phi_embed=phi, z_embed=z_embed, x_embed=x_embed)
            out += (self._rotate_fine(local, local_tbn),)
            more += (phi, local_tbn)
        return out + more if details else out

    # ---- the field baked onto the vertices of a fine mesh (MeshFeatureField.unhash / import_unhash_vertices, tools/map.py:842-873; the 'unhash' branch, :708-714) ----

    def _unhash_refuse_lit(self, who):
        if self._lit():
            raise NotImplementedError(f"CurvedField.{who}: the reference's unhash branch does not run on a field with the fine-normal net or a light model "
                                      "(its query_tbn returns a tuple the rotation of tools/map.py:725 cannot take); only the static light model without a "
                                      "normal net takes this import")

    def _unhash_mesh(self, who, vertices, faces):
        """The fine mesh of an unhash import, checked: -> (vertices [V',3] fp32, faces [F',3] int64) as numpy arrays.  A field with the fine-normal net
        or a light model is refused here, before any work."""
        self._unhash_refuse_lit(who)
        v = np.asarray(vertices.detach().cpu() if torch.is_tensor(vertices) else vertices)
        f = np.asarray(faces.detach().cpu() if torch.is_tensor(faces) else faces)
        if v.ndim != 2 or v.shape[1] != 3 or v.shape[0] < 1 or f.ndim != 2 or f.shape[1] != 3 or f.shape[0] < 1:
            raise ValueError(f"CurvedField.{who}: vertices are [V', 3] and faces [F', 3], but got {tuple(v.shape)} and {tuple(f.shape)}")
        if not np.issubdtype(f.dtype, np.integer) or f.min() < 0 or f.max() >= v.shape[0]:
            raise ValueError(f"CurvedField.{who}: every face indexes into the {v.shape[0]} fine vertices with whole numbers")
        if not np.issubdtype(v.dtype, np.number) or not np.isfinite(v.astype(np.float64)).all():
            raise ValueError(f"CurvedField.{who}: every fine vertex must be finite")
        return np.ascontiguousarray(v, dtype=np.float32), f.astype(np.int64)

    def _unhash_state(self, who, vertices, faces, features, sdf_factor):
        """The checked state of an unhash import, brought to the device -- everything that can fail, before anything of the field changes: fine
        vertices [V',3] fp32, faces [F',3], features [V',16] fp32 (a device tensor is kept as it is), the fine mesh's tracer (the tracer ALONE: the
        neighbour grid of a full MeshProjector over 5e5 points would never be read) and the [F',3] int32 table of corner vertex ids by original
        face id, padded where the tracer pads a mesh of <= 8 faces (`shape_face_uv` is padded so)."""
        v, f = self._unhash_mesh(who, vertices, faces)
        dev = self.sigma_net.weights.device
        feats = features.detach() if torch.is_tensor(features) else torch.as_tensor(np.asarray(features))
        if tuple(feats.shape) != (v.shape[0], self.encoder.output_dim):
            raise ValueError(f"CurvedField.{who}: features are [V', {self.encoder.output_dim}] = {(v.shape[0], self.encoder.output_dim)}, but got {tuple(feats.shape)}")
        feats = feats.to(device=dev, dtype=torch.float32).contiguous()
        if not bool(torch.isfinite(feats).all()):
            raise ValueError(f"CurvedField.{who}: every feature must be finite")
        factor = float(sdf_factor)
        if not np.isfinite(factor):
            raise ValueError(f"CurvedField.{who}: sdf_factor must be finite, but got {sdf_factor!r}")
        table = f.astype(np.int32)
        if len(table) <= 8:  # (RayTracer pads so small a mesh with 8 far-away faces: the table follows the tracer's face count, the rows are never hit)
            table = np.concatenate([table, np.zeros((8, 3), np.int32)], 0)
        with torch.cuda.device(dev):
            tracer = RayTracer(v, f)
        return (tracer, torch.from_numpy(v).to(dev), torch.from_numpy(f.astype(np.int64)).to(dev), torch.from_numpy(table).to(dev).contiguous(), feats, factor)

    def _set_unhash(self, state):
        self.unhash_tracer, self.unhash_vertices, self.unhash_faces, self.unhash_face_vertices, self.features_imported, self.sdf_scale_factor = state
        self.imported, self.imported_type = True, "unhash"
        self._import_version += 1

    @torch.no_grad()
    def unhash(self, min_vnum=5e5, *, mesh=None):
        """MeshFeatureField.unhash (tools/map.py:842-860), the GUI's "unhash" button: the field's own mesh subdivided at its edge midpoints until it
        has at least min_vnum vertices (`subdivide.subdivide_until`; mesh=(vertices, faces): a fine mesh taken as given instead), the field's own hash
        table looked up at every fine vertex -- `encoder(vertices, bound)` in fp32, outside autocast --, and from here on embed() / density() /
        forward() / infer() interpolate these per-vertex rows at the hit on the FINE mesh along the normal of the field's OWN mesh, until
        switch_import() or the next import.  sdf_scale_factor stays what it is.  -> dict(vertices=, faces=, features=, sdf_factor=): numpy arrays,
        what `import_unhash_vertices` takes.  The caller re-estimates the occupancy grid (Renderer.initialize_states).  A refused call changes
        nothing of the field's state."""
        if mesh is None:
            self._unhash_refuse_lit("unhash")  # (before the subdivision)
            mesh = subdivide_until(self.projector.mesh_vertices.detach().cpu().numpy(), self.mesh_faces, min_vnum)
        v, f = self._unhash_mesh("unhash", *mesh)
        dev = self.sigma_net.weights.device
        with torch.autocast("cuda", enabled=False):
            feats = self.encoder(torch.from_numpy(v).to(dev), bound=self.bound).float()
        state = self._unhash_state("unhash", v, f, feats, self.sdf_scale_factor)
        self._set_unhash(state)
        return dict(vertices=v, faces=state[2].cpu().numpy(), features=feats.cpu().numpy(), sdf_factor=float(self.sdf_scale_factor))

    def import_unhash_vertices(self, vertices, faces, features, sdf_factor=1.0):
        """MeshFeatureField.import_unhash_vertices (tools/map.py:862-873) from arrays (the reference unpickles a mesh from an .npz, which is not read
        here): fine vertices [V',3], faces [F',3] indexing into them, features [V',16], everything finite; sdf_scale_factor = sdf_factor.  The state
        `unhash()` sets, from what it returned or from a synthesis on the curved surface.  A refused call changes nothing of the field's state."""
        self._set_unhash(self._unhash_state("import_unhash_vertices", vertices, faces, features, sdf_factor))

    def _unhash_active(self):
        return bool(getattr(self, "imported", False)) and getattr(self, "imported_type", None) == "unhash"

    def _unhash_scalars(self):
        """(K, sdf_scale, sdf_offset, h_threshold) of nerftex_vertex_lookup for the state as it is: K is knn()'s default 8 (tools/map.py:709 passes
        none) clamped to the field's own vertex count; the scale is the reference's max(1e-5, sdf_scale_factor) in Python double, rounded to fp32."""
        scale = float(np.float32(max(1e-5, float(self.sdf_scale_factor))))
        return max(1, min(8, int(self.projector.mesh_vertices.shape[0]))), scale, float(self.sdf_offset), float(self.h_threshold)

    def _unhash_fused(self, x):
        """Whether the vertex lookup kernel serves this call: the default shapes under fp16 autocast without the probabilistic table, unless
        `fused_glue` is off, everything on the device of x."""
        return (self._unhash_active() and self._sigma_fused(x) and getattr(self, "fused_glue", True)
                and self._on_device_of(x, self.features_imported, self.unhash_vertices, self.unhash_face_vertices, self.projector.mesh_vertices))

    @torch.no_grad()
    def _unhash_lookup(self, x, neighbours=None):
        """nerftex_knn_query (the field's own grid) + nerftex_vertex_lookup: -> sdf [N], h_mask [N] bool, normal [N,3] (raw), face [N], bary [N,3],
        xin [N,48] half."""
        from nerftex_hip import check, lib, stream

        x, p = x.detach().float().contiguous(), self.projector
        K, scale, off, h = self._unhash_scalars()
        idx, dis = p.knn(x, K) if neighbours is None else neighbours
        idx, dis = idx.int().contiguous(), dis.float().contiguous()
        fv, table, f = self.unhash_vertices, self.unhash_face_vertices, self.features_imported
        sdf, mask, normal, face, bary, xin = out = self._lookup_buffers(x, "sdf", "mask", "normal", "face", "bary", "xin")
        check(lib.nerftex_vertex_lookup(self.unhash_tracer._handle, ptr(x), ptr(idx), ptr(dis), x.shape[0], idx.shape[1], ptr(p.mesh_vertices), ptr(p.vertex_normals),
                                        p.mesh_vertices.shape[0], 0.05, ptr(fv), fv.shape[0], ptr(table), table.shape[0], ptr(f), scale, off, h, int(self.multires),
                                        *map(ptr, out), stream()))
        return sdf, mask.bool(), normal, face, bary, xin

    def _unhash_embed_reference(self, x, neighbours=None, details=False):
        """The 'unhash' branch op by op, the reference's expressions (tools/map.py:708-714 over knn(), :454-501, barycentric_mapping, :503-528, and
        :85-93) over RayTracer.trace: -> embed [N,41] fp32, normal_coarse, h_mask (details: + sdf, the raw normal, face, bary).  The divisor is a
        0-d tensor, as in `_shape_embed_reference`.  neighbours: a neighbour list from elsewhere (default: the library's search over the field's
        own mesh)."""
        x = x.float()
        p = self.projector
        K, scale, off, h = self._unhash_scalars()
        idx, dis = p.knn(x, K) if neighbours is None else neighbours
        normal = p.knn_normal(x, idx, dis)
        p1, _, d1, f1 = self.unhash_tracer.trace(x, normal)
        p2, _, d2, f2 = self.unhash_tracer.trace(x, -normal)
        cond = d1 < d2
        sdf = torch.where(cond, -d1, d2).unsqueeze(-1) / torch.tensor(scale, dtype=torch.float32, device=x.device) - off
        p_sur = torch.where(cond.unsqueeze(-1), p1, p2)
        face = torch.where(cond, f1, f2)
        h_mask = (sdf.abs() < min(9.5, h)).squeeze(-1)
        face_mask = face == -1
        h_mask = torch.logical_and(h_mask, torch.logical_not(face_mask))
        face0 = torch.where(face_mask, torch.zeros_like(face), face)
        vertex_idx = self.unhash_faces[face0]
        bary = points_to_barycentric(self.unhash_vertices[vertex_idx], p_sur)
        x_embed = (self.features_imported[vertex_idx] * bary.unsqueeze(-1)).sum(-2)
        embed = torch.cat([x_embed, freq_encode(sdf, self.multires)], dim=-1)
        normal_coarse = normal / (normal.norm(dim=-1, keepdim=True) + 1e-5)
        if details:
            return embed, normal_coarse, h_mask, sdf[..., 0], normal, face, bary
        return embed, normal_coarse, h_mask

    # ---- the trained field exported as texture patches (NeRFNetwork.export_field -> MeshFeatureField.sample_patches, tools/map.py:951-1128) ----

    def export_field(self, sample_points, sample_normals, *, scan_points=None, first_component=None, grid_gap=None, pattern_rate=1 / 50, patch_size=128,
                     max_patch_num=2000, sample_mesh=None, record_rays=False, patches_per_chunk=None, fused=True):
        """The reference's non-trimesh path (use_trimesh_raycast=False, cast_on_mfs=True): an S x S pixel patch is laid on the tangent plane of every
        candidate, aligned with the mesh's first principal direction, cast onto the mesh along -normal, and -- unless a pixel's origin is NaN, the
        patch lies farther than min(0.1, 3 h_threshold) from the scan cloud, or a ray misses -- its hits are projected and looked up in the
        field's own tables.  What the reference gets from open3d / trimesh / sklearn comes from the caller:
          sample_points, sample_normals [n,3]  the candidate centres and their normals (Poisson-disk samples with face normals, or template vertices)
          scan_points [m,3]                    the scan cloud; None: no scan test, and candidates below y = 0 are dropped (:1026)
          sample_mesh = (vertices, faces)      the picked faces to cast on (and whose edges set grid_gap); default: the field's own mesh and tracer
          first_component, grid_gap            default: `patches.principal_direction` of the field's mesh, `patches.patch_grid_gap` of sample_mesh
        patches_per_chunk: candidates per front call (default: about 2^18 rays).  Every chunk is one nerftex_patch_front call and one read-back of
        its verdicts and slots -- the chunk's only host synchronisation; everything else stays on the device until the loop has ended, at
        max_patch_num accepted patches or the last candidate.  fused=False: the staged form (`patches._export_field_reference`), the
        reference's loop patch by patch; the two agree bit for bit.
        -> dict of float32 numpy arrays (the reference holds the same fp32 values in float64 arrays), P accepted patches, S = patch_size:
          patches [P,S,S,16], grid_gap (float), patch_coors [P,S,S,3], patch_norms [P,3], patch_sample_tbn [P,9] (the frame's axes x, y, z in
          fp32), patch_local_tbn [P,S,S,9], picked_vertices [P,3], patch_phi_embed [P,S,S,8] (None without a normal net), patch_rays [P,S,S,6]
          (None unless record_rays), and two keys the reference does not have: candidate_ids [P] int64 and verdicts [n] uint8
          (`patches.ACCEPTED` ... `patches.NOT_NEEDED`).
        Deviations: the reference's 'mesh' entry is dropped (the caller has it), and where it returns an untruncated zero array for the rays
        without record_rays, this returns None.  An imported field refuses: switch_import() back first."""
        from . import patches

        kw = dict(scan_points=scan_points, first_component=first_component, grid_gap=grid_gap, pattern_rate=pattern_rate, patch_size=patch_size,
                  max_patch_num=max_patch_num, sample_mesh=sample_mesh, record_rays=record_rays)
        if fused:
            return patches.export_field(self, sample_points, sample_normals, patches_per_chunk=patches_per_chunk, **kw)
        return patches._export_field_reference(self, sample_points, sample_normals, **kw)

    def synthesize_field(self, result, output_size, *, rescale=None, **kw):
        """The step between export and import (the reference's offline patch_matching_and_quilting.py): `synthesis.synthesize_texture` over what
        `export_field` returned, on this field's device, and `import_field` of the map it makes -- with the four light maps if this field reads a
        fine normal, without them otherwise.  -> (texture, log) as synthesize_texture returns them.  kw: its keywords."""
        from . import synthesis

        kw.setdefault("light_maps", self._lit())
        texture, log = synthesis.synthesize_texture(result, output_size, device=self.sigma_net.weights.device, **kw)
        self.import_field(rescale=rescale, **texture)
        return texture, log

    def switch_import(self):
        """network_curvedfield.py:519-521: between the imported map and the field's own mesh and table (the map is kept)."""
        if self.features_imported is None:
            raise RuntimeError("CurvedField.switch_import: nothing has been imported")
        self.imported = not self.imported
        self._import_version += 1

    def set_uv_utilize_rate(self, rate=1.0):
        self.uv_utilize_rate = float(rate)
        self._import_version += 1

    def set_sdf_offset(self, sdf_offset=0.0):
        self.sdf_offset = float(sdf_offset)
        self._import_version += 1

    def set_h_threshold(self, h_threshold=0.03):
        """network_curvedfield.py:539-541: the one threshold the mesh projector and the imported map's mask read."""
        self.h_threshold = self.projector.h_threshold = float(h_threshold)
        self._import_version += 1

    def _import_scalars(self):
        """(mode, plane scales, height scales, sdf_offset, h_threshold) of nerftex_planar_lookup for the state as it is: `rescale` multiplies,
        u, v = x, y rate and sdf = (z b0) rate - offset; otherwise u, v = x / b0, y / b1 and sdf = z - offset (the two ones multiply exactly)."""
        from nerftex_hip import PLANAR_DIVIDE, PLANAR_MULTIPLY

        b0, b1, rate = float(self.bounds[0]), float(self.bounds[1]), float(self.uv_utilize_rate)
        if self.rescale:
            return (PLANAR_MULTIPLY, rate, rate, b0, rate, float(self.sdf_offset), float(self.h_threshold))
        return (PLANAR_DIVIDE, b0, b1, 1.0, 1.0, float(self.sdf_offset), float(self.h_threshold))

    def _import_stamp(self):
        """graph_stamp()'s share of the import state: nothing unless a map is in use (the stamp of a field that never imported is unchanged)."""
        if not getattr(self, "imported", False):
            return ()
        f = self.features_imported
        if self._patch_active():  # the patch's records, its neighbour grid, the threshold
            kn = self._patch_knn
            return (("import-patch", f.data_ptr(), tuple(f.shape), None if kn is None else kn.value, self.patch_geom.data_ptr(),
                     None if self.patch_lit is None else self.patch_lit.data_ptr(), float(self.h_threshold), self._import_version))
        if self._unhash_active():  # the per-vertex rows, the fine mesh's arrays and its tracer, the scalars
            return (("import-unhash", f.data_ptr(), tuple(f.shape), self.unhash_vertices.data_ptr(), self.unhash_face_vertices.data_ptr(),
                     self.unhash_tracer._handle.value) + self._unhash_scalars()[1:] + (self._import_version,))
        if self._shape_active():
            p = self.shape_projector
            stamp = (("import-shape", f.data_ptr(), tuple(f.shape), p._knn.value, p.tracer._handle.value, p.mesh_vertices.data_ptr(), p.vertex_normals.data_ptr(),
                      self.shape_face_uv.data_ptr()) + self._shape_scalars() + (self._import_version,))
            if getattr(self, "shape_face_tbn", None) is not None:  # the lit field's maps and frames
                stamp += self._lit_maps_stamp(self.shape_face_tbn)
            return stamp
        return ("import", f.data_ptr(), tuple(f.shape)) + self._import_scalars() + (self._import_version,) + self._lit_maps_stamp()

    def _lit_maps_stamp(self, *more):
        """_import_stamp()'s share of the lit field's maps (and `more`): their storage and shapes; nothing for a field that reads no fine normal."""
        if not (self._lit() and self.phi_embed_imported is not None):
            return ()
        return tuple((m.data_ptr(), tuple(m.shape)) for m in (self.phi_embed_imported, self.local_tbn_imported, self.sample_tbn_inv_imported,
                                                              self.sample_tbn_ids_imported, self.frame_map_imported, self.sample_inv_rows_imported) + more)

    @torch.no_grad()
    def _import_lookup(self, x):
        """nerftex_planar_lookup: -> p_uv [N,2], sdf [N], h_mask [N] bool, xin [N,48] half (the sigma net's padded input)."""
        from nerftex_hip import check, lib, stream

        x, f = x.detach().float().contiguous(), self.features_imported
        p_uv, sdf, mask, xin = out = self._lookup_buffers(x, "p_uv", "sdf", "mask", "xin")
        check(lib.nerftex_planar_lookup(ptr(x), ptr(f), f.shape[0], f.shape[1], *self._import_scalars(), int(self.multires), x.shape[0], *map(ptr, out), stream()))
        return p_uv, sdf, mask.bool(), xin

    def _import_normal(self, x, normalised):
        """normal_coarse of the import branch (:667-668): (0, 0, 1), divided by |n| + 1e-5 as tools/map.py:720 does when `normalised`."""
        n = torch.zeros(x.shape[0], 3, dtype=torch.float32, device=x.device)
        n[:, 2] = 1.0
        return n / (n.norm(dim=-1, keepdim=True) + 1e-5) if normalised else n

    def _sample_map(self, m, p_uv, mode="bilinear"):
        """grid_sample of the map m [H, W, C] at p_uv [N, 2] -> [C, N].  [H, W, C] -> [1, C, W, H]: the grid's first coordinate indexes the last
        axis, so u runs along the map's first axis (tools/map.py:915-919)."""
        image = m.to(p_uv.device).permute(2, 1, 0).unsqueeze(0)
        return torch.nn.functional.grid_sample(image, p_uv[None, None], mode=mode, align_corners=True, padding_mode="zeros")[0, :, 0]

    def _lit_maps_reference(self, p_uv):
        """The four reads of the `pred_normal` part at p_uv (tools/map.py:670-675), the planar map's and the imported mesh's alike: -> the
        sampled phi_embed [N,8], local_tbn [N,3,3] and id [N] (nearest texel), and the inverted patch frames' rows `id` [N,3,3]."""
        ids = self._sample_map(self.sample_tbn_ids_imported[..., None], p_uv, mode="nearest")[0].long()
        sample_tbn_inv = self.sample_tbn_inv_imported.to(p_uv.device)[ids]
        local_tbn = self._sample_map(self.local_tbn_imported, p_uv, mode="nearest").permute(1, 0).reshape(-1, 3, 3)
        return self._sample_map(self.phi_embed_imported, p_uv).permute(1, 0), local_tbn, ids, sample_tbn_inv

    def _import_embed_reference(self, x, details=False):
        """The import branch op by op, the reference's expressions (tools/map.py:649-668): -> embed [N,41] fp32, normal_coarse, h_mask (details:
        + p_uv).  The divisors are tensors: a device division by a Python scalar is a multiplication by its reciprocal, the reference's (as
        executed) is a true division."""
        x = x.float()
        b0, b1 = (torch.tensor(b, dtype=torch.float32, device=x.device) for b in self.bounds)
        if self.rescale:
            p_sur = x[..., :2] * self.uv_utilize_rate
            sdf = x[..., -1:] * self.bounds[0] * self.uv_utilize_rate
        else:
            p_sur = torch.stack([x[..., 0] / b0, x[..., 1] / b1], dim=-1)
            sdf = x[..., -1:]
        sdf = sdf - self.sdf_offset
        h_mask = sdf[..., 0].abs() < self.h_threshold
        h_mask = torch.logical_and(h_mask, (p_sur >= -1.0).all(dim=-1))
        h_mask = torch.logical_and(h_mask, (p_sur <= 1.0).all(dim=-1))
        embed = torch.cat([self._sample_map(self.features_imported, p_sur).permute(1, 0), freq_encode(sdf, self.multires)], dim=-1)
        return (embed, self._import_normal(x, True), h_mask) + ((p_sur,) if details else ())

    def _sigma_fused(self, x=None):
        """The one shape predicate every lookup and chain below asks: the sigma side has the default shapes under fp16 autocast without the
        probabilistic table, and the samples x are on a device (None: a question about the field alone, `_glue_fused()`)."""
        return ((x is None or x.is_cuda) and self.encoder_var is None and self.in_dim == 41 and self.in_pad == 48 and self.geo_feat_dim == 15
                and self.multires == 12 and self.sigma_net.dtype == torch.float16 and torch.is_autocast_enabled()
                and torch.get_autocast_dtype("cuda") == torch.float16)

    def _import_fused(self, x):
        """Whether the lookup kernels serve the static field's imported map: what the glue launches behind them ask."""
        return self._glue_fused(x)

    def _import_light_fused(self, x):
        """_import_fused() for the lit field (which has no colour net for _glue_fused() to ask about): the planar lookups serve it once the four
        maps are there."""
        return self._lit() and self.phi_embed_imported is not None and not self._shape_active() and self._sigma_fused(x)

    def _source_fused(self, x, lit=False):
        """Whether the lookup kernels serve the ACTIVE imported source for this call (lit: with the reads the fine normal needs)."""
        if self._patch_active():
            return self._patch_fused(x)
        if self._unhash_active():
            return not lit and self._unhash_fused(x)
        lit_reads = self._shape_light_fused(x) if self._shape_active() else self._import_light_fused(x)
        return lit_reads or (not lit and self._import_fused(x))  # (the lit field without a fine normal: none of the lit reads is needed)

    def _source_lookup(self, x, lit=False):
        """The one lookup of the active imported source -- patch, map on the imported mesh, planar map -- through its kernel (`_source_fused`
        holds): h_mask [N], the raw normal [N,3] (None: the planar map's, `_import_normal`), xin [N,48] half, and with `lit` the phi_embed
        [N,8] and the frames [N,3,3] in the order `_rotate_fine` takes them."""
        if self._patch_active():
            out = self._patch_lookup(x, lit=lit)
            return _SourceLookup(out[1], out[2], out[3], *((out[7], out[8:]) if lit else ()))
        if self._unhash_active():
            out = self._unhash_lookup(x)
            return _SourceLookup(out[1], out[2], out[5])
        if self._shape_active():
            out = self._shape_light_lookup(x) if lit else self._shape_lookup(x)
            return _SourceLookup(out[2], out[3], out[5], *((out[6], out[8:]) if lit else ()))
        out = self._import_light_lookup(x) if lit else self._import_lookup(x)
        return _SourceLookup(out[2], None, out[3], *((out[4], out[6:]) if lit else ()))

    @torch.no_grad()
    def _import_light_lookup(self, x):
        """nerftex_planar_light_lookup: -> p_uv [N,2], sdf [N], h_mask [N] bool, xin [N,48] half, phi [N,8] fp32, id [N] int32, local_tbn [N,3,3],
        sample_tbn_inv [N,3,3] (row `id` of the inverted patch frames)."""
        from nerftex_hip import check, lib, stream

        x, f, rows = x.detach().float().contiguous(), self.features_imported, self.sample_inv_rows_imported
        p_uv, sdf, mask, xin, phi, ids, local, sample = out = self._lookup_buffers(x, "p_uv", "sdf", "mask", "xin", "phi", "ids", "frame", "frame")
        check(lib.nerftex_planar_light_lookup(ptr(x), ptr(f), ptr(self.phi_embed_imported), ptr(self.frame_map_imported), ptr(rows), f.shape[0], f.shape[1],
                                              rows.shape[0], *self._import_scalars(), int(self.multires), x.shape[0], *map(ptr, out), stream()))
        return p_uv, sdf, mask.bool(), xin, phi, ids, local.view(x.shape[0], 3, 3), sample.view(x.shape[0], 3, 3)

    @staticmethod
    def _rotate_fine(local, *frames):
        """tools/map.py:724-730: the local normal rotated by the texel's frame, then (a map) by the patch's inverted frame, then (the 'shape'
        branch) by the new mesh's face frame, normalised."""
        fine = local
        for tbn in frames:
            fine = torch.einsum("nba,nb->na", tbn, fine)
        return fine / (fine.norm(dim=-1, keepdim=True) + 1e-5)

    def _import_light_embed_reference(self, x, details=False):
        """The import branch with `pred_normal` op by op, the reference's expressions (tools/map.py:649-675, :722-730) over grid_sample:
        -> embed [N,41] fp32, normal_coarse, h_mask, normal_fine (details: + the sampled phi_embed, local_tbn, id and sample_tbn_inv rows)."""
        embed, normal_coarse, h_mask, p_sur = self._import_embed_reference(x, details=True)
        phi, local_tbn, ids, sample_tbn_inv = self._lit_maps_reference(p_sur)
        x_embed, z_embed = embed[:, :self.encoder.output_dim], embed[:, self.encoder.output_dim:]
        local = self.normal_net(phi_embed=phi, z_embed=z_embed, x_embed=x_embed)
        fine = self._rotate_fine(local, local_tbn, sample_tbn_inv)
        if details:
            return embed, normal_coarse, h_mask, fine, phi, local_tbn, ids, sample_tbn_inv
        return embed, normal_coarse, h_mask, fine

    def fine_normal(self, x, no_noise=False, requires_grad_xyz=False):
        """normal_fine of MeshFeatureField.forward (tools/map.py:637-641, 726-735): the factorized net's local normal rotated into the world by the
        hit face's frame, normalised.  -> (normal_fine [N,3], normal_coarse [N,3], h_mask [N])."""
        assert self.normal_net is not None, "CurvedField(pred_normal=True)"
        embed, normal_coarse, h_mask, normal_fine = self.embed(x, no_noise=no_noise, requires_grad_xyz=requires_grad_xyz, with_fine_normal=True)
        return normal_fine, normal_coarse, h_mask

    def embed(self, x, no_noise=False, requires_grad_xyz=False, with_fine_normal=False):
        """MeshFeatureField.forward (no import, tools/map.py:620-641): -> embed [N,41], normal_coarse [N,3], h_mask [N]
        (+ normal_fine [N,3] with with_fine_normal, the 4-tuple of :737 in the reference's order embed, normal_coarse, normal_fine, h_mask
        re-ordered to keep the 3-tuple's positions).
        requires_grad_xyz (network_curvedfield.py:236-259, the branch that differentiates sigma with respect to the sample position): the
        projection carries `diff_project_layer`'s gradient, the hash table is looked up with input gradients (dy_dx) and the height ladder
        is evaluated by framework ops on the differentiable height -- dL/dembed reaches x."""
        if getattr(self, "imported", False):  # the import branches (:646-707): a patch, the planar map or the map on the imported mesh instead of the mesh and the table
            if self._patch_active():
                if requires_grad_xyz or (with_fine_normal and self.patch_lit is None):
                    raise NotImplementedError("CurvedField.embed: an imported patch is rendered without gradients to the sample position, and without a fine "
                                              "normal unless it came with local_tbn and phi_embed")
            elif self._unhash_active():
                if requires_grad_xyz or with_fine_normal:
                    raise NotImplementedError("CurvedField.embed: the features baked onto a fine mesh are rendered without gradients to the sample position "
                                              "and without a fine normal")
            else:
                lit_maps = self._lit() and self.phi_embed_imported is not None and (not self._shape_active() or self.shape_face_tbn is not None)
                if requires_grad_xyz or (with_fine_normal and not lit_maps):
                    raise NotImplementedError("CurvedField.embed: an imported map is rendered without gradients to the sample position and without a fine normal")
            if self._source_fused(x, with_fine_normal):
                s = self._source_lookup(x, with_fine_normal)
                coarse = self._import_normal(x, True) if s.normal is None else s.normal / (s.normal.norm(dim=-1, keepdim=True) + 1e-5)
                if not with_fine_normal:
                    return s.xin[:, :self.in_dim], coarse, s.h_mask
                # the `pred_normal` part (:670-675, :687-692, :702-707, :722-730): the normal net fed from the source's phi_embed, one rotation per frame
                local = self.normal_net(phi_embed=s.phi, z_embed=s.xin[:, 16:self.in_dim], x_embed=s.xin[:, :16])
                return s.xin[:, :self.in_dim], coarse, s.h_mask, self._rotate_fine(local, *s.frames)
            if self._patch_active():  # ... and op by op where the kernels do not serve the call
                return self._patch_embed_reference(x, with_fine_normal=with_fine_normal)
            if self._unhash_active():
                return self._unhash_embed_reference(x)
            if self._shape_active():
                return self._shape_light_embed_reference(x) if with_fine_normal else self._shape_embed_reference(x)
            return self._import_light_embed_reference(x) if with_fine_normal else self._import_embed_reference(x)
        if requires_grad_xyz:
            p_sur, sdf, h_mask, normal, local_tbn = self.projector.project(x, K=self.projector.K, h_threshold=self.h_threshold, requires_grad_xyz=True)
            z_embed = freq_encode(sdf, self.multires)
        else:
            p_sur, sdf, h_mask, normal, local_tbn, _, z_embed = self.projector.project_fused(x, multires=self.multires)
        x_embed = self.encoder(p_sur, bound=self.bound)
        if self.encoder_var is not None:
            var = self.encoder_var(p_sur, bound=self.bound)
            noise = torch.zeros_like(var) if no_noise else torch.randn_like(var)
            x_embed = x_embed + noise * torch.exp(var)
        embed = torch.cat([x_embed, z_embed.to(x_embed.dtype)], dim=-1)
        normal = normal / (normal.norm(dim=-1, keepdim=True) + 1e-5)  # tools/map.py:720
        if with_fine_normal:
            local = self.normal_net(p_sur=p_sur, z_embed=z_embed, x_embed=x_embed)  # :639
            fine = torch.einsum("nba,nb->na", local_tbn, local)  # :727 (the frame's rows are t, b, n: local -> world)
            fine = fine / (fine.norm(dim=-1, keepdim=True) + 1e-5)  # :732
            return embed, normal, h_mask, fine
        return embed, normal, h_mask

    def _sigma(self, embed):
        ones = torch.ones(embed.shape[0], self.in_pad - self.in_dim, dtype=embed.dtype, device=embed.device)  # tcnn pads its inputs with ones
        h = self.sigma_net(torch.cat([embed, ones], dim=-1))
        return _TruncExp.apply(h[..., 0]), h[..., 1:]

    def density(self, x, requires_grad_xyz=False):
        if getattr(self, "imported", False) and not requires_grad_xyz and self._source_fused(x):
            s = self._source_lookup(x)
            h = self.sigma_net(s.xin)
            sigma = _TruncExp.apply(h[..., 0])
            return {"sigma": torch.where(s.h_mask, sigma, torch.zeros_like(sigma)), "geo_feat": h[..., 1:]}
        embed, _, h_mask = self.embed(x, requires_grad_xyz=requires_grad_xyz)
        sigma, geo = self._sigma(embed)
        return {"sigma": torch.where(h_mask, sigma, torch.zeros_like(sigma)), "geo_feat": geo}

    def density_gradient(self, x, lambda_=5e-2, create_graph=False):
        """network_curvedfield.py:236-254: sigma and d sigma_remap / dx, sigma_remap = (1 - exp(-lambda sigma)) / lambda, through the whole
        chain -- sigma net backward (with input gradients), FreqEncoder(height) and the hash table's input gradient (G3), the projection's
        `diff_project_layer`.  -> (sigma [N], gradient [N,3], h_mask [N]); the unmasked sigma, as the reference's branch has it there.
        create_graph: the reference asks autograd for a differentiable gradient (:253, create_graph=True -- its tcnn networks have second
        derivatives).  The backward kernels behind this chain (G3, the FFMLP input gradient, the projection layer) are first-order, as
        torch-ngp's own `_grid_encode.backward` is (`once_differentiable`, gridencoder/grid.py:56): with create_graph=True the returned
        gradient carries the graph of the framework ops only (sigma_remap's exp, the height ladder) and sigma stays attached."""
        with torch.enable_grad():
            x = x.detach().requires_grad_(True)
            embed, _, h_mask = self.embed(x, requires_grad_xyz=True)
            sigma, _ = self._sigma(embed)
            sigma_remap = 1 / lambda_ * (1 - torch.exp(-lambda_ * sigma))
            grad = torch.autograd.grad(sigma_remap, x, torch.ones_like(sigma), create_graph=create_graph, retain_graph=create_graph)[0]
        return (sigma if create_graph else sigma.detach()), grad, h_mask

    def density_normal(self, x, lambda_=5e-2, create_graph=False):
        """network_curvedfield.py:236-259: the normal from sigma's gradient, n = -d sigma_remap / dx normalised; samples whose gradient is
        not a number leave the mask.  -> (sigma [N], normal_grad [N,3], h_mask [N])."""
        sigma, grad, h_mask = self.density_gradient(x, lambda_, create_graph)
        normal_grad = -grad
        normal_grad = normal_grad / (normal_grad.norm(dim=-1, keepdim=True) + 1e-5)
        h_mask = torch.logical_and(h_mask, torch.logical_not(normal_grad.isnan()).all(dim=-1))
        return sigma, normal_grad, h_mask

    def _glue_fused(self, x=None):
        """The three glue launches (csrc/fieldglue.hip, round 6) serve the static light model's default shapes (`_sigma_fused`, and the colour
        side's), unless `fused_glue` is off."""
        return (getattr(self, "light_model", None) is None and getattr(self, "fused_glue", True) and self._sigma_fused(x) and self.color_pad == 32
                and self.encoder_dir.output_dim == 16)

    # ---- the lighting rotation (network_curvedfield.py:303-308, the reference's `euler`; its light turntable: nerf/utils.py:871-902) ----

    @staticmethod
    def light_rotation_matrix(euler):
        """R.from_rotvec(euler).as_matrix() without scipy: Rodrigues' formula in float64, I + sin(t) K + (1 - cos(t)) K^2 with K the unit axis'
        cross-product matrix.  -> float64 [3, 3]; a zero vector gives the identity exactly."""
        v = np.asarray(euler, dtype=np.float64).reshape(-1)
        if v.shape != (3,) or not np.isfinite(v).all():
            raise ValueError(f"CurvedField: a lighting rotation is a finite rotation vector of 3 values, but got {euler!r}")
        t = float(np.sqrt(v @ v))
        if t == 0.0:
            return np.eye(3)
        k = v / t
        K = np.array([[0.0, -k[2], k[1]], [k[2], 0.0, -k[0]], [-k[1], k[0], 0.0]])
        return np.eye(3) + np.sin(t) * K + (1.0 - np.cos(t)) * (K @ K)

    def set_light_rotation(self, euler):
        """The reference's `euler`, kept on the field: in eval the light head sees the view direction, the shading normal and the coarse normal
        rotated by R.from_rotvec(euler) (forward(), and the lit chains with `fused_relight_infer`).  None switches the rotation off; a zero vector
        does not -- as in the reference it is a product with the identity, which rounds to half under autocast.  The fp32 matrix is written IN PLACE
        into one persistent [9] device buffer: a new vector changes values a recorded graph reads, not what it bakes in (`_light_stamp`)."""
        if euler is None:
            self._light_rotation_on, self._light_euler = False, None
            return
        if getattr(self, "light_model", None) is None:
            raise ValueError("CurvedField.set_light_rotation: the static field has no light model to rotate (light_model='SH' has)")
        m = torch.from_numpy(self.light_rotation_matrix(euler).astype(np.float32).reshape(9))
        buf = getattr(self, "_light_rotation", None)
        dev = self.light_net.envSHs.device
        if buf is None or buf.device != dev:
            buf = self._light_rotation = torch.empty(9, dtype=torch.float32, device=dev)
        buf.copy_(m)
        self._light_rotation_on, self._light_euler = True, tuple(float(e) for e in np.asarray(euler, dtype=np.float64).reshape(3))

    def light_rotation(self):
        """The rotation vector set_light_rotation keeps, or None."""
        return getattr(self, "_light_euler", None) if getattr(self, "_light_rotation_on", False) else None

    def _light_rotation_active(self):
        """Whether the stored rotation turns the lighting of this call: it is set, and the field is in eval (the reference's `not self.training`)."""
        return bool(getattr(self, "_light_rotation_on", False)) and not self.training

    def _per_probe_lighting(self):
        """Whether forward() asks the head for one lighting per visibility probe (or its refusal without tables): eval, an imported lighting
        switched on, `shade_visibility`."""
        net = self.light_net
        return (not self.training and bool(getattr(net, "import_envmap", False)) and getattr(net, "envSHs_import", None) is not None
                and bool(getattr(self, "shade_visibility", True)))

    def _relight_desc(self):
        """The nerftex_relight_desc of a lit chain's call (and the tensors it points into), or None where neither per-probe lighting nor a rotation
        is in effect: then the plain entry is called, as before."""
        probe, rot = self._per_probe_lighting(), self._light_rotation_active()
        if not (probe or rot):
            return None
        net = self.light_net
        probes, tables = (net.probes, net.envSHs_import_vis) if probe else (None, None)
        buf = self._light_rotation if rot else None
        return RelightDesc(probes=ptr(probes), probe_shs=ptr(tables), K=0 if probes is None else probes.shape[0], rotation=ptr(buf)), (probes, tables, buf)

    @staticmethod
    def _rotate_lighting(rotation, *vectors):
        """network_curvedfield.py:305-308: einsum('ab,nb->na', rot, v) for each [N,3] vector (None stays None), rot in the vectors' dtype and on
        their device as there; the results as fp32."""
        ref = next(v for v in vectors if v is not None)
        rot = rotation.to(device=ref.device, dtype=ref.dtype)
        return tuple(None if v is None else torch.einsum("ab,nb->na", rot, v).float() for v in vectors)

    def _forward_light(self, x, d, normal_supervision=False, rotation=None):
        """network_curvedfield.py:272-301, 327-349, 396-409 with the SH light model: the head shades with the fine normal -- detached in training
        (:331), blended with the coarse normal by fc_weight and renormalised in eval (:293-301) -- and the view direction as it is.  In eval
        `light_visual_mode` picks the head's output.  normal_supervision (training): the reference's ret_dict, 'normal' = the fine normal on the
        graph, 'normal_grad' = the density normal (first order, detached: the reference detaches it too) blended with the coarse normal by
        smooth_grad_weight and renormalised (:274-277); samples whose density normal is not a number leave the mask (:258).
        The reference differentiates sigma on EVERY training forward of a light-model network (:236-258), so there its training mask always
        drops those samples; here a training call without normal_supervision does not evaluate the density normal and keeps them.  With
        normal_supervision the projector and the table lookup run twice, once in embed() and once in density_normal()."""
        embed, normal_coarse, h_mask, normal_fine = self.embed(x, with_fine_normal=True)
        sigma, geo = self._sigma(embed)
        ret = {}
        if self.training and normal_supervision:
            _, normal_grad, h_mask = self.density_normal(x)
            sup = normal_grad.detach() * (1 - self.smooth_grad_weight) + normal_coarse * self.smooth_grad_weight
            ret = {"normal": normal_fine, "normal_grad": sup / (sup.norm(dim=-1, keepdim=True) + 1e-5)}
        normal = normal_fine / (normal_fine.norm(dim=-1, keepdim=True) + 1e-5)
        if self.training:
            normal = normal.detach()
        else:
            coarse = normal_coarse / (normal_coarse.norm(dim=-1, keepdim=True) + 1e-5)
            normal = self.fc_weight * normal + (1 - self.fc_weight) * coarse
            normal = normal / (normal.norm(dim=-1, keepdim=True) + 1e-5)
        relight = {}
        if not self.training and getattr(self.light_net, "import_envmap", False):
            # the probe of an imported lighting is chosen by the coarse normal (:296, :339, :341: shade_visibility = self.shade_visibility or
            # self.training); the head reads neither outside eval with an import, so only then are they handed over
            relight = dict(normal_secondary=normal_coarse / (normal_coarse.norm(dim=-1, keepdim=True) + 1e-5),
                           shade_visibility=bool(getattr(self, "shade_visibility", True)))
        if rotation is not None and not self.training:
            # :304-308 op by op.  Under fp16 autocast each einsum is a half product (both operands cast to half, fp32 accumulation, a half result);
            # the head's kernels take fp32 vectors, so the half values are widened again
            d, normal, secondary = self._rotate_lighting(rotation, d, normal, relight.get("normal_secondary"))
            if relight:
                relight["normal_secondary"] = secondary
        full, specular, diffuse, albedo = self.light_net(geo, normal, d, mask=h_mask, **relight)
        modes = {"Full": full, "Specular": specular, "Diffuse": diffuse, "Albedo": albedo}
        if not self.training and self.light_visual_mode not in modes:
            raise ValueError(f"CurvedField.light_visual_mode is one of {sorted(modes)}, but got {self.light_visual_mode!r}")
        color = full if self.training else modes[self.light_visual_mode]
        return torch.where(h_mask, sigma, torch.zeros_like(sigma)), color, ret

    def forward(self, x, d, **kwargs):
        """euler (keyword, as NeRFNetwork.forward's): a lighting rotation vector for this call, overriding set_light_rotation's -- None: no
        rotation.  The static field has no lighting to rotate and raises ValueError rather than ignore one."""
        if getattr(self, "light_model", None) == "SH":
            if "euler" in kwargs:
                rotation = None if kwargs["euler"] is None else torch.from_numpy(self.light_rotation_matrix(kwargs["euler"]).astype(np.float32))
            else:
                rotation = self._light_rotation.view(3, 3) if self._light_rotation_active() else None
            return self._forward_light(x, d, normal_supervision=bool(kwargs.get("normal_supervision", False)), rotation=rotation)
        if kwargs.get("euler") is not None or getattr(self, "_light_rotation_on", False):
            raise ValueError("CurvedField.forward: a lighting rotation is set, but the static field has no light model to rotate")
        if getattr(self, "imported", False) and self._glue_fused(x) and self._source_fused(x):
            s = self._source_lookup(x)
            normal = self._import_normal(x, False) if s.normal is None else s.normal
            h = self.sigma_net(s.xin)
            sigma_raw, cin = _CurvedMid.apply(h, normal, d, self.fc_weight, 2 | int(not self.training))  # (bit 1: tools/map.py:720 in the kernel)
            sigma, color = _CurvedOut.apply(self.color_net(cin), sigma_raw, s.h_mask)
            return sigma, color, {}
        if self._glue_fused(x) and not getattr(self, "imported", False):
            p_sur, sdf, h_mask, normal, local_tbn, _, z_embed = self.projector.project_fused(x, multires=self.multires)
            x_embed = self.encoder(p_sur, bound=self.bound)
            if x_embed.dtype == torch.float16 and z_embed.dtype == torch.float32:
                h = self.sigma_net(_CurvedPack.apply(x_embed, z_embed))
                # (mode bit 1: the kernel also does MeshFeatureField's own normalisation of the projector's normal, tools/map.py:720)
                sigma_raw, cin = _CurvedMid.apply(h, normal, d, self.fc_weight, 2 | int(not self.training))
                sigma, color = _CurvedOut.apply(self.color_net(cin), sigma_raw, h_mask)
                return sigma, color, {}
        embed, normal_coarse, h_mask = self.embed(x)
        sigma, geo = self._sigma(embed)
        normal = normal_coarse / (normal_coarse.norm(dim=-1, keepdim=True) + 1e-5)  # network_curvedfield.py:283-285 (normal = normal_coarse)
        if not self.training:  # :289-291 with the coarse normal on both sides
            normal = self.fc_weight * normal + (1 - self.fc_weight) * normal
            normal = normal / (normal.norm(dim=-1, keepdim=True) + 1e-5)
        dn = d / (d.norm(dim=-1, keepdim=True) + 1e-5)
        wr = 2 * (-dn * normal).sum(-1, keepdim=True) * normal + dn  # the view direction reflected about the normal (:305-306)
        wr = (wr + 1) / 2  # tcnn's SH takes [0, 1] ...
        dir_embed = self.encoder_dir(wr * 2 - 1)  # ... and maps it back
        pad = torch.ones(x.shape[0], self.color_pad - self.color_in, dtype=geo.dtype, device=x.device)
        h = self.color_net(torch.cat([dir_embed.to(geo.dtype), geo, pad], dim=-1))
        color = torch.sigmoid(h)
        return torch.where(h_mask, sigma, torch.zeros_like(sigma)), torch.where(h_mask.unsqueeze(-1), color, torch.zeros_like(color)), {}

    def graph_stamp(self):
        """What a recorded graph of `infer` bakes in besides the parameters (Renderer.render_infer_graphed adds it to its stamp): the neighbour
        grid's and the tracer's handles, the mesh buffers' storage, the projector's and the field's scalars, train / eval, the fused switch."""
        p = self.projector
        return (p._knn.value, p.tracer._handle.value, p.mesh_vertices.data_ptr(), p.vertex_normals.data_ptr(), p.tbn.data_ptr(), int(p.K),
                p._height_limit(...), float(self.fc_weight), float(self.bound), bool(self.training), bool(getattr(self, "fused_glue", True))) + self._light_stamp() + self._import_stamp()

    def _light_stamp(self):
        """graph_stamp()'s share of the light model: nothing without one (the stamp of today's field is unchanged)."""
        if getattr(self, "light_model", None) is None:
            return ()
        net = self.light_net
        stamp = (self.light_model, self.light_visual_mode, float(net.gamma), bool(net.use_specular), bool(net.fused), net.envSHs.data_ptr(), tuple(net.envSHs.shape))
        if not getattr(self, "fused_light_infer", False):
            return stamp + (False,) + self._relight_stamp() + self._rotation_stamp()
        # the fused chain bakes in the normal net's table and the packed copy of its weights: the table's storage and every parameter's version
        nn = self.normal_net
        return stamp + (True, nn.encoder.embeddings.data_ptr(), nn.encoder.offsets.data_ptr(),
                        tuple((q.data_ptr(), q._version) for q in list(nn.phi_net.parameters()) + list(nn.theta_net.parameters()))) + self._relight_stamp() + self._rotation_stamp()

    def _rotation_stamp(self):
        """_light_stamp()'s share of `fused_relight_infer` and the lighting rotation, appended only once the switch is on or a rotation is set (the
        stamp without either is unchanged): the switch, whether a rotation is on, the rotation buffer's storage.  Never the rotation's VALUES: the
        kernels read them from that buffer when they run, so a new rotation vector replays the recorded graphs."""
        switch, on = bool(getattr(self, "fused_relight_infer", False)), bool(getattr(self, "_light_rotation_on", False))
        if not (switch or on):
            return ()
        buf = getattr(self, "_light_rotation", None)
        return (switch, on, buf.data_ptr() if on and buf is not None else 0)

    def _lighting(self):
        """The lighting the head shades with: light_net.lighting() -- the imported coefficients in eval once switched on, envSHs otherwise (and
        of a head that knows no imported lighting)."""
        net = self.light_net
        return net.lighting() if hasattr(net, "lighting") else net.envSHs

    def _relight_stamp(self):
        """_light_stamp()'s share of an imported lighting, appended only once one has been loaded (the stamp without one is unchanged): the
        storage and shape of the lighting in effect, the import switch, shade_visibility and the probe tables' storage."""
        net = self.light_net
        if getattr(net, "envSHs_import", None) is None:
            return ()
        env = self._lighting()
        return (env.data_ptr(), tuple(env.shape), bool(net.import_envmap), bool(getattr(self, "shade_visibility", True)),
                0 if net.envSHs_import_vis is None else net.envSHs_import_vis.data_ptr(), 0 if net.probes is None else net.probes.data_ptr())

    # ---- the nine fused inference chains: what each asks of a call (the entries refuse everything else) ----
    _SIGMA_NET, _COLOR_NET, _BRDF_NET = (48, 32, 2, 16), (32, 64, 3, 3), (16, 64, 3, 5)  # (in, hidden, layers, out) the entries' kernels are built for

    @staticmethod
    def _on_device_of(x, *tensors):
        return all(t.device == x.device for t in tensors)

    # ---- the predicates of `_INFER_ROUTES`, composed of four conjuncts: the batch and the sigma net (`_infer_rows_ok`), the static back half
    # (`_infer_static_back_ok`), the lit one (`_infer_light_back_fused`), the source's tensors on the device of x (`_on_device_of`) -- and of what
    # serves the source's lookup (`_infer_front_fused`, `_import_fused`, `_import_light_fused`, `_shape_light_fused`, `_patch_fused`).

    def _infer_rows_ok(self, x, d):
        """The batch every entry takes -- whole 128-row workgroups, contiguous fp32 inputs -- and the sigma net its kernels are built for."""
        B, s = x.shape[0], self.sigma_net
        return (B > 0 and B % 128 == 0 and x.dtype == torch.float32 and d.dtype == torch.float32 and x.is_contiguous() and d.is_contiguous()
                and (s.input_dim, s.hidden_dim, s.num_layers, s.padded_output_dim) == self._SIGMA_NET)

    def _infer_static_back_ok(self, x):
        """What the static light model's three chains ask alike behind the lookup: _glue_fused() and the colour net the entries are built for."""
        c = self.color_net
        return self._glue_fused(x) and c.dtype == torch.float16 and (c.input_dim, c.hidden_dim, c.num_layers, c.output_dim) == self._COLOR_NET

    def _infer_fused(self, x, d):
        """Whether nerftex_curved_field_infer serves this call: _glue_fused(), the shapes the entry's kernels are built for (it refuses every
        other one), an fp16 table, and what the entry asks of its buffers.  Everything else goes through forward()."""
        return self._infer_static_back_ok(x) and self._infer_front_ok(x, d)  # (`_sigma_fused`: _glue_fused() has asked)

    def _infer_front_fused(self, x, d):
        """What the two fused chains ask alike (their front half, csrc/fieldglue.hip): fp16 autocast, no probabilistic table, the default texture
        table and sigma net, a batch of whole 128-row workgroups, contiguous fp32 inputs, an fp16 table."""
        return self._sigma_fused(x) and self._infer_front_ok(x, d)

    def _infer_front_ok(self, x, d):
        enc = self.encoder
        return (self._infer_rows_ok(x, d) and (enc.input_dim, enc.level_dim, enc.num_levels) == (3, 2, 8) and 1 <= self.projector.K <= 16
                and enc._table().dtype == torch.float16)

    def _infer_weights(self, attr, net2, more_stamp=(), more=None):
        """The 16-bit copies of the sigma net's and the entry's second network's weights, and what `more()` makes beside them: kept in the attribute
        `attr` between calls and re-made when a stamped version or address changes, as GridEncoder._table() and fused.ngp_field_infer keep theirs."""
        from gridencoder.grid import register_offsets

        ws, w2 = self.sigma_net._weights(), net2._weights()
        stamp = (ws._version, ws.data_ptr(), w2._version, w2.data_ptr()) + more_stamp
        cache = getattr(self, attr, None)
        if cache is None or cache[0] != stamp:
            register_offsets(self.encoder.offsets, self.encoder.num_levels)
            cache = (stamp, ws.detach().to(torch.float16), w2.detach().to(torch.float16)) + (more() if more else ())
            setattr(self, attr, cache)
        return cache[1:]

    # ---- the descriptors' member blocks: every member is written once, as a keyword argument of the block that owns it.  A descriptor is a composition
    # of blocks: a member named twice is a TypeError there, a member not named is ctypes' NULL / 0 (tests/test_curved_infer_members_cpu.py).

    def _infer_rows(self, x, d, live, sigma, rgbs, scratch, eval_bits=0):
        """What every descriptor has: the rows and the device count that bounds them (live = (int32 device tensor, rows per unit or code); None: all
        rows), outputs, scratch, fc_weight, eval = train / eval | eval_bits (static light: bit 1, tools/map.py:720's normalisation in the mid kernel)."""
        units, rows_per_unit = (ptr(live[0]), int(live[1])) if live is not None else (None, 0)
        return dict(xyz=ptr(x), dirs=ptr(d), B=x.shape[0], fc_weight=float(self.fc_weight), eval=eval_bits | int(not self.training), sigma=ptr(sigma),
                    rgbs=ptr(rgbs), units_dev=units, rows_per_unit=rows_per_unit, scratch=ptr(scratch), scratch_bytes=scratch.numel())

    def _infer_sigma_net(self, ws_h):
        s = self.sigma_net
        return dict(sigma_weights=ptr(ws_h), sigma_in=s.input_dim, sigma_hidden=s.hidden_dim, sigma_layers=s.num_layers, sigma_out=s.padded_output_dim)

    def _infer_static_back(self, x, d, live, sigma, rgbs, scratch):
        """Behind the front half or the lookup, the static light model's three descriptors alike -- sigma net, colour net, `_infer_rows` -- and the
        16-bit weights they point into."""
        c = self.color_net
        ws_h, wc_h = self._infer_weights("_infer_cache", c)
        return dict(color_weights=ptr(wc_h), color_in=c.input_dim, color_hidden=c.hidden_dim, color_layers=c.num_layers, color_out=c.output_dim,
                    **self._infer_sigma_net(ws_h), **self._infer_rows(x, d, live, sigma, rgbs, scratch, eval_bits=2)), (ws_h, wc_h)

    def _infer_lit_back(self, x, d, live, sigma, rgbs, scratch, shading_normal):
        """... and the SH light model's three: sigma net, the head -- the normal net's packed block, the BRDF net, the lighting, the flags and the
        output it shows (in training always "Full"), shading_normal (fp32 [B,3] or None) -- and `_infer_rows`; the weights and the lighting."""
        net = self.light_net
        br, env = net.brdf_layer, self._lighting().detach()
        ws_h, wb_h, nw, nb = self._infer_light_weights()
        mode = "Full" if self.training else self.light_visual_mode
        return dict(normal_weights=ptr(nw), normal_biases=ptr(nb), normal_hidden=16, normal_layers=2, brdf_weights=ptr(wb_h), brdf_in=br.input_dim,
                    brdf_hidden=br.hidden_dim, brdf_layers=br.num_layers, brdf_out=br.output_dim, env_shs=ptr(env), n_sh=env.shape[0], n_color=env.shape[1],
                    gamma=float(net.gamma), flags=SH_LIGHT_SPECULAR if net.use_specular else 0, visual_mode=LIGHT_VISUAL[mode],
                    shading_normal=ptr(shading_normal), **self._infer_sigma_net(ws_h), **self._infer_rows(x, d, live, sigma, rgbs, scratch)), (ws_h, wb_h, nw, nb, env)

    @staticmethod
    def _infer_mesh(p, K):
        """The neighbour search and the tracer over the projector p's mesh: the field's own, or the imported shape's."""
        return dict(knn=p._knn.value, tracer=p.tracer._handle.value, n_verts=p.mesh_vertices.shape[0], mesh_vertices=ptr(p.mesh_vertices),
                    vertex_normals=ptr(p.vertex_normals), K=K)

    def _infer_ladder(self, h_threshold):
        return dict(h_threshold=h_threshold, n_freqs=int(self.multires))

    def _infer_map(self, sdf_offset, h_threshold):
        """The imported feature map and the height it is read at: the planar and the shape chains' alike."""
        f = self.features_imported
        return dict(map=ptr(f), map_h=f.shape[0], map_w=f.shape[1], n_features=f.shape[2], sdf_offset=sdf_offset, **self._infer_ladder(h_threshold))

    def _infer_planar(self):
        mode, p0, p1, h0, h1, off, h = self._import_scalars()
        return dict(mode=mode, plane_scale0=p0, plane_scale1=p1, height_scale0=h0, height_scale1=h1, **self._infer_map(off, h))

    def _infer_shape(self):
        """The map on the imported mesh: the mesh, its per-face UVs, `_shape_scalars`."""
        K, scale, off, rate, h = self._shape_scalars()
        uv = self.shape_face_uv
        return dict(face_uv=ptr(uv), n_faces=uv.shape[0], sdf_scale=scale, uv_rate=rate, **self._infer_mesh(self.shape_projector, K), **self._infer_map(off, h))

    def _infer_patch(self):
        """The imported patch: its neighbour grid and records, the threshold and the ladder."""
        f = self.features_imported
        return dict(knn=self._patch_knn.value, n_points=f.shape[0], geom=ptr(self.patch_geom), features=ptr(f), n_features=f.shape[1],
                    **self._infer_ladder(float(self.h_threshold)))

    def _lit_maps(self):
        """The four maps the lit import chains read: the features and the three beside them."""
        return self.features_imported, self.phi_embed_imported, self.frame_map_imported, self.sample_inv_rows_imported

    def _infer_lit_maps(self):
        """The three maps the lit import chains read beside the features, and the four maps."""
        _, phi, frame, rows = maps = self._lit_maps()
        return dict(phi_map=ptr(phi), frame_map=ptr(frame), sample_tbn_inv=ptr(rows), n_phi=phi.shape[2], n_patches=rows.shape[0]), maps

    def _infer_unhash(self):
        """The features baked onto the fine mesh: the field's OWN neighbour grid and vertex arrays, the FINE mesh's tracer, arrays and rows,
        `_unhash_scalars`."""
        p, fv, table, f = self.projector, self.unhash_vertices, self.unhash_face_vertices, self.features_imported
        K, scale, off, h = self._unhash_scalars()
        return dict(knn=p._knn.value, tracer=self.unhash_tracer._handle.value, n_verts=p.mesh_vertices.shape[0], mesh_vertices=ptr(p.mesh_vertices),
                    vertex_normals=ptr(p.vertex_normals), K=K, dir_vec_wdist=0.05, fine_vertices=ptr(fv), n_fine_verts=fv.shape[0], face_vertices=ptr(table),
                    n_faces=table.shape[0], vertex_features=ptr(f), n_features=f.shape[1], sdf_scale=scale, sdf_offset=off, **self._infer_ladder(h))

    def _infer_lit_patch(self):
        """The lit records the lit patch chain reads beside the patch's own, and everything of the patch the call points into."""
        lit = self.patch_lit
        return dict(lit=ptr(lit), n_phi=self.patch_phi_embed.shape[1]), (self.features_imported, self.patch_geom, lit, self._patch_knn)

    def _infer_front_desc(self):
        """The front half's members of the two mesh-field descriptors, knn .. in_mul, and the 16-bit texture table they point into."""
        enc, p = self.encoder, self.projector
        table = enc._table()
        return dict(
            tbn=ptr(p.tbn), dir_vec_wdist=0.05, table=ptr(table), offsets=ptr(enc.offsets), D=int(enc.input_dim), C=int(enc.level_dim),
            L=int(enc.num_levels), S=float(np.log2(enc.per_level_scale)), H=int(enc.base_resolution), gridtype=int(enc.gridtype_id),
            align_corners=int(bool(enc.align_corners)), in_add=float(self.bound), in_mul=float(np.float32(1.0) / np.float32(2 * self.bound)),
            **self._infer_mesh(p, int(p.K)), **self._infer_ladder(p._height_limit(...))), table

    def _infer_desc(self, x, d, live, sigma, rgbs, scratch):
        """The nerftex_curved_infer_desc of one call (and the tensors it points into, to be kept until the call is enqueued)."""
        front, table = self._infer_front_desc()
        back, weights = self._infer_static_back(x, d, live, sigma, rgbs, scratch)
        return CurvedInferDesc(**front, **back), (table,) + weights

    def _infer_import_fused(self, x, d):
        """Whether nerftex_curved_import_infer (or, on an imported mesh, nerftex_curved_shape_infer) serves this call: _infer_fused()'s conditions
        without the neighbour search's and the table's."""
        return self._infer_static_back_ok(x) and self._infer_rows_ok(x, d) and self._on_device_of(x, self.features_imported)

    def _infer_import_desc(self, x, d, live, sigma, rgbs, scratch):
        """The nerftex_curved_import_infer_desc of one call (and the tensors it points into, to be kept until the call is enqueued)."""
        back, weights = self._infer_static_back(x, d, live, sigma, rgbs, scratch)
        return CurvedImportInferDesc(**self._infer_planar(), **back), (self.features_imported,) + weights

    def _infer_shape_desc(self, x, d, live, sigma, rgbs, scratch):
        """The nerftex_curved_shape_infer_desc of one call (and the tensors it points into, to be kept until the call is enqueued)."""
        back, weights = self._infer_static_back(x, d, live, sigma, rgbs, scratch)
        return CurvedShapeInferDesc(**self._infer_shape(), **back), (self.features_imported,) + weights

    def _infer_light_fused(self, x, d):
        """Whether nerftex_curved_light_infer serves this call: the SH light model with the switch `fused_light_infer` set (default: not), fp16
        autocast, the fused head (`light_net.fused`), no probabilistic table, the default shapes (the entry refuses every other one), no bounded
        angles, a visual mode the head has, fp16 tables, and what the entry asks of its buffers.  Everything else goes through forward()."""
        nn = self.normal_net
        return (self._infer_light_back_fused(x) and (nn.encoder.input_dim, nn.encoder.level_dim, nn.encoder.num_levels) == (3, 2, 4)
                and self._infer_front_fused(x, d) and nn.encoder._table().dtype == torch.float16)

    def _infer_light_back_fused(self, x):
        """What the two lit chains ask alike (the light mid, the BRDF net, the head): the switch, the fused head, the normal nets' and the BRDF
        net's default shapes, no bounded angles, a visual mode the head has, fp32 lighting of 1 or 3 colours."""
        if not (getattr(self, "light_model", None) == "SH" and getattr(self, "fused_light_infer", False)):
            return False
        nn, net = self.normal_net, self.light_net
        probe, rot = self._per_probe_lighting(), self._light_rotation_active()
        if probe or rot:
            # per-probe lighting and the rotation are the _relit entries' (DESIGN.md 4.23), opt-in: without `fused_relight_infer` they are forward()'s,
            # as is per-probe lighting without its tables (forward() raises there: the chain must not render it)
            if not getattr(self, "fused_relight_infer", False):
                return False
            if probe and (net.envSHs_import_vis is None or net.probes is None or not self._on_device_of(x, net.envSHs_import_vis, net.probes)):
                return False
            if rot and not self._on_device_of(x, self._light_rotation):
                return False
        br, env = net.brdf_layer, self._lighting()
        return (bool(net.fused) and nn is not None and not nn.bound_output and (self.training or self.light_visual_mode in LIGHT_VISUAL)
                and x.is_cuda and br.dtype == torch.float16 and (br.input_dim, br.hidden_dim, br.num_layers, br.output_dim) == self._BRDF_NET
                and (nn.low_freq_band_len_x, nn.low_freq_band_len_z) == (16, 12)
                and [tuple(l.W.shape) for l in nn.phi_net.layers] == [(16, 20), (16, 16), (1, 16)]
                and [tuple(l.W.shape) for l in nn.theta_net.layers] == [(16, 28), (16, 16), (1, 16)]
                and env.shape[0] >= 9 and env.shape[1] in (1, 3) and env.dtype == torch.float32)

    def _infer_light_import_fused(self, x, d):
        """Whether nerftex_curved_light_import_infer serves this call: _infer_light_fused()'s conditions without the neighbour search's and the
        two tables', with the imported maps on x's device instead."""
        return (getattr(self, "imported", False) and self._infer_light_back_fused(x) and self._import_light_fused(x) and self._infer_rows_ok(x, d)
                and self._on_device_of(x, *self._lit_maps()))

    def _infer_light_shape_fused(self, x, d):
        """Whether nerftex_curved_light_shape_infer serves this call: _infer_light_import_fused()'s conditions over the maps on the imported mesh,
        with its frames and a K the neighbour search serves."""
        return (self._infer_light_back_fused(x) and self._shape_light_fused(x) and self._infer_rows_ok(x, d) and 1 <= self._shape_scalars()[0] <= 16
                and self._on_device_of(x, *self._lit_maps(), self.shape_face_uv, self.shape_face_tbn))

    def _infer_patch_fused(self, x, d):
        """Whether nerftex_curved_patch_infer serves this call: an imported patch, and _infer_import_fused()'s conditions over it."""
        return self._patch_fused(x) and self._infer_static_back_ok(x) and self._infer_rows_ok(x, d)

    def _infer_light_patch_fused(self, x, d):
        """Whether nerftex_curved_light_patch_infer serves this call: an imported patch with its lit records, and
        _infer_light_import_fused()'s conditions over it."""
        return (self._infer_light_back_fused(x) and self._patch_fused(x) and self.patch_lit is not None and self._infer_rows_ok(x, d)
                and self._on_device_of(x, self.patch_lit))

    def _infer_unhash_fused(self, x, d):
        """Whether nerftex_curved_unhash_infer serves this call: features baked onto a fine mesh, and _infer_import_fused()'s conditions over them."""
        return self._unhash_fused(x) and self._infer_static_back_ok(x) and self._infer_rows_ok(x, d)

    def _infer_unhash_desc(self, x, d, live, sigma, rgbs, scratch):
        """The nerftex_curved_unhash_infer_desc of one call (and the tensors it points into, to be kept until the call is enqueued)."""
        back, weights = self._infer_static_back(x, d, live, sigma, rgbs, scratch)
        return CurvedUnhashInferDesc(**self._infer_unhash(), **back), (self.features_imported, self.unhash_vertices, self.unhash_face_vertices, self.unhash_tracer) + weights

    def _infer_patch_desc(self, x, d, live, sigma, rgbs, scratch):
        """The nerftex_curved_patch_infer_desc of one call (and the tensors it points into, to be kept until the call is enqueued)."""
        back, weights = self._infer_static_back(x, d, live, sigma, rgbs, scratch)
        return CurvedPatchInferDesc(**self._infer_patch(), **back), (self.features_imported, self.patch_geom, self._patch_knn) + weights

    def _infer_light_patch_desc(self, x, d, live, sigma, rgbs, scratch, shading_normal=None):
        """The nerftex_curved_light_patch_infer_desc of one call (and the tensors it points into, to be kept until the call is enqueued)."""
        lit, records = self._infer_lit_patch()
        back, kept = self._infer_lit_back(x, d, live, sigma, rgbs, scratch, shading_normal)
        return CurvedLightPatchInferDesc(**self._infer_patch(), **lit, **back), records + kept

    def _infer_light_desc(self, x, d, live, sigma, rgbs, scratch, shading_normal=None):
        """The nerftex_curved_light_infer_desc of one call (and the tensors it points into).  Kept between calls and re-made when a parameter
        changes: the 16-bit MLP weights, and the normal net's packed block -- every LipLayer's normalization().half(), which is what the
        framework's half GEMM multiplies with under autocast, and its fp32 biases, in the order include/nerftex_hip.h gives."""
        nenc = self.normal_net.encoder
        ntable = nenc._table()
        front, table = self._infer_front_desc()
        back, kept = self._infer_lit_back(x, d, live, sigma, rgbs, scratch, shading_normal)
        desc = CurvedLightInferDesc(
            normal_table=ptr(ntable), normal_offsets=ptr(nenc.offsets), normal_C=int(nenc.level_dim), normal_L=int(nenc.num_levels),
            normal_S=float(np.log2(nenc.per_level_scale)), normal_H=int(nenc.base_resolution), normal_gridtype=int(nenc.gridtype_id),
            normal_align_corners=int(bool(nenc.align_corners)), normal_in_add=1.0, normal_in_mul=float(np.float32(1.0) / np.float32(2)),  # (encoder(p_sur): bound 1)
            **front, **back)
        return desc, (table, ntable) + kept

    def _infer_light_weights(self):
        """-> (sigma net, BRDF net: 16-bit weights; the normal net's packed block: half weights, fp32 biases) of the two lit chains, kept between
        calls (`_infer_weights`)."""
        from gridencoder.grid import register_offsets

        nn = self.normal_net
        nenc = nn.encoder
        layers = list(nn.phi_net.layers) + list(nn.theta_net.layers)

        def normal_block():
            register_offsets(nenc.offsets, nenc.num_levels)
            with torch.autocast("cuda", enabled=False):
                nw = torch.cat([l.normalization().detach().float().half().reshape(-1) for l in layers]).contiguous()
                nb = torch.cat([l.b.detach().float().reshape(-1) for l in layers]).contiguous()
            return nw, nb

        return self._infer_weights("_infer_light_cache", self.light_net.brdf_layer, (tuple((q.data_ptr(), q._version) for l in layers for q in (l.W, l.b, l.c)),),
                                   normal_block)

    def _infer_light_import_desc(self, x, d, live, sigma, rgbs, scratch, shading_normal=None):
        """The nerftex_curved_light_import_infer_desc of one call (and the tensors it points into, to be kept until the call is enqueued)."""
        lit, maps = self._infer_lit_maps()
        back, kept = self._infer_lit_back(x, d, live, sigma, rgbs, scratch, shading_normal)
        return CurvedLightImportInferDesc(**self._infer_planar(), **lit, **back), maps + kept

    def _infer_light_shape_desc(self, x, d, live, sigma, rgbs, scratch, shading_normal=None):
        """The nerftex_curved_light_shape_infer_desc of one call (and the tensors it points into, to be kept until the call is enqueued)."""
        lit, maps = self._infer_lit_maps()
        back, kept = self._infer_lit_back(x, d, live, sigma, rgbs, scratch, shading_normal)
        frames = self.shape_face_tbn  # (the new mesh's)
        return CurvedLightShapeInferDesc(face_tbn=ptr(frames), n_tbn_faces=frames.shape[0], **self._infer_shape(), **lit, **back), maps + kept

    def _infer_call(self, entry, make_desc, x, d, live, *more):
        """One call of the library entry `entry` (its scratch query is `entry`_scratch_bytes) over the descriptor make_desc builds: -> (sigma [B],
        rgbs [B,3]), fp32 views of one allocation.  The scratch is one buffer per stream (the ray ranges of a pipelined frame run side by side),
        grown to the largest batch seen: the loop's batch size changes with nearly every iteration.  A buffer that is replaced goes back to the
        allocator, which hands it out again only behind the work this stream still has queued on it.  Under a graph capture: a fresh one (the
        graph's pool keeps it)."""
        import ctypes

        from nerftex_hip import check, lib, stream

        B, st = x.shape[0], stream()
        nbytes = getattr(lib, entry + "_scratch_bytes")(B)
        if torch.cuda.is_current_stream_capturing():
            scratch = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
        else:
            held = getattr(self, "_infer_scratch", None)
            if held is None:
                held = self._infer_scratch = {}
            scratch = held.get((x.device, st))
            if scratch is None or scratch.numel() < nbytes:
                scratch = held[(x.device, st)] = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
        out = torch.empty(4 * B, dtype=torch.float32, device=x.device)  # [sigma | rgb] in one allocation
        sigma, rgbs = out[:B], out[B:].view(B, 3)
        desc, _keep = make_desc(x, d, live, sigma, rgbs, scratch, *more)
        relight = self._relight_desc() if getattr(self, "light_model", None) == "SH" and hasattr(desc, "env_shs") else None
        if relight is None:
            check(getattr(lib, entry)(ctypes.byref(desc), st))
        else:  # (per-probe lighting or a rotation in effect: the lit chain's _relit entry, the same scratch)
            check(getattr(lib, entry + "_relit")(ctypes.byref(desc), ctypes.byref(relight[0]), st))
        return sigma, rgbs

    @torch.no_grad()
    def infer_light(self, x, d, live=None, shading_normal=None):
        """infer() of the SH-lit field through nerftex_curved_light_infer (see `_infer_light_fused`, which the caller has checked);
        shading_normal: an fp32 [B,3] tensor that receives the normal the head shades with."""
        return self._infer_call("nerftex_curved_light_infer", self._infer_light_desc, x, d, live, shading_normal)

    @torch.no_grad()
    def infer_light_import(self, x, d, live=None, shading_normal=None):
        """infer() of the SH-lit field over its imported maps through nerftex_curved_light_import_infer (see `_infer_light_import_fused`, which
        the caller has checked)."""
        return self._infer_call("nerftex_curved_light_import_infer", self._infer_light_import_desc, x, d, live, shading_normal)

    @torch.no_grad()
    def infer_light_shape(self, x, d, live=None, shading_normal=None):
        """infer() of the SH-lit field over its imported maps on the imported mesh through nerftex_curved_light_shape_infer (see
        `_infer_light_shape_fused`, which the caller has checked)."""
        return self._infer_call("nerftex_curved_light_shape_infer", self._infer_light_shape_desc, x, d, live, shading_normal)

    # The one priority table of the nine chains: (the sources a row serves, its predicate, the library entry, the builder of its descriptor, lit).
    # The first row of the ACTIVE source whose predicate holds serves the call.  A source sees its own rows only: an imported patch never takes a
    # map's chain (the maps of an earlier import_field are not this import's), an import never the mesh field's.  Patch: DESIGN.md 4.20; the maps:
    # 4.18, 4.17, 4.16, 4.15 (the lit planar row serves either map source: its predicate refuses the imported mesh); the mesh field: lit (4.14, opt-in:
    # `fused_light_infer`), static; the features baked onto a fine mesh (static light only): 4.25.  The predicates are looked up by name: the tests
    # substitute them.
    _INFER_ROUTES = (
        (("mesh",), "_infer_light_fused", "nerftex_curved_light_infer", "_infer_light_desc", True),
        (("mesh",), "_infer_fused", "nerftex_curved_field_infer", "_infer_desc", False),
        (("patch",), "_infer_light_patch_fused", "nerftex_curved_light_patch_infer", "_infer_light_patch_desc", True),
        (("patch",), "_infer_patch_fused", "nerftex_curved_patch_infer", "_infer_patch_desc", False),
        (("shape",), "_infer_light_shape_fused", "nerftex_curved_light_shape_infer", "_infer_light_shape_desc", True),
        (("field", "shape"), "_infer_light_import_fused", "nerftex_curved_light_import_infer", "_infer_light_import_desc", True),
        (("shape",), "_infer_import_fused", "nerftex_curved_shape_infer", "_infer_shape_desc", False),
        (("field",), "_infer_import_fused", "nerftex_curved_import_infer", "_infer_import_desc", False),
        (("unhash",), "_infer_unhash_fused", "nerftex_curved_unhash_infer", "_infer_unhash_desc", False),
    )

    def _infer_row(self, x, d):
        """The row of `_INFER_ROUTES` that serves infer(x, d), or None: forward()."""
        source = getattr(self, "imported_type", None) if getattr(self, "imported", False) else "mesh"
        for row in self._INFER_ROUTES:
            if source in row[0] and getattr(self, row[1])(x, d):
                return row
        return None

    def _infer_route(self, x, d):
        """The chain that serves infer(x, d): (the library entry's name, the builder of its descriptor), or None: forward()."""
        row = self._infer_row(x, d)
        return None if row is None else (row[2], getattr(self, row[3]))

    @torch.no_grad()
    def infer_padded(self, x, d):
        """infer(x, d) for a batch of ANY size (the reference loop's iterations, Renderer.render_infer): where the light model's fused chain
        applies but for the batch's size, the batch is padded to the next multiple of 128 with marked slots (which cost nothing) -- every
        sample then has the bits the device-count loops give it, whatever iteration it falls into."""
        B = x.shape[0]
        pad = -B % 128
        if pad and B and getattr(self, "fused_light_infer", False):
            xp = torch.full((B + pad, 3), 1e30, dtype=x.dtype, device=x.device)
            dp = torch.full((B + pad, 3), 1e30, dtype=d.dtype, device=d.device)
            xp[:B], dp[:B] = x, d
            row = self._infer_row(xp, dp)
            if row is not None and row[4]:  # (the lit chains only)
                sigma, rgbs = self._infer_call(row[2], getattr(self, row[3]), xp, dp, None)
                return sigma[:B], rgbs[:B]
        return self.infer(x, d)

    @torch.no_grad()
    def infer(self, x, d, live=None):
        """(sigma fp32 [B], rgbs fp32 [B,3]) of forward(x, d) without an autograd node: the whole chain as ONE library call
        (nerftex_curved_field_infer) in the device-count form a renderer's inference iteration needs -- live = (int32 device tensor, rows per
        unit or NERFTEX_ROWS_AUTO code): rows past live[0][0] * rows per unit are not touched, the slots the march marked unused (direction 1e30)
        cost no neighbour search, no traversal and no table read and come out as exactly 0; every other row holds forward()'s values, bit for
        bit.  The scratch is one buffer per stream, grown to the largest batch seen (under a graph capture: the graph's pool keeps it).
        Where the fused chain does not apply (no fp16 autocast, prob_model, other shapes, fused_glue = False, a batch that is no multiple of
        128) this is forward(x, d) on all rows, cast to fp32: slower, the same image.
        light_model="SH": forward(x, d) on all rows unless `fused_light_infer` is set (default False) -- then the light model's own chain,
        nerftex_curved_light_infer, under the same rows contract: sigma and the mask are forward()'s bit for bit, the shading normal and the
        colour follow forward()'s arithmetic at its rounding points; over imported maps, nerftex_curved_light_import_infer
        (DESIGN.md 4.17), and over the maps on an imported mesh nerftex_curved_light_shape_infer.  The lit chains shade with
        light_net.lighting(), so a uniform imported lighting goes through them; per-probe lighting (`shade_visibility` with an imported
        lighting in eval) is forward()'s, and so is a lighting rotation (set_light_rotation) -- unless `fused_relight_infer` is
        set (default False): then the chain's _relit entry shades with the probe tables and the rotation.
        An imported patch (import_patch): nerftex_curved_patch_infer, and for the SH-lit field with the switch set
        nerftex_curved_light_patch_infer, under the same contract.  The field baked onto a fine mesh (unhash,
        import_unhash_vertices): nerftex_curved_unhash_infer."""
        row = self._infer_row(x, d)
        if row is None:
            sigma, rgbs, _ = self.forward(x, d)
            return sigma.float(), rgbs.float()
        return self._infer_call(row[2], getattr(self, row[3]), x, d, live)

    @torch.no_grad()
    def forward_graphed(self, x, d):
        """The no-grad forward (a renderer's inference iteration, the occupancy update's query) as ONE replayed HIP graph (round 6):
        neighbour search, projector, hash-grid lookup, the two FFMLPs and the ~25 framework ops between them (normalisations, the reflected view
        direction, pads, concatenations, masks) are recorded once for this shape and replayed -- the kernels were 609 of the 919 us a call took, the
        rest was the host getting ~40 launches out.  x, d [N, 3] are copied into the graph's static inputs; the returned (sigma, color) are the
        graph's static outputs: valid until the next call.  Same values as forward() (tests/test_gpu_round6.py).  Re-recorded when N, the autocast
        state, train / eval or a parameter changes."""
        from .streams import capture_section

        x, d = x.contiguous().float(), d.contiguous().float()
        stamp = (tuple(x.shape), tuple(d.shape), self.training, torch.is_autocast_enabled(), torch.get_autocast_dtype("cuda"),
                 tuple((p.data_ptr(), p._version) for p in self.parameters()))
        st = getattr(self, "_fwd_graph", None)
        if st is None or st["stamp"] != stamp:
            xs, ds = x.clone(), d.clone()
            for _ in range(2):  # lazy initialisation (level-table registration, workspaces, cached 16-bit weights) outside the capture
                self.forward(xs, ds)
            torch.cuda.synchronize()
            with capture_section():
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g, capture_error_mode="thread_local"):
                    sigma, color, _ = self.forward(xs, ds)
            st = self._fwd_graph = {"stamp": stamp, "x": xs, "d": ds, "graph": g, "out": (sigma, color)}
        st["x"].copy_(x, non_blocking=True), st["d"].copy_(d, non_blocking=True)
        st["graph"].replay()
        return st["out"][0], st["out"][1], {}

    def regular_loss(self, lip_weight=0.0):
        """tools/map.py:770-774; lip_weight: network_curvedfield.py:225-227 adds 1e-4 * normal_net.regularization() when the light model renders."""
        loss = 1e-8 * self.encoder.clustering_loss()
        if lip_weight and self.normal_net is not None:
            loss = loss + lip_weight * self.normal_net.regularization()
        return loss

    def get_params(self, lr):
        return [{"params": self.parameters(), "lr": lr}]
