"""TEST INFRASTRUCTURE: tests/import_light_float64.py's fine-normal chain for imported maps on a NEW UV-mapped mesh (the `pred_normal` part of the
'shape' branch of MeshFeatureField.forward, tools/map.py:693-707, :722-730), in float64 with the same running per-element bound, for
tests/test_import_shape_light_cpu.py and tests/test_gpu_import_shape_light.py.  Plain numpy.  It imports shape_float64, import_light_float64
and normal_net_float64 unchanged and adds what the branch adds: the local normal is rotated a THIRD time, by the hit face's frame of the new
mesh, the same half product as the other two:

    rotation 3  n3_a = half(sum_b half(F3[b, a]) half(n2_b))                F3 = tbn[face] of the new mesh; half(n2) = n2
    normalise   twice; eval: the blend with the new mesh's coarse normal normalised twice; normalise

THE ERROR MODEL is import_light_float64's, with one more rotation term of the form it gives the second rotation:
    |F3| err_in + 2 u mag + 2 UH |s| + SUB,   err_in = err(n2) + 2 UH |n2| + SUB
and the coarse normal of the blend is the lookup's raw normal (normal_net_float64's `coarse_raw` rule) instead of (0, 0, 1).

It also holds the float64 statement of the per-face frames (calculate_tbn, tools/map.py:119-138): `uv_face_frames`.
"""
import numpy as np

import import_light_float64 as il64
import normal_net_float64 as nn64
import shape_float64 as sf  # noqa: F401  (the meshes and cases the two tests take from it)

U, UH, SUB = nn64.U, nn64.UH, nn64.SUB
_half = nn64._half

MUTANTS = ("no_third", "third_transposed", "frames_multiplied", "bvh_position")


def uv_face_frames(vertices, faces, uvs):
    """Per face, everything in float64: [t; b] = inv(UV edges) (3-D edges), with 1e-3 added to element [1, 1] of EVERY matrix of rank < 2 (numpy's
    SVD rank with its default tolerance, as the reference asks for it); n = the normalised cross product of the first two edges; b = n x t; rows
    normalised.  -> [F, 3, 3] float64."""
    v, f, uv = np.asarray(vertices, np.float64), np.asarray(faces).astype(np.int64), np.asarray(uvs, np.float64)
    e3 = v[f][:, 1:] - v[f][:, :1]
    e2 = uv[f][:, 1:] - uv[f][:, :1]
    rank = np.linalg.matrix_rank(e2)
    e2[rank < 2, 1, 1] += 1e-3
    det = e2[:, 0, 0] * e2[:, 1, 1] - e2[:, 0, 1] * e2[:, 1, 0]
    inv = np.stack([np.stack([e2[:, 1, 1], -e2[:, 0, 1]], -1), np.stack([-e2[:, 1, 0], e2[:, 0, 0]], -1)], -2) / det[:, None, None]
    t = inv[:, 0, 0, None] * e3[:, 0] + inv[:, 0, 1, None] * e3[:, 1]
    n = np.cross(e3[:, 0], e3[:, 1])
    n /= np.linalg.norm(n, axis=-1, keepdims=True)
    b = np.cross(n, t)
    out = np.stack([t, b, n], 1)
    return out / np.linalg.norm(out, axis=-1, keepdims=True)


def frames_bar(vertices, faces, uvs):
    """The bar on |fp32 frame - float64 frame| per face when the UV edges are FP32 and their rank and inverse numpy's fp32 ones (what the
    reference's call hands over): the float64 result rounds to fp32 within 2^-24 per component (the rows are unit vectors), and the fp32
    inverse carries a relative error of a few fp32 roundings times the matrix's condition number into the direction of t (b = n x t follows
    t; n does not depend on the UVs).  bar = 2^-24 + 16 * 2^-24 * cond(UV edges), per face."""
    f, uv = np.asarray(faces).astype(np.int64), np.asarray(uvs, np.float64)
    e2 = uv[f][:, 1:] - uv[f][:, :1]
    rank = np.linalg.matrix_rank(e2)
    e2[rank < 2, 1, 1] += 1e-3
    return U + 16 * U * np.linalg.cond(e2)


def padded_table(frames):
    """CurvedField.shape_face_tbn of [F, 3, 3] frames: [F', 12] fp32, nine floats and three zeros per face, eight zero rows behind a mesh of at
    most eight faces (where the tracer pads its BVH and import_shape the UV table)."""
    F = len(frames)
    out = np.zeros((F + (8 if F <= 8 else 0), 12), np.float32)
    out[:F, :9] = np.asarray(frames, np.float32).reshape(F, 9)
    return out


def fine_normal(phi_feat, x_feat, z, weights, biases, local_tbn, sample_tbn_inv, new_tbn, coarse_raw=None, fc_weight=1.0, blend=False, fp32_inputs=False,
                dweights=None, mutate=None):
    """il64.fine_normal with the third rotation by new_tbn [B,3,3] and, in the blend, the raw coarse normal [B,3] of the new mesh.
    mutate: one of MUTANTS (a deliberately wrong third rotation; "bvh_position" is the caller's, who hands over other frames).
    -> dict(local, bound_local, fine, bound_fine, normal, bound_normal)."""
    base = il64.fine_normal(phi_feat, x_feat, z, weights, biases, local_tbn, sample_tbn_inv, fp32_inputs=fp32_inputs, dweights=dweights)
    local, e_local = base["local"], base["bound_local"]
    n1, e1 = il64._rotate(local_tbn, _half(local), e_local + 2 * UH * np.abs(local) + SUB, fp32_inputs)
    if mutate == "frames_multiplied":  # one rotation by the product of the second and third frames, rounded once
        F2, F3 = (np.asarray(a, np.float64).reshape(-1, 3, 3) for a in (sample_tbn_inv, new_tbn))
        n3, e3 = il64._rotate(np.einsum("nbc,nca->nba", F2, F3), n1, e1 + 2 * UH * np.abs(n1) + SUB, True)
    else:
        n2, e2 = il64._rotate(sample_tbn_inv, n1, e1 + 2 * UH * np.abs(n1) + SUB, fp32_inputs)
        if mutate == "no_third":
            n3, e3 = n2, e2
        else:
            F3 = np.asarray(new_tbn, np.float64).reshape(-1, 3, 3)
            n3, e3 = il64._rotate(F3.transpose(0, 2, 1) if mutate == "third_transposed" else F3, n2, e2 + 2 * UH * np.abs(n2) + SUB, fp32_inputs)
    fine, e_fine = nn64._unit(n3, e3)
    n, e_n = nn64._unit(fine, e_fine)
    if blend:
        fc = float(np.float32(fc_weight))
        c, e_c = nn64._unit(np.asarray(coarse_raw, np.float64), np.zeros(n.shape))
        c, e_c = nn64._unit(c, e_c)
        s = fc * n + (1 - fc) * c
        e_s = abs(fc) * e_n + abs(1 - fc) * e_c + U * (np.abs(fc * n) + 2 * np.abs((1 - fc) * c) + np.abs(s))
        n, e_n = nn64._unit(s, e_s)
    return dict(local=local, bound_local=e_local, fine=fine, bound_fine=e_fine, normal=n, bound_normal=e_n)


def rotate_half(frames, v):
    """einsum('nba,nb->na') as the GPU's half product evaluates it: both operands rounded to half, fp32 products and sums in ascending b, the
    result rounded to half.  An emulation of the arithmetic in numpy (fp32 scalars), independent of `_rotate`'s float64 statement."""
    F = np.asarray(frames, np.float32).reshape(-1, 3, 3).astype(np.float16).astype(np.float32)
    h = np.asarray(v, np.float32).astype(np.float16).astype(np.float32)
    s = (F[:, 0] * h[:, 0:1] + F[:, 1] * h[:, 1:2]).astype(np.float32) + F[:, 2] * h[:, 2:3]
    return s.astype(np.float32).astype(np.float16).astype(np.float32)
